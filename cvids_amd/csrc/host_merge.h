// host_merge.h -- chisel_hip_merge_map (included by chisel_hip.hip; the kernels and the definition: kernels_merge.h; the
// frame it shares with the other entries that rewrite a map: host_rewrite.h).
// Everything runs on the destination's stream, ordered behind what the source has queued and in front of what it queues next, with the
// events behind chisel_hip_order_stream_after_map.  One host wait: the number of candidate chunks and how many of them the destination
// lacks, from which the pool and the grids are sized -- and from which a fixed pool that cannot take them refuses, before the first
// chunk is created.  The scratch lives in the destination (chisel_hip_map::merge_mem), is sized from the source's chunk count, reused
// by the next merge and freed with the map.
#pragma once

namespace {

// `waiter` starts what it is given next after what `m` has queued so far (chisel_hip_order_stream_after_map's event)
int order_after_map(chisel_hip_map *m, hipStream_t waiter) {
    if (!m->order_events[0]) HIP_TRY(hipEventCreateWithFlags(&m->order_events[0], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(m->order_events[0], m->stream));
    HIP_TRY(hipStreamWaitEvent(waiter, m->order_events[0], 0));
    return CHISEL_HIP_OK;
}

// room for `chunks` source chunks: a key table of twice the ids they can list (27 each), the list and the per-entry slots
int ensure_merge_scratch(chisel_hip_map *dst, int64_t chunks) {
    chisel_hip_map::MergeMemory &O = dst->merge_mem;
    MergeView &G = O.view;
    if (!O.host) {
        HIP_TRY(O.host.alloc(16));
        HIP_TRY(alloc_viewed(O.ctl, G.ctl, (size_t)MG_INTS));
        HIP_TRY(alloc_viewed(O.stats, G.stats, (size_t)MS_WORDS));
    }
    uint64_t want = 1024;
    while (want < 2ull * 27ull * (uint64_t)std::max<int64_t>(chunks, 1)) want *= 2;
    if (want > (1ull << 30)) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_merge_map: the source holds more chunks than one merge lists");
    if (want <= G.table_capacity) return CHISEL_HIP_OK;
    G.table_capacity = 0;
    const int rc = grow_buffer(O.table, (size_t)want, dst->stream, &G.table);  // (waits for the stream: nothing reads the other two any more)
    if (rc) return rc;
    HIP_TRY(alloc_viewed(O.list, G.list, (size_t)want / 2));
    HIP_TRY(alloc_viewed(O.slots, G.slots, (size_t)want / 2));
    G.table_capacity = (unsigned)want;
    return CHISEL_HIP_OK;
}

// M = the inverse of src_to_dst taken as rigid (R^T, -R^T t), in double, products and sums left to right, each entry rounded to fp32;
// and the affine inverse of THAT matrix in double (cofactors), which the candidate boxes go by
void merge_transform(const float *a, MergeTransform &T, double pad) {
    double R[9], t[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)a[4 * i + j];
        t[i] = (double)a[4 * i + 3];
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T.m[4 * i + j] = (float)R[3 * j + i];
        T.m[4 * i + 3] = (float)(-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]));
    }
    double m[12];
    for (int i = 0; i < 12; i++) m[i] = (double)T.m[i];
    auto at = [&](int i, int j) { return m[4 * i + j]; };
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return at(i1, j1) * at(i2, j2) - at(i1, j2) * at(i2, j1);
    };
    const double det = at(0, 0) * cof(0, 0) + at(0, 1) * cof(0, 1) + at(0, 2) * cof(0, 2);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T.f[4 * i + j] = cof(j, i) / det;
        T.f[4 * i + 3] = 0.0;
    }
    for (int i = 0; i < 3; i++) T.f[4 * i + 3] = -((T.f[4 * i] * m[3] + T.f[4 * i + 1] * m[7]) + T.f[4 * i + 2] * m[11]);
    T.pad = pad;
}

template <int N>
void launch_merge_gather(chisel_hip_map *dst, chisel_hip_map *src, const MeshParams &P, const MergeView &G, const MergeTransform &T, int n) {
    if (dst->cfg.use_color && src->cfg.use_color)
        hipLaunchKernelGGL((merge_gather_kernel<N, true>), dim3(n), dim3(256), 0, dst->stream, dst->view, src->view, P, G, T, n);
    else
        hipLaunchKernelGGL((merge_gather_kernel<N, false>), dim3(n), dim3(256), 0, dst->stream, dst->view, src->view, P, G, T, n);
}

}  // namespace

extern "C" int chisel_hip_merge_map(chisel_hip_map *dst, chisel_hip_map *src, const float src_to_dst[12], chisel_hip_merge_stats *stats) {
    static_assert(sizeof(chisel_hip_merge_stats) == 32, "chisel_hip_merge_stats is four 64-bit counts");
    // ---- refusals: nothing of either map is touched by a refused call
    if (!dst || !src || !src_to_dst) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: null argument");
    if (dst == src) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: a map cannot be merged into itself");
    if (dst->is_group || src->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_merge_map reads and writes the voxels of all owners: a group's shards hold a part each (merge maps of one shard)");
    if (dst->cfg.n_shards > 1 || src->cfg.n_shards > 1) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_merge_map reads and writes the voxels of all owners: one of the maps is one shard of several");
    if (dst->device != src->device) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: the maps live on different devices");
    if (dst->N != src->N || memcmp(&dst->cfg.voxel_resolution, &src->cfg.voxel_resolution, sizeof(float)) != 0)
        return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: the maps differ in chunk size or voxel resolution");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(src_to_dst[i])) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: src_to_dst has an entry that is not finite");
    {
        double worst = 0.0;  // max |R^T R - I|, in double
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s += (double)src_to_dst[4 * k + i] * (double)src_to_dst[4 * k + j];
                worst = std::max(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
            }
        if (!(worst <= 1e-4)) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_merge_map: the rotation part of src_to_dst is not a rotation (max |R^T R - I| > 1e-4)");
    }
    int rc = rewrite_begin(dst);
    if (rc) return rc;
    rc = rewrite_begin(src);  // (the source is only read; the same holds for it)
    if (rc) return rc;

    // ---- the candidates (read-only for both maps)
    rc = ensure_merge_scratch(dst, std::min<int64_t>(src->view.committed, std::max<int64_t>(dst->merge_mem.chunks_hint, 1024)));
    if (rc) return rc;
    rc = wait_for_input(dst, dst->stream);  // chisel_hip_wait_event / _order_map_after_stream on the destination
    if (rc) return rc;
    rc = wait_for_input(src, dst->stream);  // ... and on the source: what it was told to wait for, its reader waits for
    if (rc) return rc;
    rc = order_after_map(src, dst->stream);  // behind everything queued on the source's stream
    if (rc) return rc;
    chisel_hip_map::MergeMemory &O = dst->merge_mem;
    MergeTransform T;
    merge_transform(src_to_dst, T, (double)dst->cfg.voxel_resolution);
    const double edge = (double)dst->N * (double)dst->cfg.voxel_resolution;
    volatile int *words = O.host.get();
    for (int attempt = 0;; attempt++) {
        const MergeView &G = O.view;
        HIP_TRY(hipMemsetAsync(G.table, 0xff, (size_t)G.table_capacity * sizeof(unsigned long long), dst->stream));
        HIP_TRY(hipMemsetAsync(G.ctl, 0, MG_INTS * sizeof(int), dst->stream));
        HIP_TRY(hipMemsetAsync(G.stats, 0, MS_WORDS * sizeof(unsigned long long), dst->stream));
        hipLaunchKernelGGL(merge_candidates_kernel, dim3((src->view.committed + 255) / 256), dim3(256), 0, dst->stream, src->view, G, T, edge);
        hipLaunchKernelGGL(merge_classify_kernel, dim3(G.table_capacity / 2 / 256), dim3(256), 0, dst->stream, dst->view, G);
        hipLaunchKernelGGL(report_words_kernel<int>, dim3(1), dim3(1), 0, dst->stream, (const int *)G.ctl, O.host.dev(), MG_INTS);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(dst->stream));  // the one wait of a merge
        note_stream_idle(dst);
        std::atomic_thread_fence(std::memory_order_acquire);
        O.chunks_hint = words[MG_SRC_CHUNKS];
        if (!words[MG_OVERFLOW]) break;
        if (attempt) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_merge_map: more candidate chunks than the source's chunks can list");
        rc = ensure_merge_scratch(dst, std::max<int64_t>(words[MG_SRC_CHUNKS], 8 * (int64_t)O.view.table_capacity / 54));  // (sized from the true count, and again)
        if (rc) return rc;
    }
    const MergeView G = O.view;
    const int n_unique = words[MG_UNIQUE], n_absent = words[MG_ABSENT], n_src = words[MG_SRC_CHUNKS], n_free = words[MG_DST_FREE];
    if (stats) *stats = chisel_hip_merge_stats{n_src, 0, 0, 0};
    auto release_source = [&]() { return order_after_map(dst, src->stream); };  // the source's next call starts behind the reads
    if (n_unique == 0) return release_source();

    // ---- the pool: decided before the first chunk is created
    if (n_absent > n_free) {
        const int64_t want = (int64_t)dst->view.committed + (n_absent - n_free);
        if (!dst->growable || want > dst->view.max_chunks) {
            (void)release_source();
            return fail(CHISEL_HIP_ERR_POOL_FULL, "chisel_hip_merge_map: the destination's chunk pool cannot take the chunks the source may create: raise chisel_hip_config.max_chunks");
        }
    }
    if (dst->growable) {  // (as a point cloud or a map load makes room; and a quarter of the pool free afterwards, for the integration that follows)
        const int64_t used_after = (int64_t)dst->view.committed - n_free + n_absent;
        if (n_absent > n_free || (int64_t)dst->view.committed - used_after < (int64_t)dst->view.committed / 4) {
            const int before = dst->view.committed;
            rc = grow_pool(dst, std::max<int64_t>(2 * (int64_t)dst->view.committed, used_after + used_after / 2));
            if (rc) return rc;
            if ((int64_t)(dst->view.committed - before) + n_free < n_absent) {
                (void)release_source();
                return fail(CHISEL_HIP_ERR_POOL_FULL, "chisel_hip_merge_map: the destination's chunk pool is at its limit");
            }
        }
    }

    // ---- create, gather, bookkeeping
    if (n_absent > 0) {
        dst->topology_epoch++;
        hipLaunchKernelGGL(merge_create_kernel, dim3((n_unique + 255) / 256), dim3(256), 0, dst->stream, (const MapView *)dst->view_dev.get(), G, n_unique);
    }
    const MeshParams P = mesh_params(dst);
    FOR_CHUNK_SIZE(dst->N, launch_merge_gather<N>(dst, src, P, G, T, n_unique));
    HIP_TRY(hipGetLastError());
    rc = rewrite_end(dst);
    if (rc) return rc;
    rc = release_source();
    if (rc) return rc;
    if (!stats) return CHISEL_HIP_OK;
    hipLaunchKernelGGL(report_words_kernel<unsigned long long>, dim3(1), dim3(1), 0, dst->stream, (const unsigned long long *)G.stats,
                       reinterpret_cast<unsigned long long *>(O.host.dev() + 8), MS_WORDS);
    HIP_TRY(hipGetLastError());
    rc = check_device_error(dst);  // waits
    if (rc) return rc;
    const volatile unsigned long long *res = reinterpret_cast<const volatile unsigned long long *>(O.host.get() + 8);
    stats->dst_chunks_created = (int64_t)res[MS_CREATED];
    stats->dst_chunks_updated = (int64_t)res[MS_UPDATED];
    stats->voxels_updated = (int64_t)res[MS_VOXELS];
    return CHISEL_HIP_OK;
}

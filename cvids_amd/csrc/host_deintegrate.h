// host_deintegrate.h -- chisel_hip_deintegrate_depth and chisel_hip_deintegrate_batch (included by chisel_hip.hip; the kernels and the definition: kernels_deintegrate.h,
// DESIGN.md 3.10).  Everything runs on the map's stream: the list kernel, then the apply kernel, whose fixed grid reads the list's length
// from the device -- no host wait between them, and none at all when the caller asks for neither stats nor ids.  The scratch lives in the
// map (chisel_hip_map::deintegrate_mem), is reused by the next call and freed with the map; a host image goes through the map's
// staging buffer (stage_depth; the batch entry stages a launch set's host images side by side and keeps its per-frame constants in a
// table on the device).  Both entries read top to bottom: refusals, scratch, staging or table, launches, tail.  The frame they share
// with the other entries that rewrite a map: host_rewrite.h; what they refuse about their arguments, and the planes of the list
// kernel: host_checks.h.
#pragma once

namespace {
namespace deintegrate {

// what both entries refuse about the map, in one order: group, null, shard (nothing is touched by a refused call).  null_argument: the
// entry has another argument that is null; null_what: what it says of a null argument
int map_refusal(const chisel_hip_map *m, const char *name, bool null_argument, const char *null_what) {
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " rewrites the voxels of all owners: a group's shards hold a part each, and ghost chunks would need a rule of their own");
    if (!m || null_argument) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + null_what);
    if (m->cfg.n_shards > 1) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " rewrites the voxels of all owners: this map is one shard of several");
    return CHISEL_HIP_OK;
}

// Room for one list entry per committed slot, the stats and a list length per launch set, `max_ids` ids -> the batch kernels' view of
// them (single_view: the single frame's, which reads the list as int and keeps its length in stats[DS_LISTED]).
// One set serves both entries: every call queues on the map's stream, so a call's kernels run behind those of the call before, and a
// call that reads the pinned block waits for the stream before it returns, so no later call's report can land in it first.  (A buffer
// grows behind a wait for the stream: a launch chain before this one may still read it.)
int ensure_scratch(chisel_hip_map *m, int n_sets, int max_ids, DeintegrateBatchView &G) {
    chisel_hip_map::DeintegrateMemory &O = m->deintegrate_mem;
    if (!O.host) HIP_TRY(O.host.alloc(DS_WORDS));
    int rc = grow_buffer(O.list, (size_t)std::max(m->view.committed, 1), m->stream);
    if (!rc) rc = grow_buffer(O.words, (size_t)DS_WORDS + (size_t)n_sets, m->stream);
    if (!rc) rc = grow_buffer(O.ids, (size_t)3 * max_ids, m->stream);
    G = DeintegrateBatchView{O.list.get(), O.words.get(), nullptr, max_ids ? O.ids.get() : nullptr, max_ids, nullptr, 0};
    return rc;
}
inline DeintegrateView single_view(const DeintegrateBatchView &G) { return DeintegrateView{reinterpret_cast<int *>(G.list), G.stats, G.emptied, G.max_ids}; }

// the call's constants: the integrator's settings and the map's (the camera and the image are the frame's)
void fill_constants(const chisel_hip_map *m, int color_rules, DeintegrateFrame &F) {
    F.trunc_kind = m->integ.truncator_kind;
    F.trunc_param = m->integ.truncator_param;
    F.weight = m->integ.weight;
    F.res = m->cfg.voxel_resolution;
    F.half_res = m->cfg.voxel_resolution * 0.5f;                                          // ChunkManager.cpp:52
    F.diag = (float)(2.0 * ::sqrt((double)3.0f) * (double)m->cfg.voxel_resolution);       // ProjectionIntegrator.h:58,109
    F.color_rules = color_rules ? 1 : 0;
    F.max_depth = color_rules ? 100.0f : 50.0f;
}

inline unsigned list_grid(const chisel_hip_map *m) { return (unsigned)std::max(1, (m->view.committed + 255) / 256); }
inline unsigned apply_grid(const chisel_hip_map *m) { return (unsigned)std::max(1, std::min(m->view.committed, DEINTEGRATE_GRID)); }

// Behind the last launch: the map's bookkeeping; without `stats` a wait only where a caller's host image is still being copied
// (`host_images`); with them the report, the one wait, the six counts and the ids.
int finish(chisel_hip_map *m, const DeintegrateBatchView &G, bool host_images, chisel_hip_deintegrate_stats *stats, int *emptied_ids_xyz) {
    static_assert(sizeof(chisel_hip_deintegrate_stats) == 48, "chisel_hip_deintegrate_stats is six 64-bit counts");
    static_assert(sizeof(chisel_hip_deintegrate_stats) <= DS_WORDS * sizeof(unsigned long long), "the stats travel in the report words");
    HIP_TRY(hipGetLastError());
    int rc = rewrite_end(m);
    if (rc) return rc;
    if (!stats) {
        if (host_images) HIP_TRY(hipStreamSynchronize(m->stream));  // (the copies of the caller's images are over on return)
        return CHISEL_HIP_OK;
    }
    PinnedBuffer<unsigned long long> &host = m->deintegrate_mem.host;
    hipLaunchKernelGGL(report_words_kernel<unsigned long long>, dim3(1), dim3(1), 0, m->stream, (const unsigned long long *)G.stats, host.dev(), DS_WORDS);
    HIP_TRY(hipGetLastError());
    rc = check_device_error(m);  // the one wait
    if (rc) return rc;
    const volatile unsigned long long *res = host.get();
    stats->chunks_tested = (int64_t)res[DS_TESTED];
    stats->chunks_touched = (int64_t)res[DS_TOUCHED];
    stats->chunks_emptied = (int64_t)res[DS_EMPTIED];
    stats->voxels_updated = (int64_t)res[DS_UPDATED];
    stats->voxels_cleared = (int64_t)res[DS_CLEARED];
    stats->voxels_skipped = (int64_t)res[DS_SKIPPED];
    const int64_t n_ids = std::min<int64_t>(stats->chunks_emptied, G.max_ids);
    if (n_ids > 0) HIP_TRY(hipMemcpy(emptied_ids_xyz, G.emptied, (size_t)n_ids * 3 * sizeof(int), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}

inline size_t stage_floats_of(const chisel_hip_depth_frame &f) { return f.on_device ? 0 : (((size_t)f.width * f.height + 3) & ~(size_t)3); }  // (16-byte sections)

}  // namespace deintegrate
}  // namespace

extern "C" int chisel_hip_deintegrate_depth(chisel_hip_map *m, const chisel_hip_depth_frame *frame, int color_rules, chisel_hip_deintegrate_stats *stats,
                                            int *emptied_ids_xyz, int max_ids) {
    const char *name = "chisel_hip_deintegrate_depth";
    // ---- refusals: nothing is touched by a refused call
    int rc = deintegrate::map_refusal(m, name, !frame || !frame->depth, "null map, frame or depth image");
    if (rc) return rc;
    if (const char *why = deintegrate_refusal(frame->depth, frame->width, frame->height, frame->pose, frame->fx, frame->fy, frame->cx, frame->cy,
                                              stats != nullptr, emptied_ids_xyz != nullptr, max_ids))
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    rc = rewrite_begin(m);
    if (rc) return rc;
    DeintegrateBatchView B;
    rc = deintegrate::ensure_scratch(m, 0, emptied_ids_xyz ? max_ids : 0, B);
    if (rc) return rc;
    DeintegrateFrame F;
    rc = stage_depth(m, frame, &F.depth);
    if (rc) return rc;
    rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: a device image is ready behind it
    if (rc) return rc;

    // ---- the two launches
    const DeintegrateView G = deintegrate::single_view(B);
    fill_camera(F.cam, frame->pose, frame->fx, frame->fy, frame->cx, frame->cy, frame->width, frame->height);
    deintegrate::fill_constants(m, color_rules, F);
    DeintegratePyramid Y;
    deintegrate_pyramid(frame->pose, frame->fx, frame->fy, frame->cx, frame->cy, frame->width, frame->height, m->N, m->cfg.voxel_resolution, Y);
    HIP_TRY(hipMemsetAsync(G.stats, 0, DS_WORDS * sizeof(unsigned long long), m->stream));
    hipLaunchKernelGGL(deintegrate_list_kernel, dim3(deintegrate::list_grid(m)), dim3(256), 0, m->stream, m->view, G, Y);
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL((deintegrate_apply_kernel<N, 256, DeintegrateView>), dim3(deintegrate::apply_grid(m)), dim3(256), 0, m->stream, m->view, G, F));
    return deintegrate::finish(m, B, !frame->on_device, stats, emptied_ids_xyz);
}

// Many frames in one call: launch sets of at most KMAX frames, in order, two launches each, all on the map's stream with no host wait
// between them.  One table of per-frame constants per call (a later call's upload is queued behind this call's kernels), one memset of
// the stats and the sets' list lengths per call.
extern "C" int chisel_hip_deintegrate_batch(chisel_hip_map *m, int n, const chisel_hip_depth_frame *frames, int color_rules, chisel_hip_deintegrate_stats *stats,
                                            int *emptied_ids_xyz, int max_ids) {
    const char *name = "chisel_hip_deintegrate_batch";
    // ---- refusals: every frame is looked at before anything is touched
    int rc = deintegrate::map_refusal(m, name, false, "null map");
    if (rc) return rc;
    int bad_frame = -1;
    if (const char *why = deintegrate_batch_refusal(n, frames, stats != nullptr, emptied_ids_xyz != nullptr, max_ids, &bad_frame))
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + (bad_frame >= 0 ? "frame " + std::to_string(bad_frame) + ": " : std::string()) + why);
    if (stats) *stats = chisel_hip_deintegrate_stats{0, 0, 0, 0, 0, 0};
    if (n == 0) return CHISEL_HIP_OK;
    rc = rewrite_begin(m);
    if (rc) return rc;
    const int n_sets = (n + KMAX - 1) / KMAX;
    size_t stage_floats = 0;  // the largest set's host images
    bool any_host = false;
    for (int s = 0; s < n_sets; s++) {
        size_t sum = 0;
        for (int i = s * KMAX; i < std::min(n, (s + 1) * KMAX); i++) sum += deintegrate::stage_floats_of(frames[i]);
        stage_floats = std::max(stage_floats, sum);
        any_host = any_host || sum != 0;
    }
    chisel_hip_map::DeintegrateMemory &O = m->deintegrate_mem;
    DeintegrateBatchView G;
    rc = deintegrate::ensure_scratch(m, n_sets, emptied_ids_xyz ? max_ids : 0, G);
    if (!rc) rc = grow_buffer(O.table, (size_t)n, m->stream);
    if (!rc && stage_floats) rc = grow_buffer(m->frame_stage, stage_floats, m->stream);
    if (rc) return rc;
    chisel_hip_map::DeintegrateMemory::TableUpload *up = nullptr;
    rc = take_upload(O.uploads, (size_t)n, &up);  // (chisel_hip.hip)
    if (rc) return rc;

    // ---- the table: a host image of set s has the s-th use of its place in the staging buffer
    DeintegrateBatchEntry *T = up->host.get();
    for (int s = 0; s < n_sets; s++) {
        size_t at = 0;
        for (int i = s * KMAX; i < std::min(n, (s + 1) * KMAX); i++) {
            const chisel_hip_depth_frame &f = frames[i];
            deintegrate_pyramid(f.pose, f.fx, f.fy, f.cx, f.cy, f.width, f.height, m->N, m->cfg.voxel_resolution, T[i].Y);
            fill_camera(T[i].cam, f.pose, f.fx, f.fy, f.cx, f.cy, f.width, f.height);
            T[i].depth = f.on_device ? f.depth : m->frame_stage.get() + at;
            at += deintegrate::stage_floats_of(f);
        }
    }
    rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: a device image is ready behind it
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(O.table.get(), T, (size_t)n * sizeof(DeintegrateBatchEntry), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipEventRecord(up->copied, m->stream));

    // ---- per set: its host images, then the two launches
    G.table = O.table.get();
    DeintegrateFrame F{};  // the call's constants; the camera and the image come from the table
    deintegrate::fill_constants(m, color_rules, F);
    HIP_TRY(hipMemsetAsync(G.stats, 0, ((size_t)DS_WORDS + (size_t)n_sets) * sizeof(unsigned long long), m->stream));
    for (int s = 0; s < n_sets; s++) {
        const int first = s * KMAX, count = std::min(n - first, KMAX);
        for (int i = first; i < first + count; i++)
            if (!frames[i].on_device)
                HIP_TRY(hipMemcpyAsync(const_cast<float *>(T[i].depth), frames[i].depth, (size_t)frames[i].width * frames[i].height * sizeof(float), hipMemcpyHostToDevice, m->stream));
        G.listed = G.stats + DS_WORDS + s;
        G.first = first;
        hipLaunchKernelGGL(deintegrate_list_batch_kernel, dim3(deintegrate::list_grid(m)), dim3(256), 0, m->stream, m->view, G, first, count);
        FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL((deintegrate_apply_kernel<N, deintegrate_batch_threads(N), DeintegrateBatchView>), dim3(deintegrate::apply_grid(m)), dim3(deintegrate_batch_threads(N)), 0, m->stream, m->view, G, F));
    }
    return deintegrate::finish(m, G, any_host, stats, emptied_ids_xyz);
}

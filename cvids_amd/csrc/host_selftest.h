// host_selftest.h -- the chisel_hip_kat_* and chisel_hip_debug_* entry points of include/chisel_hip_selftest.h (included by
// chisel_hip.hip): tests only, not part of the reference surface.
extern "C" {

// ---- known-answer entry points (tests only; not part of the reference surface) -------------------------
int chisel_hip_kat_truncation(int kind, float param, const float *depths, int n, float *trunc, float *weight1) {
    DeviceBuffer<float> d_in, d_t, d_w;
    HIP_TRY(d_in.alloc(n));
    HIP_TRY(d_t.alloc(n));
    HIP_TRY(d_w.alloc(n));
    HIP_TRY(hipMemcpy(d_in.get(), depths, n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kat_truncation_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, kind, param, d_in.get(), n, d_t.get(), d_w.get());
    HIP_TRY(hipMemcpy(trunc, d_t.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(weight1, d_w.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_dist(const float *ops, int n, float *out) {
    DeviceBuffer<float> d_in, d_out;
    HIP_TRY(d_in.alloc(n * 3));
    HIP_TRY(d_out.alloc(n * 2));
    HIP_TRY(hipMemcpy(d_in.get(), ops, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kat_dist_kernel, dim3(1), dim3(64), 0, 0, d_in.get(), n, d_out.get());
    HIP_TRY(hipMemcpy(out, d_out.get(), n * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_raycast(const float *rays, int n, const int lo[3], const int hi[3], int *cells, int cap, int *count) {
    DeviceBuffer<float> d_in;
    DeviceBuffer<int> d_cells, d_count;
    HIP_TRY(d_in.alloc((size_t)n * 6));
    HIP_TRY(d_cells.alloc((size_t)n * cap * 3));
    HIP_TRY(d_count.alloc((size_t)n));
    HIP_TRY(hipMemcpy(d_in.get(), rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kat_raycast_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d_in.get(), n, make_int3(lo[0], lo[1], lo[2]),
                       make_int3(hi[0], hi[1], hi[2]), d_cells.get(), cap, d_count.get());
    HIP_TRY(hipMemcpy(cells, d_cells.get(), (size_t)n * cap * 3 * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, d_count.get(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_color(const uint8_t *ops, int n, uint8_t *out) {
    DeviceBuffer<uint8_t> d_in, d_out;
    HIP_TRY(d_in.alloc(n * 4));
    HIP_TRY(d_out.alloc(n * 4));
    HIP_TRY(hipMemcpy(d_in.get(), ops, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kat_color_kernel, dim3(1), dim3(64), 0, 0, d_in.get(), n, d_out.get());
    HIP_TRY(hipMemcpy(out, d_out.get(), n * 4, hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_color_fresh(unsigned *mismatches) {
    DeviceBuffer<unsigned> d;
    HIP_TRY(d.alloc(1));
    HIP_TRY(hipMemset(d.get(), 0, sizeof(unsigned)));
    hipLaunchKernelGGL(kat_color_fresh_kernel, dim3(8 * 256 * 256 / 256), dim3(256), 0, 0, d.get());
    HIP_TRY(hipMemcpy(mismatches, d.get(), sizeof(unsigned), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
// diagnostics of the last cloud: listed chunks, (unit, point) pairs, rays of the largest unit, units with rays
int chisel_hip_debug_cloud_stats(chisel_hip_map *m, int64_t out[4]) {
    SETTLE(m);
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "per-shard read-out");
    if (!m || !m->cloud.view.ctl) return fail(CHISEL_HIP_ERR_INVALID, "no cloud yet");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    int ctl[2] = {0, 0};
    HIP_TRY(hipMemcpy(ctl, m->cloud.view.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    const int units = std::min(ctl[0], CLOUD_MAX_LISTED) * CloudUnits(m->N, 0, cloud_unit_depth(m->N)).count;
    std::vector<int> off((size_t)units + 1);
    HIP_TRY(hipMemcpy(off.data(), m->cloud.view.offsets, off.size() * sizeof(int), hipMemcpyDeviceToHost));
    int64_t mx = 0, used = 0;
    for (int i = 0; i < units; i++) {
        mx = std::max<int64_t>(mx, off[i + 1] - off[i]);
        used += off[i + 1] > off[i];
    }
    out[0] = ctl[0]; out[1] = ctl[1]; out[2] = mx; out[3] = used;
    return CHISEL_HIP_OK;
}
// the chunk hash and the slot tables as they stand once the map's stream has drained (copies only): info = {hash capacity, committed
// slots, free_top, 0}; arrays that are null are skipped -- a first call with none of them tells the sizes
int chisel_hip_debug_hash_table(chisel_hip_map *m, int64_t info[4], uint64_t *hash_keys, int *hash_vals, uint64_t *slot_key, int *free_list) {
    SETTLE(m);
    if (!m || !info || m->is_group) return fail(CHISEL_HIP_ERR_INVALID, "the read-out of one map's table (not of a group)");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const size_t cap = (size_t)m->view.hash_mask + 1, committed = (size_t)m->view.committed;
    int top = 0;
    HIP_TRY(hipMemcpy(&top, m->view.free_top, sizeof(int), hipMemcpyDeviceToHost));
    info[0] = (int64_t)cap; info[1] = (int64_t)committed; info[2] = top; info[3] = 0;
    if (hash_keys) HIP_TRY(hipMemcpy(hash_keys, m->view.hash_keys, cap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (hash_vals) HIP_TRY(hipMemcpy(hash_vals, m->view.hash_vals, cap * sizeof(int), hipMemcpyDeviceToHost));
    if (slot_key && committed) HIP_TRY(hipMemcpy(slot_key, m->view.slot_key, committed * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (free_list && committed) HIP_TRY(hipMemcpy(free_list, m->view.free_list, committed * sizeof(int), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_color_any(unsigned *mismatches) {
    DeviceBuffer<unsigned> d;
    HIP_TRY(d.alloc(1));
    HIP_TRY(hipMemset(d.get(), 0, sizeof(unsigned)));
    hipLaunchKernelGGL(kat_color_any_kernel, dim3(256 * 256 * 256 / 256), dim3(256), 0, 0, d.get());
    HIP_TRY(hipMemcpy(mismatches, d.get(), sizeof(unsigned), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_reciprocal(unsigned long long *mismatches, unsigned *example_bits) {
    DeviceBuffer<unsigned long long> d;
    DeviceBuffer<unsigned> e;
    HIP_TRY(d.alloc(1));
    HIP_TRY(e.alloc(1));
    HIP_TRY(hipMemset(d.get(), 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(e.get(), 0, sizeof(unsigned)));
    unsigned lo, hi;
    const float fmin = FASTZ_MIN, fmax = FASTZ_MAX;
    memcpy(&lo, &fmin, 4);
    memcpy(&hi, &fmax, 4);
    hipLaunchKernelGGL(kat_reciprocal_kernel, dim3(4096), dim3(256), 0, 0, lo, (unsigned long long)(hi - lo) + 1ull, d.get(), e.get());
    HIP_TRY(hipMemcpy(mismatches, d.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(example_bits, e.get(), sizeof(unsigned), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
int chisel_hip_kat_floor(unsigned long long *mismatches, unsigned *example_bits) {
    DeviceBuffer<unsigned long long> d;
    DeviceBuffer<unsigned> e;
    HIP_TRY(d.alloc(1));
    HIP_TRY(e.alloc(1));
    HIP_TRY(hipMemset(d.get(), 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(e.get(), 0, sizeof(unsigned)));
    hipLaunchKernelGGL(kat_floor_kernel, dim3(4096), dim3(256), 0, 0, d.get(), e.get());
    HIP_TRY(hipMemcpy(mismatches, d.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(example_bits, e.get(), sizeof(unsigned), hipMemcpyDeviceToHost));
    return CHISEL_HIP_OK;
}
// the candidate ids cull_kernel hands to shard `rank` of `n_shards` for an id range (host evaluation of CullSpace; no GPU needed):
// returns the number of slots, writes the ids of the slots that hold one (at most `capacity`), *count = how many do
int chisel_hip_debug_cull_space(const int range_min[3], const int range_dim[3], int n_shards, int shard_rank, int shard_block, int *ids,
                                int capacity, int *count) {
    CullParams P;
    memset(&P, 0, sizeof(P));
    for (int a = 0; a < 3; a++) {
        P.range_min[a] = range_min[a];
        P.range_dim[a] = range_dim[a];
    }
    P.ip.n_shards = n_shards;
    P.ip.shard_rank = shard_rank;
    P.ip.shard_block = shard_block;
    const CullSpace space(P);
    int n = 0;
    for (int c = 0; c < space.total; c++) {
        int x, y, z;
        if (!space.id(P, c, x, y, z)) continue;
        if (n < capacity) {
            ids[3 * n] = x; ids[3 * n + 1] = y; ids[3 * n + 2] = z;
        }
        n++;
    }
    *count = n;
    return space.total;
}
int chisel_hip_debug_frustum_range(const float *pose, float near_plane, float far_plane, float fy, float cy, int W, int H,
                                   int chunk_n, float res, int *range_min3, int *range_dim3, float *planes24, float *corners24) {
    hostmath::FrustumRange fr = hostmath::frustum_range(pose, near_plane, far_plane, fy, cy, W, H, chunk_n, res);
    memcpy(range_min3, fr.range_min, sizeof(fr.range_min));
    memcpy(range_dim3, fr.range_dim, sizeof(fr.range_dim));
    if (planes24) memcpy(planes24, fr.planes, sizeof(fr.planes));
    if (corners24) memcpy(corners24, fr.corners, sizeof(fr.corners));
    return CHISEL_HIP_OK;
}

}  // extern "C"

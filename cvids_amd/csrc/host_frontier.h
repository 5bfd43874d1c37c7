// host_frontier.h -- chisel_hip_frontiers (included by chisel_hip.hip; the kernels: kernels_frontier.h; the refusals, the widened
// window, the tile grid and the scratch sizes: frontier_checks.h; the definition: DESIGN.md 3.18).  chisel_hip_distance_field's frame
// (host_distance.h) in front of the wait -- the map is only read, everything goes on the map's stream behind whatever was queued
// before --, chisel_hip_filter_mesh's behind it (host_components.h): THE WAIT for the totals (pinned memory), the capacities, then what
// writes the caller's arrays.  With device pointers nothing is waited for behind those launches; host arrays are staged through one
// owned buffer sized by the totals, copied out once with exactly their live rows, and are complete on return.  The cluster table is
// host memory whatever on_device says: its rows are written into pinned memory behind the wait, which costs a wait of its own.
//
// Scratch the map owns (chisel_hip_map::frontier_mem), grown on demand, freed with the map.
#pragma once

namespace {
namespace frontier {

struct Totals {
    int64_t unknown, free, occupied, frontier, clusters, largest_voxels, kept_clusters, kept_voxels;
};

inline unsigned blocks(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

// the planes, the per-voxel ints and the control words of a call, and the view on them
int ensure_memory(chisel_hip_map *m, const FrontierPlan &plan, FrontierView &X) {
    chisel_hip_map::FrontierMemory &F = m->frontier_mem;
    if (int rc = grow_buffer(F.planes, (size_t)plan.plane_words, m->stream)) return rc;  // (waits for the stream before it replaces a buffer)
    if (int rc = grow_buffer(F.ints, (size_t)plan.ints, m->stream)) return rc;
    if (!F.ctl) HIP_TRY(F.ctl.alloc(FRONTIER_HOST_WORDS));
    HIP_TRY(F.host.ensure(FRONTIER_HOST_WORDS, m->stream));
    unsigned long long *p = F.planes.get();
    const size_t wide = (size_t)plan.wide_words, words = (size_t)plan.words;
    X.wide_free = p;
    X.wide_unknown = p + wide;
    p += 2 * wide;
    X.front = p;
    X.roots = p + words;
    X.kept = p + 2 * words;
    X.kept_roots = p + 3 * words;
    X.prefix = p + 4 * words;
    X.sums = p + 5 * words;
    int *q = F.ints.get();
    X.parent = q;
    X.root_of = q + (size_t)plan.voxels;
    X.count = q + 2 * (size_t)plan.voxels;
    X.ctl = F.ctl.get();
    return CHISEL_HIP_OK;
}

}  // namespace frontier
}  // namespace

extern "C" {

int chisel_hip_frontiers(chisel_hip_map *m, const chisel_hip_frontier_window *window, uint8_t *state, int32_t *label, int64_t capacity_voxels, int32_t *voxels,
                         int64_t capacity_clusters, int64_t *cluster_table, int on_device, chisel_hip_frontier_totals *totals) {
    static_assert(sizeof(chisel_hip_frontier_totals) == 64, "chisel_hip_frontier_totals is 64 bytes");
    static_assert(sizeof(chisel_hip_frontier_window) == 40, "chisel_hip_frontier_window is 40 bytes");
    const char *name = "chisel_hip_frontiers";
    SETTLE(m);
    {
        int rc_r = query_refusal(m, name, "reads the voxels of the window and of a margin around it");
        if (rc_r) return rc_r;
    }
    FrontierPlan plan;
    {
        int code = 0;
        if (const char *why = frontier_refusal(window, totals, capacity_voxels, voxels, capacity_clusters, cluster_table, &code, &plan))
            return fail(code == FRONTIER_REFUSED_UNSUPPORTED ? CHISEL_HIP_ERR_UNSUPPORTED : CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    }
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
        if (rc_m) return rc_m;
    }
    // ---- the scratch, everything in front of the wait, the wait
    FrontierView X{};
    for (int a = 0; a < 3; a++) {
        X.wo[a] = plan.wo[a];
        X.wd[a] = plan.wd[a];
        X.dims[a] = window->dims[a];
        X.tiles[a] = (int)plan.tiles[a];
    }
    X.min_unknown_faces = window->min_unknown_faces;
    X.level = frontier_level(window->connectivity);
    X.min_voxels = window->min_voxels;
    X.surface_offset = window->surface_offset;
    X.wide_words_per_row = (int)plan.wide_words_per_row;
    X.words_per_row = (int)plan.words_per_row;
    X.words = plan.words;
    {
        int rc_s = frontier::ensure_memory(m, plan, X);
        if (rc_s) return rc_s;
    }
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
        if (rc_w) return rc_w;
    }
    chisel_hip_map::FrontierMemory &F = m->frontier_mem;
    const dim3 block(FRONTIER_THREADS);
    const dim3 per_word(frontier::blocks(plan.words, FRONTIER_THREADS)), per_voxel(frontier::blocks(plan.words, 4)), per_tile((unsigned)plan.n_tiles);
    HIP_TRY(hipMemsetAsync(X.ctl, 0, FRONTIER_HOST_WORDS * sizeof(unsigned long long), m->stream));
    const long long n_runs = plan.wide_words;  // (a run holds a voxel of the widened window)
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(frontier_seed_kernel<N>, dim3(frontier::blocks(n_runs, 4)), dim3(256), 0, m->stream, m->view, X, n_runs));
    hipLaunchKernelGGL(frontier_mark_kernel, per_word, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_tile_kernel, per_tile, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_merge_kernel, per_tile, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_label_kernel, per_voxel, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_keep_kernel, per_voxel, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_sums_kernel, per_word, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_scan_sums_kernel, dim3(1), block, 0, m->stream, X.sums, (long long)plan.scan_tiles, X.ctl);
    hipLaunchKernelGGL(frontier_prefix_kernel, per_word, block, 0, m->stream, X);
    hipLaunchKernelGGL(frontier_report_kernel, dim3(1), dim3(64), 0, m->stream, (const unsigned long long *)X.ctl, F.host.dev());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));  // THE WAIT
    note_stream_idle(m);
    std::atomic_thread_fence(std::memory_order_acquire);
    frontier::Totals T;
    {
        volatile long long *w = F.host.get();
        T.unknown = w[FC_UNKNOWN];
        T.free = w[FC_FREE];
        T.occupied = plan.voxels - T.unknown - T.free;
        T.frontier = w[FC_FRONTIER];
        T.clusters = w[FC_CLUSTERS];
        T.largest_voxels = w[FC_LARGEST];
        T.kept_clusters = w[FC_KEPT_CLUSTERS];
        T.kept_voxels = w[FC_KEPT_VOXELS];
    }
    if (frontier_is_query(state, label, capacity_voxels, voxels, capacity_clusters, cluster_table)) {
        copy_totals(T, totals);
        return CHISEL_HIP_OK;
    }
    if (const char *why = frontier_capacity_refusal(T.kept_voxels, T.kept_clusters, capacity_voxels, voxels, capacity_clusters, cluster_table)) {
        copy_totals(T, totals);  // (the caller can retry)
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    }
    // ---- the per-voxel arrays, the list and the table
    const bool table = cluster_table && capacity_clusters > 0 && T.kept_clusters > 0;
    const size_t table_words = (size_t)T.kept_clusters * FRONTIER_TABLE_WORDS;
    if (table) {
        int rc_t = grow_buffer(F.acc, table_words, m->stream);
        if (rc_t) return rc_t;
        HIP_TRY(F.table_host.ensure(table_words, m->stream));
    }
    uint8_t *ds = state;
    int32_t *dl = label, *dv = voxels && capacity_voxels > 0 && T.kept_voxels > 0 ? voxels : nullptr;
    Staging out(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
    out.out(ds, (size_t)plan.voxels);
    out.out(dl, (size_t)plan.voxels * sizeof(int32_t));
    out.out(dv, (size_t)T.kept_voxels * 4 * sizeof(int32_t));
    HIP_TRY(out.begin());
    if (ds || dl || dv) hipLaunchKernelGGL(frontier_write_kernel, per_voxel, block, 0, m->stream, X, ds, dl, dv);
    if (table) {
        hipLaunchKernelGGL(frontier_table_init_kernel, dim3(frontier::blocks((int64_t)table_words, FRONTIER_THREADS)), block, 0, m->stream, F.acc.get(), (long long)T.kept_clusters);
        hipLaunchKernelGGL(frontier_table_kernel, dim3(frontier::blocks(plan.words, 4 * FRONTIER_TABLE_SPAN)), block, 0, m->stream, X, F.acc.get());
        hipLaunchKernelGGL(frontier_table_rows_kernel, dim3(frontier::blocks((int64_t)table_words, FRONTIER_THREADS)), block, 0, m->stream, (const long long *)F.acc.get(),
                           F.table_host.dev(), (long long)table_words);
    }
    hipError_t e = out.finish(hipGetLastError());
    if (e == hipSuccess && table) {  // (host arrays have waited in finish; device arrays are left on the stream, the table is not)
        if (on_device) e = hipStreamSynchronize(m->stream);
        std::atomic_thread_fence(std::memory_order_acquire);
        volatile long long *rows = F.table_host.get();
        for (size_t i = 0; e == hipSuccess && i < table_words; i++) cluster_table[i] = rows[i];
    }
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // extern "C"

// host_frontier.h -- chisel_hip_frontiers (included by chisel_hip.hip; the kernels: kernels_frontier.h; the refusals, the widened
// window, the tile grid and the scratch sizes: frontier_checks.h; the definition: DESIGN.md 3.18).  chisel_hip_distance_field's frame
// (host_distance.h) in front of the wait -- the map is only read, and a group is answered by query_refusal --, the frame of
// host_totals.h from the control words on.  The cluster table is host memory whatever on_device says.  Scratch:
// chisel_hip_map::frontier_mem.
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
    if (int rc = F.ctl.prepare(m, FRONTIER_HOST_WORDS)) return rc;
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
    X.ctl = F.ctl.dev();
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
    if (int rc = query_refusal(m, name, "reads the voxels of the window and of a margin around it")) return rc;
    FrontierPlan plan;
    {
        int code = 0;
        if (const char *why = frontier_refusal(window, totals, capacity_voxels, voxels, capacity_clusters, cluster_table, &code, &plan))
            return refusal(name, why, code == FRONTIER_REFUSED_UNSUPPORTED);
    }
    HIP_TRY(hipSetDevice(m->device));
    if (int rc = check_mesh_totals(m)) return rc;  // a recompute in flight reads the voxels as they are
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
    if (int rc = frontier::ensure_memory(m, plan, X)) return rc;
    if (int rc = wait_for_input(m, m->stream)) return rc;  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
    chisel_hip_map::FrontierMemory &F = m->frontier_mem;
    const dim3 block(FRONTIER_THREADS);
    const dim3 per_word(frontier::blocks(plan.words, FRONTIER_THREADS)), per_voxel(frontier::blocks(plan.words, 4)), per_tile((unsigned)plan.n_tiles);
    HIP_TRY(F.ctl.zero(m->stream));
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
    frontier::Totals T;
    {
        volatile long long *w;
        if (int rc = F.ctl.report_and_wait(m, &w)) return rc;
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
        return refusal(name, why, false);
    }
    // ---- the per-voxel arrays, the list and the table
    const bool table = cluster_table && capacity_clusters > 0 && T.kept_clusters > 0;
    const size_t table_words = (size_t)T.kept_clusters * FRONTIER_TABLE_WORDS;
    if (table) {
        if (int rc = grow_buffer(F.acc, table_words, m->stream)) return rc;
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
    if (table) e = read_pinned_table(m, F.table_host, table_words, on_device != 0, e, cluster_table);
    if (e != hipSuccess) return hip_failure(name, e);
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // extern "C"

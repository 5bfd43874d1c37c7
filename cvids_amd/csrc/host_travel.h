// host_travel.h -- chisel_hip_travel_field and chisel_hip_travel_path (included by chisel_hip.hip; the kernels: kernels_travel.h; the
// refusals, the seed check, the tile grid, the scratch sizes and the walk: travel_checks.h; the definition: DESIGN.md 3.19).
// chisel_hip_frontiers' frame (host_frontier.h) in front of the rounds -- the map is only read, and a group is answered by
// query_refusal --, then the host loop: TRAVEL_ROUNDS_PER_WAIT round launches, the tiles flagged behind the last of them through the
// control words of host_totals.h, another batch while that number is not zero.  The group table is host memory whatever on_device
// says.  Scratch: chisel_hip_map::travel_mem; with a clearance the distance field's own (distance_mem) beside it.
#pragma once

namespace {
namespace travel {

struct Totals {
    int64_t unknown, free, occupied, traversable, seeds_used, seeds_ignored, reached, largest_cost, targets_reached, targets_ignored, rounds, tile_visits;
};

inline unsigned blocks(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

int ensure_memory(chisel_hip_map *m, const TravelPlan &plan, int64_t n_seeds, FrontierView &X, TravelView &T, int **dist2, bool clearance) {
    chisel_hip_map::TravelMemory &F = m->travel_mem;
    if (int rc = grow_buffer(F.planes, (size_t)plan.plane_words, m->stream)) return rc;  // (waits for the stream before it replaces a buffer)
    if (int rc = grow_buffer(F.ints, (size_t)plan.ints, m->stream)) return rc;
    if (int rc = grow_buffer(F.seeds, (size_t)n_seeds * 3, m->stream)) return rc;
    if (int rc = F.ctl.prepare(m, TRAVEL_HOST_WORDS)) return rc;
    unsigned long long *p = F.planes.get();
    X.wide_free = p;
    X.wide_unknown = p + (size_t)plan.wide_words;
    T.trav = p + 2 * (size_t)plan.wide_words;
    int *q = F.ints.get();
    T.cost = q;
    q += (size_t)plan.voxels;
    *dist2 = clearance ? q : nullptr;
    if (clearance) q += (size_t)plan.voxels;
    T.flags = q;
    T.ctl = F.ctl.dev();
    return CHISEL_HIP_OK;
}

}  // namespace travel
}  // namespace

extern "C" {

int chisel_hip_travel_field(chisel_hip_map *m, const chisel_hip_travel_window *window, const int32_t *seeds, int64_t n_seeds, const int32_t *targets,
                            int64_t n_targets, int64_t n_groups, int32_t *cost, uint8_t *step, uint8_t *state, int64_t *group_table, int on_device,
                            chisel_hip_travel_totals *totals) {
    static_assert(sizeof(chisel_hip_travel_totals) == 96, "chisel_hip_travel_totals is 96 bytes");
    static_assert(sizeof(chisel_hip_travel_window) == 56, "chisel_hip_travel_window is 56 bytes");
    const char *name = "chisel_hip_travel_field";
    SETTLE(m);
    if (int rc = query_refusal(m, name, "reads the voxels of the window and of a margin around it")) return rc;
    TravelPlan plan;
    DistancePlan dplan;
    chisel_hip_distance_window dw{};
    {
        int code = 0;
        if (const char *why = travel_refusal(window, seeds, n_seeds, targets, n_targets, n_groups, group_table, totals, &code, &plan))
            return refusal(name, why, code == TRAVEL_REFUSED_UNSUPPORTED);
        if (window->clearance > 0) {
            for (int a = 0; a < 3; a++) {
                dw.origin[a] = window->origin[a];
                dw.dims[a] = window->dims[a];
            }
            dw.radius = window->clearance;
            dw.unknown_is_obstacle = window->unknown_is_obstacle;
            dw.surface_offset = window->surface_offset;
            if (const char *why = distance_refusal(&dw, true, &code, &dplan)) return refusal(name, why, code == DISTANCE_REFUSED_UNSUPPORTED);
        }
    }
    HIP_TRY(hipSetDevice(m->device));
    if (int rc = check_mesh_totals(m)) return rc;  // a recompute in flight reads the voxels as they are
    // ---- the scratch and the views
    FrontierView X{};
    TravelView T{};
    for (int a = 0; a < 3; a++) {
        X.wo[a] = plan.wo[a];
        X.wd[a] = plan.wd[a];
        X.dims[a] = T.dims[a] = window->dims[a];
        X.tiles[a] = T.tiles[a] = (int)plan.tiles[a];
        T.step_cost[a] = window->step_cost[a];
    }
    X.surface_offset = window->surface_offset;
    X.wide_words_per_row = (int)plan.wide_words_per_row;
    X.words_per_row = T.words_per_row = (int)plan.words_per_row;
    X.words = T.words = plan.words;
    T.voxels = plan.voxels;
    T.level = travel_level(window->connectivity);
    T.max_cost = window->max_cost;
    T.n_tiles = plan.n_tiles;
    int *dist2 = nullptr;
    if (int rc = travel::ensure_memory(m, plan, n_seeds, X, T, &dist2, window->clearance > 0)) return rc;
    if (window->clearance > 0)
        if (int rc = ensure_distance_scratch(m, dplan, true, false)) return rc;
    if (int rc = wait_for_input(m, m->stream)) return rc;  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
    chisel_hip_map::TravelMemory &F = m->travel_mem;
    const dim3 block(TRAVEL_THREADS);
    const dim3 per_voxel(travel::blocks(plan.words, 4)), per_tile((unsigned)plan.n_tiles);
    // ---- 1. the seed
    HIP_TRY(F.ctl.zero(m->stream));
    HIP_TRY(hipMemsetAsync(T.flags, 0, 2 * (size_t)plan.n_tiles * sizeof(int), m->stream));
    HIP_TRY(hipMemcpyAsync(F.seeds.get(), seeds, (size_t)n_seeds * 3 * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    const long long n_runs = plan.wide_words;  // (a run holds a voxel of the widened window)
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(frontier_seed_kernel<N>, dim3(travel::blocks(n_runs, 4)), dim3(256), 0, m->stream, m->view, X, n_runs));
    if (dist2) launch_distance_passes(m, &dw, dplan, nullptr, dist2, nullptr);
    hipLaunchKernelGGL(travel_plane_kernel, per_voxel, block, 0, m->stream, X, (const int *)dist2, const_cast<unsigned long long *>(T.trav), T.cost, T.ctl);
    hipLaunchKernelGGL(travel_seed_kernel, dim3(travel::blocks(n_seeds, TRAVEL_THREADS)), block, 0, m->stream, T, (const int *)F.seeds.get(), (long long)n_seeds);
    // ---- 2. and 3. the rounds: a batch of launches, one look at the flagged tiles
    volatile long long *w = nullptr;
    int per_wait = TRAVEL_ROUNDS_PER_WAIT;
    if (const char *e = getenv("CHISEL_HIP_TRAVEL_ROUNDS_PER_WAIT")) {  // tuning hook of tools/travel_bench.py: 8, 16, 32 or 64
        const int v = atoi(e);
        if (v == 8 || v == 16 || v == 32 || v == 64) per_wait = v;
    }
    for (int64_t round = 0;;) {
        for (int k = 0; k < per_wait; k++, round++) hipLaunchKernelGGL(travel_round_kernel, per_tile, block, 0, m->stream, T, (int)round);
        hipLaunchKernelGGL(travel_count_kernel, dim3(1), block, 0, m->stream, T, (int)round);
        if (int rc = F.ctl.report_and_wait(m, &w)) return rc;
        if (w[TC_FLAGGED] == 0) break;
        if (round > plan.max_rounds) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": internal error: the rounds did not end within the window's voxels");
    }
    // ---- 4. the finish, the targets, the totals
    const bool with_targets = n_targets > 0;
    const size_t table_words = with_targets ? (size_t)n_groups * TRAVEL_TABLE_WORDS : 0;
    if (with_targets) {
        if (int rc = grow_buffer(F.acc, table_words, m->stream)) return rc;
        HIP_TRY(F.table_host.ensure(table_words, m->stream));
    }
    int32_t *dc = cost;
    uint8_t *dp = step, *ds = state;
    const int32_t *dt = with_targets ? targets : nullptr;
    Staging out(m->stream, on_device != 0);
    out.out(dc, (size_t)plan.voxels * sizeof(int32_t));
    out.out(dp, (size_t)plan.voxels);
    out.out(ds, (size_t)plan.voxels);
    out.in(dt, (size_t)n_targets * 4 * sizeof(int32_t));
    HIP_TRY(out.begin());
    hipLaunchKernelGGL(travel_finish_kernel, per_voxel, block, 0, m->stream, T, X, dc, dp, ds);
    if (with_targets) {
        hipLaunchKernelGGL(travel_table_init_kernel, dim3(travel::blocks((int64_t)table_words, TRAVEL_THREADS)), block, 0, m->stream, F.acc.get(), (long long)n_groups);
        hipLaunchKernelGGL(travel_targets_kernel, dim3(travel::blocks(n_targets, TRAVEL_THREADS)), block, 0, m->stream, T, (const int *)dt, (long long)n_targets,
                           (long long)n_groups, F.acc.get());
        hipLaunchKernelGGL(travel_table_kernel, dim3(travel::blocks(n_groups, TRAVEL_THREADS)), block, 0, m->stream, (const long long *)F.acc.get(), F.table_host.dev(),
                           (long long)n_groups);
    }
    travel::Totals R;
    {
        if (int rc = F.ctl.report_and_wait(m, &w)) return rc;  // (the table's rows are complete behind it too)
        R.unknown = w[TC_UNKNOWN];
        R.free = w[TC_FREE];
        R.occupied = plan.voxels - R.unknown - R.free;
        R.traversable = w[TC_TRAVERSABLE];
        R.seeds_used = w[TC_SEEDS_USED];
        R.seeds_ignored = w[TC_SEEDS_IGNORED];
        R.reached = w[TC_REACHED];
        R.largest_cost = w[TC_LARGEST] - 1;  // (-1: nothing reached)
        R.targets_reached = w[TC_TARGETS_REACHED];
        R.targets_ignored = w[TC_TARGETS_IGNORED];
        R.rounds = w[TC_ROUNDS];
        R.tile_visits = w[TC_TILE_VISITS];
    }
    hipError_t e = out.finish(hipSuccess);
    if (group_table) e = read_pinned_table(m, F.table_host, table_words, false, e, group_table);
    if (e != hipSuccess) return hip_failure(name, e);
    copy_totals(R, totals);
    return CHISEL_HIP_OK;
}

int chisel_hip_travel_path(const uint8_t *step, const int dims[3], const int from[3], int64_t capacity, int32_t *path, int64_t *length) {
    if (const char *why = travel_path_walk(step, dims, from, capacity, path, length)) return refusal("chisel_hip_travel_path", why, false);
    return CHISEL_HIP_OK;
}

}  // extern "C"

// host_distance.h -- chisel_hip_distance_field (included by chisel_hip.hip; the kernels: kernels_distance.h; the argument check, the
// widened window and the scratch sizes: distance_checks.h; the definition: DESIGN.md 3.11).  The frame is chisel_hip_query_points' own
// (host_query.h): the map is only read; with device pointers everything goes on the map's stream behind whatever was queued before and
// nothing is waited for; host arrays are staged through one owned device buffer and are complete on return.  The scratch lives in the
// map (chisel_hip_map::distance_mem), is sized from the widened window, reused by a later call that fits and freed with the map.
#pragma once

namespace {

// room for the plan's bit rows and 16-bit intermediates (grown as ensure_merge_scratch grows its table: a buffer that is replaced may
// still be read by what the stream holds, which is waited for first; one that is large enough costs nothing), and the distance table.
// An entry of the table depends on the map's resolution alone (distance_checks.h: distance_table), so the map keeps the one of the
// largest radius and uploads it once, from pinned memory that is never written again.
int ensure_distance_scratch(chisel_hip_map *m, const DistancePlan &plan, bool passes, bool want_table) {
    chisel_hip_map::DistanceMemory &O = m->distance_mem;
    if (int rc = grow_buffer(O.bits, (size_t)plan.bits_words, m->stream)) return rc;
    if (passes) {
        if (int rc = grow_buffer(O.g1, (size_t)plan.g1_elems, m->stream)) return rc;
        if (int rc = grow_buffer(O.g2, (size_t)plan.g2_elems, m->stream)) return rc;
    }
    if (want_table && !O.table) {
        const size_t n = (size_t)DISTANCE_MAX_RADIUS * DISTANCE_MAX_RADIUS + 1;
        HIP_TRY(O.table_host.alloc(n));
        distance_table(DISTANCE_MAX_RADIUS, m->cfg.voxel_resolution, O.table_host.get());
        HIP_TRY(O.table.alloc(n));
        HIP_TRY(hipMemcpyAsync(O.table.get(), O.table_host.get(), n * sizeof(float), hipMemcpyHostToDevice, m->stream));
    }
    return CHISEL_HIP_OK;
}

// The seed and, where dist2 or distance is asked for, the three passes of a call, queued on the map's stream into device memory
// (chisel_hip_travel_field launches them too, as they are, with a dist2 of its own call's scratch).  ensure_distance_scratch first.
void launch_distance_passes(chisel_hip_map *m, const chisel_hip_distance_window *window, const DistancePlan &plan, uint8_t *dstate, int32_t *dd2, float *ddist) {
    const bool passes = dd2 || ddist;
    chisel_hip_map::DistanceMemory &O = m->distance_mem;
    const int R = window->radius, nx = window->dims[0], ny = window->dims[1], nz = window->dims[2];
    DistanceSeedArgs A;
    for (int a = 0; a < 3; a++) {
        A.wo[a] = plan.wo[a];
        A.wd[a] = plan.wd[a];
        A.dims[a] = window->dims[a];
    }
    A.R = R;
    A.unknown_is_obstacle = window->unknown_is_obstacle != 0;
    A.surface_offset = window->surface_offset;
    A.words_per_row = plan.words_per_row;
    const long long n_runs = plan.bits_words;  // (<= 2^30: a run holds a voxel of the widened window)
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(distance_seed_kernel<N>, dim3((unsigned)((n_runs + 3) / 4)), dim3(256), 0, m->stream, m->view, A, n_runs, dstate,
                                            O.bits.get()));
    if (passes) {
        const long long n1 = plan.g1_elems;  // along x: every row of the widened y and z
        hipLaunchKernelGGL(distance_x_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, m->stream, O.bits.get(), (long long)plan.words_per_row, nx, n1, R,
                           O.g1.get());
        const size_t lds = (size_t)(DIST_TILE + 2 * R) * 64 * sizeof(unsigned short);
        {  // along y: every plane of the widened z
            const long long X = nx, bx = (X + 63) / 64, ba = (ny + DIST_TILE - 1) / DIST_TILE;
            hipLaunchKernelGGL(distance_axis_kernel<false>, dim3((unsigned)(bx * ba * plan.wd[2])), dim3(256), lds, m->stream, O.g1.get(), O.g2.get(),
                               (int *)nullptr, (float *)nullptr, (const float *)nullptr, X, ny, bx, ba, R);
        }
        {  // along z: the planes of the window are one contiguous dimension
            const long long X = (long long)nx * ny, bx = (X + 63) / 64, ba = (nz + DIST_TILE - 1) / DIST_TILE;
            hipLaunchKernelGGL(distance_axis_kernel<true>, dim3((unsigned)(bx * ba)), dim3(256), lds, m->stream, O.g2.get(), (unsigned short *)nullptr, dd2, ddist,
                               O.table.get(), X, nz, bx, ba, R);
        }
    }
}

}  // namespace

extern "C" {

int chisel_hip_distance_field(chisel_hip_map *m, const chisel_hip_distance_window *window, uint8_t *state, int32_t *dist2, float *distance,
                              int on_device) {
    SETTLE(m);
    {
        int rc_r = query_refusal(m, "chisel_hip_distance_field", "reads the voxels of the window and of a margin around it");
        if (rc_r) return rc_r;
    }
    DistancePlan plan;
    {
        int code = 0;
        if (const char *why = distance_refusal(window, state || dist2 || distance, &code, &plan))
            return fail(code == DISTANCE_REFUSED_UNSUPPORTED ? CHISEL_HIP_ERR_UNSUPPORTED : CHISEL_HIP_ERR_INVALID, std::string("chisel_hip_distance_field: ") + why);
    }
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
        if (rc_m) return rc_m;
    }
    const bool passes = dist2 || distance;
    {
        int rc_s = ensure_distance_scratch(m, plan, passes, distance != nullptr);
        if (rc_s) return rc_s;
    }
    const size_t cnt = (size_t)plan.voxels;
    uint8_t *dstate = state;
    int32_t *dd2 = dist2;
    float *ddist = distance;
    Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
    st.out(dstate, cnt);
    st.out(dd2, cnt * sizeof(int32_t));
    st.out(ddist, cnt * sizeof(float));
    HIP_TRY(st.begin());
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
        if (rc_w) return rc_w;
    }
    launch_distance_passes(m, window, plan, dstate, dd2, ddist);
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_distance_field: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

}  // extern "C"

// host_query.h -- chisel_hip_query_points and chisel_hip_cast_rays (included by chisel_hip.hip; the kernels: kernels_query.h).
// Both only read the map.  With device pointers the kernel goes on the map's stream behind whatever was queued before and nothing is
// waited for; host arrays are staged through one owned device buffer (host_buffer.h: Staging) and are complete on return.
// query_refusal: host_render.h.
#pragma once

extern "C" {

int chisel_hip_query_points(chisel_hip_map *m, const float *positions, int64_t n, uint8_t *found, float *sdf, float *weight, float *gradient,
                            float *colors, int on_device) {
    SETTLE(m);
    {
        int rc_r = query_refusal(m, "chisel_hip_query_points", "reads the voxels around every position");
        if (rc_r) return rc_r;
    }
    if (n < 0) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_query_points: a negative number of positions");
    if (n == 0) return CHISEL_HIP_OK;  // nothing to answer: the other arguments are not looked at
    if (n > 0 && !positions) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_query_points: null positions");
    if (!found && !sdf && !weight && !gradient && !colors) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_query_points: no output asked for");
    if (colors && !m->view.rgbw) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_query_points: colours asked of a map without colour voxels");
    if ((n + 255) / 256 > (int64_t)INT32_MAX) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_query_points: more positions than one launch takes (2^31 blocks of 256)");
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
        if (rc_m) return rc_m;
    }
    const size_t cnt = (size_t)n, f3 = cnt * 3 * sizeof(float), f1 = cnt * sizeof(float);
    const float *dp = positions;
    uint8_t *dfound = found;
    float *ds = sdf, *dw = weight, *dg = gradient, *dc = colors;
    Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
    st.in(dp, f3);
    st.out(dfound, cnt);
    st.out(ds, f1);
    st.out(dw, f1);
    st.out(dg, f3);
    st.out(dc, f3);
    HIP_TRY(st.begin());
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the positions are ready behind it
        if (rc_w) return rc_w;
    }
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((n + 255) / 256));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(query_points_kernel<N>, grid, dim3(256), 0, m->stream, m->view, P, dp, (long long)n, dfound, ds, dw, dg, dc));
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_query_points: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

int chisel_hip_cast_rays(chisel_hip_map *m, const chisel_hip_ray *rays, int64_t n, float step, float *t_hit, uint8_t *status, float *normals,
                         float *colors, int on_device) {
    static_assert(sizeof(chisel_hip_ray) == sizeof(QueryRay), "chisel_hip_ray and the kernel's QueryRay are one layout");
    SETTLE(m);
    {
        int rc_r = query_refusal(m, "chisel_hip_cast_rays", "marches every ray through the voxels");
        if (rc_r) return rc_r;
    }
    if (n < 0) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: a negative number of rays");
    if (n == 0) return CHISEL_HIP_OK;  // nothing to answer: the other arguments are not looked at
    if (n > 0 && !rays) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: null rays");
    if (!t_hit) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: null t_hit");
    if (step != step) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: the step is NaN");
    if (colors && !m->view.rgbw) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: colours asked of a map without colour voxels");
    if ((n + 255) / 256 > (int64_t)INT32_MAX) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: more rays than one launch takes (2^31 blocks of 256)");
    if (on_device && ((uintptr_t)rays & 15)) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_cast_rays: device rays must be 16-byte aligned");
    const float h = step > 0.0f ? step : m->cfg.voxel_resolution;
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
        if (rc_m) return rc_m;
    }
    const size_t cnt = (size_t)n, f3 = cnt * 3 * sizeof(float), f1 = cnt * sizeof(float);
    const QueryRay *dr = reinterpret_cast<const QueryRay *>(rays);
    uint8_t *dst = status;
    float *dt = t_hit, *dn = normals, *dc = colors;
    Staging st(m->stream, on_device != 0);
    st.in(dr, cnt * sizeof(QueryRay));
    st.out(dt, f1);
    st.out(dst, cnt);
    st.out(dn, f3);
    st.out(dc, f3);
    HIP_TRY(st.begin());
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the rays are ready behind it
        if (rc_w) return rc_w;
    }
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((n + 255) / 256));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(cast_rays_kernel<N>, grid, dim3(256), 0, m->stream, m->view, P, dr, (long long)n, h, dt, dst, dn, dc));
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_cast_rays: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

}  // extern "C"

// host_query.h -- chisel_hip_query_points and chisel_hip_cast_rays (included by chisel_hip.hip; the kernels: kernels_query.h).
// Both only read the map.  With device pointers the kernel goes on the map's stream behind whatever was queued before and nothing is
// waited for; host arrays are staged through one owned device buffer and are complete on return.
#pragma once

namespace {

// what both entries refuse before they look at their own arguments; 0 = go on
int query_refusal(chisel_hip_map *m, const char *name, const char *what) {
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " " + what + " of all owners: a group's shards hold a part each (query a map of one shard)");
    if (!m) return fail(CHISEL_HIP_ERR_INVALID, "null map");
    if (m->cfg.n_shards > 1) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " " + what + " of all owners: this map is one shard of several");
    return CHISEL_HIP_OK;
}

size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace

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
    DeviceBuffer<unsigned char> d;
    const float *dp = positions;
    uint8_t *dfound = found;
    float *ds = sdf, *dw = weight, *dg = gradient, *dc = colors;
    if (!on_device) {
        // positions | sdf | weight | gradient | colours | found: only what is asked for takes room
        size_t at = round16(f3);
        const size_t at_s = at; at += sdf ? round16(f1) : 0;
        const size_t at_w = at; at += weight ? round16(f1) : 0;
        const size_t at_g = at; at += gradient ? round16(f3) : 0;
        const size_t at_c = at; at += colors ? round16(f3) : 0;
        const size_t at_f = at; at += found ? round16(cnt) : 0;
        HIP_TRY(d.alloc(at));
        unsigned char *b = d.get();
        HIP_TRY(hipMemcpyAsync(b, positions, f3, hipMemcpyHostToDevice, m->stream));
        dp = reinterpret_cast<const float *>(b);
        ds = sdf ? reinterpret_cast<float *>(b + at_s) : nullptr;
        dw = weight ? reinterpret_cast<float *>(b + at_w) : nullptr;
        dg = gradient ? reinterpret_cast<float *>(b + at_g) : nullptr;
        dc = colors ? reinterpret_cast<float *>(b + at_c) : nullptr;
        dfound = found ? b + at_f : nullptr;
    }
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the positions are ready behind it
        if (rc_w) return rc_w;
    }
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((n + 255) / 256));
    switch (m->N) {
        case 8: hipLaunchKernelGGL(query_points_kernel<8>, grid, dim3(256), 0, m->stream, m->view, P, dp, (long long)n, dfound, ds, dw, dg, dc); break;
        case 16: hipLaunchKernelGGL(query_points_kernel<16>, grid, dim3(256), 0, m->stream, m->view, P, dp, (long long)n, dfound, ds, dw, dg, dc); break;
        case 32: hipLaunchKernelGGL(query_points_kernel<32>, grid, dim3(256), 0, m->stream, m->view, P, dp, (long long)n, dfound, ds, dw, dg, dc); break;
    }
    hipError_t e = hipGetLastError();
    if (!on_device) {  // (device outputs are left on the map's stream: nothing is waited for)
        if (e == hipSuccess && found) e = hipMemcpyAsync(found, dfound, cnt, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && sdf) e = hipMemcpyAsync(sdf, ds, f1, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && weight) e = hipMemcpyAsync(weight, dw, f1, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && gradient) e = hipMemcpyAsync(gradient, dg, f3, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && colors) e = hipMemcpyAsync(colors, dc, f3, hipMemcpyDeviceToHost, m->stream);
        const hipError_t e_sync = hipStreamSynchronize(m->stream);  // (also after a failed copy: the buffer is freed on return)
        if (e == hipSuccess) e = e_sync;
    }
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
    DeviceBuffer<unsigned char> d;
    const QueryRay *dr = reinterpret_cast<const QueryRay *>(rays);
    uint8_t *dst = status;
    float *dt = t_hit, *dn = normals, *dc = colors;
    if (!on_device) {
        // rays | t_hit | normals | colours | status
        size_t at = cnt * sizeof(QueryRay);
        const size_t at_t = at; at += round16(f1);
        const size_t at_n = at; at += normals ? round16(f3) : 0;
        const size_t at_c = at; at += colors ? round16(f3) : 0;
        const size_t at_s = at; at += status ? round16(cnt) : 0;
        HIP_TRY(d.alloc(at));
        unsigned char *b = d.get();
        HIP_TRY(hipMemcpyAsync(b, rays, cnt * sizeof(QueryRay), hipMemcpyHostToDevice, m->stream));
        dr = reinterpret_cast<const QueryRay *>(b);
        dt = reinterpret_cast<float *>(b + at_t);
        dn = normals ? reinterpret_cast<float *>(b + at_n) : nullptr;
        dc = colors ? reinterpret_cast<float *>(b + at_c) : nullptr;
        dst = status ? b + at_s : nullptr;
    }
    {
        int rc_w = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the rays are ready behind it
        if (rc_w) return rc_w;
    }
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((n + 255) / 256));
    switch (m->N) {
        case 8: hipLaunchKernelGGL(cast_rays_kernel<8>, grid, dim3(256), 0, m->stream, m->view, P, dr, (long long)n, h, dt, dst, dn, dc); break;
        case 16: hipLaunchKernelGGL(cast_rays_kernel<16>, grid, dim3(256), 0, m->stream, m->view, P, dr, (long long)n, h, dt, dst, dn, dc); break;
        case 32: hipLaunchKernelGGL(cast_rays_kernel<32>, grid, dim3(256), 0, m->stream, m->view, P, dr, (long long)n, h, dt, dst, dn, dc); break;
    }
    hipError_t e = hipGetLastError();
    if (!on_device) {
        if (e == hipSuccess) e = hipMemcpyAsync(t_hit, dt, f1, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && status) e = hipMemcpyAsync(status, dst, cnt, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && normals) e = hipMemcpyAsync(normals, dn, f3, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess && colors) e = hipMemcpyAsync(colors, dc, f3, hipMemcpyDeviceToHost, m->stream);
        const hipError_t e_sync = hipStreamSynchronize(m->stream);
        if (e == hipSuccess) e = e_sync;
    }
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_cast_rays: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

}  // extern "C"

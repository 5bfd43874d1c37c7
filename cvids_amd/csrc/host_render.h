// host_render.h -- chisel_hip_shade_vertices and chisel_hip_render_view (included by chisel_hip.hip; the kernels: kernels_mesh.h:
// shade_vertices_kernel, kernels_render.h), and what the read-only entries behind them (host_query.h, host_align.h) share with them.
// All of them only read the map; host arrays are staged through one owned device buffer (host_buffer.h: Staging) and are complete
// on return.
#pragma once

namespace {

// what the query and align entries refuse before they look at their own arguments; 0 = go on
int query_refusal(chisel_hip_map *m, const char *name, const char *what) {
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " " + what + " of all owners: a group's shards hold a part each (query a map of one shard)");
    if (!m) return fail(CHISEL_HIP_ERR_INVALID, "null map");
    if (m->cfg.n_shards > 1) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + " " + what + " of all owners: this map is one shard of several");
    return CHISEL_HIP_OK;
}

// the camera whose pixels' rays kernels_render.h: pixel_ray gives (chisel_hip_view, chisel_hip_depth_frame)
PixelCamera pixel_camera(const float pose[12], float fx, float fy, float cx, float cy) {
    PixelCamera c;
    memcpy(c.pose, pose, sizeof(c.pose));
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy;
    return c;
}

}  // namespace

extern "C" {

int chisel_hip_shade_vertices(chisel_hip_map *m, const float *vertices, int64_t n, float *normals, float *colors, int stages) {
    SETTLE(m);
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_shade_vertices reads the voxels around every vertex: ask the shard that owns them (a group's meshes are shaded by chisel_hip_update_meshes)");
    if (!m || n < 0 || (n > 0 && !vertices)) return fail(CHISEL_HIP_ERR_INVALID, "bad argument");
    if (n == 0) return CHISEL_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);
        if (rc_m) return rc_m;
    }
    // (a stage that is off, or has nowhere to go, is not run: the kernel takes the null pointer for it)
    const size_t f3 = (size_t)n * 3 * sizeof(float);
    const float *dv = vertices;
    float *dn = (stages & 1) ? normals : nullptr, *dc = (stages & 2) && m->view.rgbw ? colors : nullptr;
    Staging st(m->stream, false);
    st.in(dv, f3);
    st.inout(dn, f3);  // a normal is replaced only where the gradient lookup succeeds
    st.out(dc, f3);
    HIP_TRY(st.begin());
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((n + 255) / 256));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(shade_vertices_kernel<N>, grid, dim3(256), 0, m->stream, m->view, P, dv, (long long)n, dn, dc, stages));
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_shade_vertices: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

// One ray march per pixel over the voxels as they are (kernels_render.h; DESIGN.md "Rendering a view"): the map is only read.
int chisel_hip_render_view(chisel_hip_map *m, const chisel_hip_view *view, float *depth, float *normals, float *colors, int on_device) {
    SETTLE(m);
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_render_view marches every ray through the voxels of all owners: a group's shards hold a part each (render a map of one shard)");
    if (!m || !view || !depth) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    if (m->cfg.n_shards > 1) return fail(CHISEL_HIP_ERR_UNSUPPORTED, "chisel_hip_render_view marches every ray through the voxels of all owners: this map is one shard of several");
    if (view->width < 1 || view->height < 1) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_render_view: non-positive image size");
    if (colors && !m->view.rgbw) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_render_view: colours asked of a map without colour voxels");
    RenderCamera cam;
    cam.cam = pixel_camera(view->pose, view->fx, view->fy, view->cx, view->cy);
    cam.near_plane = view->near_plane;
    cam.step = view->step > 0.0f ? view->step : m->cfg.voxel_resolution;
    cam.width = view->width; cam.height = view->height;
    const float last = floorf((view->far_plane - view->near_plane) / cam.step);  // K = (int)floorf((far - near) / step) + 1
    if (!(last >= 0.0f) || last > (float)(RENDER_MAX_SAMPLES - 1)) return fail(CHISEL_HIP_ERR_INVALID, "chisel_hip_render_view: (far - near) / step gives less than 1 or more than 65536 samples per ray");
    cam.n_samples = (int)last + 1;
    HIP_TRY(hipSetDevice(m->device));
    {
        int rc_m = check_mesh_totals(m);
        if (rc_m) return rc_m;
    }
    const size_t f1 = (size_t)view->width * view->height * sizeof(float);
    float *dd = depth, *dn = normals, *dc = colors;
    Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
    st.out(dd, f1);
    st.out(dn, 3 * f1);
    st.out(dc, 3 * f1);
    HIP_TRY(st.begin());
    const MeshParams P = mesh_params(m);
    const dim3 grid((unsigned)((view->width + 15) / 16), (unsigned)((view->height + 15) / 16));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(render_view_kernel<N>, grid, dim3(256), 0, m->stream, m->view, P, cam, dd, dn, dc));
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string("chisel_hip_render_view: ") + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

}  // extern "C"

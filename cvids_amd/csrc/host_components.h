// host_components.h -- chisel_hip_mesh_components and chisel_hip_filter_mesh (included by chisel_hip.hip; the kernels:
// kernels_components.h; the refusals and the size arithmetic: components_checks.h; the definition: DESIGN.md 3.16).  The frame
// of host_totals.h; the map is neither read nor written, and a chisel_hip_indexed_mesh(on_device) queued before, whose outputs are
// this call's inputs, is in front of it on the stream.  In front of the wait: label() -- init, hook, label, the scans.  The component
// table is host memory whatever on_device says (the number of its rows is a total).  Scratch: chisel_hip_map::components_mem.
#pragma once

namespace {
namespace components {

struct Totals {
    int64_t vertices, triangles, invalid_triangles, components, largest_triangles, kept_components, kept_vertices, kept_triangles;
};

inline unsigned tiles(int64_t n) { return (unsigned)components_tiles(n); }

// the scratch of a call of V vertices and T triangles, carved out of one buffer of ints, and the view on it
int ensure_memory(chisel_hip_map *m, int64_t V, int64_t T, ComponentsView &X) {
    chisel_hip_map::ComponentsMemory &C = m->components_mem;
    const size_t v = (size_t)V, t = (size_t)T, n_sums = (size_t)components_tiles(std::max(V, T));
    if (int rc = grow_ints(m, C.words, 6 * v + t + n_sums)) return rc;
    if (int rc = C.ctl.prepare(m, COMPONENTS_HOST_WORDS)) return rc;
    int *p = C.words.get();
    X.parent = p;
    X.root_of = p + v;
    X.vertex_count = p + 2 * v;
    X.tri_count = p + 3 * v;
    X.number = p + 4 * v;
    X.vertex_prefix = p + 5 * v;
    X.tri_prefix = p + 6 * v;
    X.sums = p + 6 * v + t;
    X.ctl = C.ctl.dev();
    return CHISEL_HIP_OK;
}

template <int F>
void scan(chisel_hip_map *m, const ComponentsView &X, int64_t n, int word) {
    if (n == 0) return;
    const dim3 grid(tiles(n)), block(COMPONENTS_TILE);
    hipLaunchKernelGGL(components_sums_kernel<F>, grid, block, 0, m->stream, X);
    hipLaunchKernelGGL(components_scan_sums_kernel, dim3(1), block, 0, m->stream, X.sums, (int)tiles(n), X.ctl, word);
    hipLaunchKernelGGL(components_prefix_kernel<F>, grid, block, 0, m->stream, X);
}

// Everything in front of the wait, then the wait: the components of X.indices, with `filter` the kept flags' prefixes too. -> T
int label(chisel_hip_map *m, ComponentsView &X, bool filter, Totals &T) {
    chisel_hip_map::ComponentsMemory &C = m->components_mem;
    const dim3 per_vertex(tiles(X.V)), per_triangle(tiles(X.T)), block(COMPONENTS_TILE);
    HIP_TRY(C.ctl.zero(m->stream));
    if (X.V) hipLaunchKernelGGL(components_init_kernel, per_vertex, block, 0, m->stream, X);
    if (X.V && X.T) hipLaunchKernelGGL(components_hook_kernel, per_triangle, block, 0, m->stream, X);
    if (X.V) hipLaunchKernelGGL(components_label_vertices_kernel, per_vertex, block, 0, m->stream, X);
    if (X.T) hipLaunchKernelGGL(components_label_triangles_kernel, per_triangle, block, 0, m->stream, X);
    scan<FLAG_ROOT>(m, X, X.V, CC_COMPONENTS);
    if (filter) {
        scan<FLAG_KEPT_VERTEX>(m, X, X.V, CC_KEPT_VERTICES);
        if (X.V) scan<FLAG_KEPT_TRIANGLE>(m, X, X.T, CC_KEPT_TRIANGLES);  // (without a vertex no triangle is valid)
    }
    volatile long long *w;
    if (int rc = C.ctl.report_and_wait(m, &w)) return rc;
    T.vertices = X.V;
    T.triangles = X.T;
    T.invalid_triangles = w[CC_INVALID];
    T.components = w[CC_COMPONENTS];
    T.largest_triangles = T.components ? components_key_triangles((uint64_t)w[CC_LARGEST_KEY]) : 0;
    T.kept_components = w[CC_KEPT_COMPONENTS];
    T.kept_vertices = w[CC_KEPT_VERTICES];
    T.kept_triangles = w[CC_KEPT_TRIANGLES];
    return CHISEL_HIP_OK;
}

int run_components(chisel_hip_map *m, const char *name, int64_t V, int64_t T_, const int32_t *indices, int on_device, int32_t *vertex_component,
                   int32_t *triangle_component, int64_t capacity_components, int64_t *component_table, chisel_hip_components_totals *totals) {
    // ---- refusals that need no device
    int rc = begin_on_one_device(m, name);
    if (rc) return rc;
    bool unsupported = false;
    if (const char *why = components_request_refusal(V, T_, indices, vertex_component, triangle_component, capacity_components, component_table, totals, &unsupported))
        return refusal(name, why, unsupported);
    Totals T{V, T_, 0, 0, 0, 0, 0, 0};
    if (V == 0 && T_ == 0) {  // nothing is launched
        copy_totals(T, totals);
        return CHISEL_HIP_OK;
    }
    // ---- the input, the scratch, the labels, the wait
    ComponentsView X{};
    X.V = (int)V;
    X.T = (int)T_;
    X.min_triangles = 1;
    if ((rc = ensure_memory(m, V, T_, X))) return rc;
    if ((rc = wait_for_input(m, m->stream))) return rc;  // chisel_hip_wait_event / _order_map_after_stream: the arrays are ready behind it
    const int32_t *d_indices = T_ ? indices : nullptr;
    Staging in(m->stream, on_device != 0);
    in.in(d_indices, (size_t)T_ * 3 * sizeof(int32_t));
    HIP_TRY(in.begin());
    X.indices = d_indices;
    if ((rc = label(m, X, false, T))) return rc;
    if (const char *why = components_capacity_refusal(T.components, capacity_components, component_table)) {
        copy_totals(T, totals);  // (the caller can retry)
        return refusal(name, why, false);
    }
    // ---- the labels and the table
    chisel_hip_map::ComponentsMemory &C = m->components_mem;
    const bool table = component_table && capacity_components > 0 && T.components > 0;
    if (table) HIP_TRY(C.table_host.ensure(3 * (size_t)T.components, m->stream));
    int32_t *dv = V ? vertex_component : nullptr, *dt = T_ ? triangle_component : nullptr;
    if (dv || dt || table) {
        Staging out(m->stream, on_device != 0);
        out.out(dv, (size_t)V * sizeof(int32_t));
        out.out(dt, (size_t)T_ * sizeof(int32_t));
        HIP_TRY(out.begin());
        const dim3 block(COMPONENTS_TILE);
        if (dv) hipLaunchKernelGGL(components_write_vertices_kernel, dim3(tiles(V)), block, 0, m->stream, X, dv);
        if (dt) hipLaunchKernelGGL(components_write_triangles_kernel, dim3(tiles(T_)), block, 0, m->stream, X, dt);
        if (table) hipLaunchKernelGGL(components_write_table_kernel, dim3(tiles(V)), block, 0, m->stream, X, C.table_host.dev(), (long long)T.components);
        hipError_t e = out.finish(hipGetLastError());
        if (table) e = read_pinned_table(m, C.table_host, 3 * (size_t)T.components, on_device != 0, e, component_table);
        if (e != hipSuccess) return hip_failure(name, e);
    }
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

int run_filter(chisel_hip_map *m, const char *name, int64_t V, int64_t T_, const int32_t *indices, const float *vertices, const float *normals, const float *colors,
               int64_t min_triangles, int largest_only, int64_t capacity_vertices, int64_t capacity_triangles, float *out_vertices, int32_t *out_indices,
               float *out_normals, float *out_colors, int32_t *vertex_map, int32_t *triangle_map, int on_device, chisel_hip_components_totals *totals) {
    // ---- refusals that need no device
    int rc = begin_on_one_device(m, name);
    if (rc) return rc;
    bool unsupported = false;
    if (const char *why = filter_request_refusal(V, T_, indices, vertices, normals, colors, min_triangles, largest_only, capacity_vertices, capacity_triangles,
                                                 out_vertices, out_indices, out_normals, out_colors, totals, &unsupported))
        return refusal(name, why, unsupported);
    const bool query = capacity_vertices == 0 && capacity_triangles == 0;
    Totals T{V, T_, 0, 0, 0, 0, 0, 0};
    if (V == 0 && T_ == 0) {  // nothing is launched
        copy_totals(T, totals);
        return CHISEL_HIP_OK;
    }
    // ---- the inputs, the scratch, the labels and the kept flags' prefixes, the wait
    ComponentsView X{};
    X.V = (int)V;
    X.T = (int)T_;
    X.min_triangles = (int)std::min<int64_t>(min_triangles, COMPONENTS_MAX_INTS);  // (no component has 2^31 - 1 triangles: none is kept)
    X.largest_only = largest_only;
    if ((rc = ensure_memory(m, V, T_, X))) return rc;
    if ((rc = wait_for_input(m, m->stream))) return rc;
    const bool rows = !query && out_vertices && V;  // (the float rows are read only where they are written)
    const size_t f3 = (size_t)V * 3 * sizeof(float);
    const int32_t *d_indices = T_ ? indices : nullptr;
    const float *sv = rows ? vertices : nullptr, *sn = rows && out_normals ? normals : nullptr, *sc = rows && out_colors ? colors : nullptr;
    Staging in(m->stream, on_device != 0);
    in.in(d_indices, (size_t)T_ * 3 * sizeof(int32_t));
    in.in(sv, f3);
    in.in(sn, f3);
    in.in(sc, f3);
    HIP_TRY(in.begin());
    X.indices = d_indices;
    if ((rc = label(m, X, true, T))) return rc;
    if (!query) {
        if (const char *why = filter_capacity_refusal(T.kept_vertices, T.kept_triangles, capacity_vertices, capacity_triangles, out_vertices, out_indices)) {
            copy_totals(T, totals);  // (the caller can retry)
            return refusal(name, why, false);
        }
        // ---- the maps, the renumbered ids, the copied rows
        const size_t k3 = (size_t)T.kept_vertices * 3 * sizeof(float);
        float *dv = T.kept_vertices ? out_vertices : nullptr, *dn = T.kept_vertices ? out_normals : nullptr, *dc = T.kept_vertices ? out_colors : nullptr;
        int32_t *di = T.kept_triangles ? out_indices : nullptr, *dvm = V ? vertex_map : nullptr, *dtm = T_ ? triangle_map : nullptr;
        Staging out(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
        out.out(dv, k3);
        out.out(di, (size_t)T.kept_triangles * 3 * sizeof(int32_t));
        out.out(dn, k3);
        out.out(dc, k3);
        out.out(dvm, (size_t)V * sizeof(int32_t));
        out.out(dtm, (size_t)T_ * sizeof(int32_t));
        HIP_TRY(out.begin());
        const dim3 block(COMPONENTS_TILE);
        if (dv || dvm)
            hipLaunchKernelGGL(filter_vertices_kernel, dim3(tiles(V)), block, 0, m->stream, X, (const unsigned *)sv, (const unsigned *)sn, (const unsigned *)sc, (unsigned *)dv,
                               (unsigned *)dn, (unsigned *)dc, dvm);
        if (di || dtm) hipLaunchKernelGGL(filter_triangles_kernel, dim3(tiles(T_)), block, 0, m->stream, X, di, dtm);
        const hipError_t e = out.finish(hipGetLastError());
        if (e != hipSuccess) return hip_failure(name, e);
    }
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // namespace components
}  // namespace

extern "C" {

int chisel_hip_mesh_components(chisel_hip_map *m, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, int on_device, int32_t *vertex_component,
                               int32_t *triangle_component, int64_t capacity_components, int64_t *component_table, chisel_hip_components_totals *totals) {
    static_assert(sizeof(chisel_hip_components_totals) == 64, "chisel_hip_components_totals is 64 bytes");
    if (m && !m->is_group) SETTLE(m);
    return components::run_components(m, "chisel_hip_mesh_components", n_vertices, n_triangles, indices, on_device, vertex_component, triangle_component,
                                      capacity_components, component_table, totals);
}

int chisel_hip_filter_mesh(chisel_hip_map *m, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, const float *vertices, const float *normals,
                           const float *colors, int64_t min_triangles, int largest_only, int64_t capacity_vertices, int64_t capacity_triangles, float *out_vertices,
                           int32_t *out_indices, float *out_normals, float *out_colors, int32_t *vertex_map, int32_t *triangle_map, int on_device,
                           chisel_hip_components_totals *totals) {
    if (m && !m->is_group) SETTLE(m);
    return components::run_filter(m, "chisel_hip_filter_mesh", n_vertices, n_triangles, indices, vertices, normals, colors, min_triangles, largest_only,
                                  capacity_vertices, capacity_triangles, out_vertices, out_indices, out_normals, out_colors, vertex_map, triangle_map, on_device, totals);
}

}  // extern "C"

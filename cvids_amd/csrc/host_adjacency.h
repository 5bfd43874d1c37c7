// host_adjacency.h -- chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh (included by
// chisel_hip.hip; the kernels: kernels_adjacency.h; the refusals, the valence limit and the scratch arithmetic: adjacency_checks.h; the
// definition: DESIGN.md 3.17).  The frame of host_totals.h; the map is neither read nor written.  In front of the wait: build() -- count, scan,
// fill, rows, scan: the whole structure, in the map's scratch, so that the compact neighbour arrays need no wait of their own.
// Behind it the valence limit stands in front of the capacities.  Scratch: chisel_hip_map::adjacency_mem.
#pragma once

namespace {
namespace adjacency {

struct Totals {
    int64_t vertices, triangles, invalid_triangles, incidences, neighbors, max_incident, max_neighbors, boundary_vertices, nonmanifold_vertices, isolated_vertices,
        pinned_vertices, reserved;
};

inline unsigned tiles(int64_t n) { return (unsigned)components_tiles(n); }

// the scratch of a call of V vertices and T triangles, carved out of one buffer of ints, and the view on it
int ensure_memory(chisel_hip_map *m, int64_t V, int64_t T, AdjacencyView &X) {
    chisel_hip_map::AdjacencyMemory &A = m->adjacency_mem;
    const size_t v = (size_t)V, t = (size_t)T;
    if (int rc = grow_ints(m, A.words, (size_t)adjacency_scratch_ints(V, T))) return rc;
    if (int rc = A.ctl.prepare(m, ADJACENCY_HOST_WORDS)) return rc;
    int *p = A.words.get();
    X.deg = p;
    X.cursor = p + v;
    X.nbr_count = p + 2 * v;
    X.flags = p + 3 * v;
    X.tri_off = p + 4 * v;
    X.nbr_off = p + 5 * v + 1;
    X.tri_items = p + 6 * v + 2;
    X.nbr_rows = p + 6 * v + 2 + 3 * t;
    X.sums = p + 6 * v + 2 + 9 * t;
    X.maxes = X.sums + (size_t)adjacency_scan_tiles(V);
    X.ctl = A.ctl.dev();
    return CHISEL_HIP_OK;
}

// values[n] -> prefix[n + 1], the total into ctl[total_word], the maximum into ctl[max_word]
void scan(chisel_hip_map *m, const AdjacencyView &X, const int *values, int n, int *prefix, int total_word, int max_word) {
    const dim3 grid(tiles((int64_t)n + 1)), block(COMPONENTS_TILE);
    hipLaunchKernelGGL(adjacency_sums_kernel, grid, block, 0, m->stream, values, n, X.sums, X.maxes);
    hipLaunchKernelGGL(adjacency_scan_sums_kernel, dim3(1), block, 0, m->stream, X.sums, (const int *)X.maxes, (int)grid.x, X.ctl, total_word, max_word);
    hipLaunchKernelGGL(adjacency_prefix_kernel, grid, block, 0, m->stream, values, n, (const int *)X.sums, prefix);
}

// Everything in front of the wait, then the wait: the sorted incidence rows, the neighbour rows and the flags of X.indices in the
// scratch. -> T
int build(chisel_hip_map *m, AdjacencyView &X, Totals &T) {
    chisel_hip_map::AdjacencyMemory &A = m->adjacency_mem;
    const dim3 per_triangle(tiles(X.T)), block(COMPONENTS_TILE);
    HIP_TRY(A.ctl.zero(m->stream));
    if (X.V) HIP_TRY(hipMemsetAsync(X.deg, 0, 2 * (size_t)X.V * sizeof(int), m->stream));  // deg and cursor
    if (X.T) hipLaunchKernelGGL(adjacency_count_kernel, per_triangle, block, 0, m->stream, X);
    scan(m, X, X.deg, X.V, X.tri_off, AC_INCIDENCES, AC_MAX_INCIDENT);
    if (X.V && X.T) hipLaunchKernelGGL(adjacency_fill_kernel, per_triangle, block, 0, m->stream, X);
    if (X.V)
        hipLaunchKernelGGL(adjacency_rows_kernel, dim3((unsigned)((X.V + ADJACENCY_ROWS_THREADS - 1) / ADJACENCY_ROWS_THREADS)), dim3(ADJACENCY_ROWS_THREADS), 0, m->stream, X);
    scan(m, X, X.nbr_count, X.V, X.nbr_off, AC_NEIGHBORS, AC_MAX_NEIGHBORS);
    volatile long long *w;
    if (int rc = A.ctl.report_and_wait(m, &w)) return rc;
    T.vertices = X.V;
    T.triangles = X.T;
    T.invalid_triangles = w[AC_INVALID];
    T.incidences = w[AC_INCIDENCES];
    T.neighbors = w[AC_NEIGHBORS];
    T.max_incident = w[AC_MAX_INCIDENT];
    T.max_neighbors = w[AC_MAX_NEIGHBORS];
    T.boundary_vertices = w[AC_BOUNDARY];
    T.nonmanifold_vertices = w[AC_NONMANIFOLD];
    T.isolated_vertices = w[AC_ISOLATED];
    T.pinned_vertices = w[AC_PINNED];
    T.reserved = 0;
    return CHISEL_HIP_OK;
}

// refusals that need no device are over: the view, the scratch, the staged indices (and vertices), build(), the valence limit
struct Call {
    chisel_hip_map *m;
    const char *name;
    AdjacencyView X{};
    Totals T{};
    Staging in;
    const int32_t *d_indices;
    const float *d_vertices;
    Call(chisel_hip_map *m_, const char *name_, int on_device) : m(m_), name(name_), in(m_->stream, on_device != 0), d_indices(nullptr), d_vertices(nullptr) {}

    int run(int64_t V, int64_t T_, const int32_t *indices, const float *vertices, int pin_flags, bool count_pinned, chisel_hip_adjacency_totals *totals) {
        X.V = (int)V;
        X.T = (int)T_;
        X.pin_flags = pin_flags;
        X.count_pinned = count_pinned ? 1 : 0;
        int rc = ensure_memory(m, V, T_, X);
        if (rc) return rc;
        if ((rc = wait_for_input(m, m->stream))) return rc;  // chisel_hip_wait_event / _order_map_after_stream: the arrays are ready behind it
        d_indices = T_ ? indices : nullptr;
        d_vertices = V ? vertices : nullptr;
        in.in(d_indices, (size_t)T_ * 3 * sizeof(int32_t));
        in.in(d_vertices, (size_t)V * 3 * sizeof(float));
        HIP_TRY(in.begin());
        X.indices = d_indices;
        if ((rc = build(m, X, T))) return rc;
        if (const char *why = adjacency_valence_refusal(T.max_incident)) {
            copy_totals(T, totals);  // (max_incident says how large it was)
            return refusal(name, why, true);
        }
        return CHISEL_HIP_OK;
    }
};

void launch_normals(chisel_hip_map *m, const AdjacencyView &X, const float *P, float *normals) {
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(tiles(X.V)), dim3(COMPONENTS_TILE), 0, m->stream, X, P, normals);
}

int run_adjacency(chisel_hip_map *m, const char *name, int64_t V, int64_t T_, const int32_t *indices, int on_device, int32_t *tri_offsets, int64_t capacity_incidence,
                  int32_t *tri_items, int32_t *nbr_offsets, int64_t capacity_neighbors, int32_t *nbr_items, int32_t *vertex_flags, chisel_hip_adjacency_totals *totals) {
    int rc = begin_on_one_device(m, name);
    if (rc) return rc;
    bool unsupported = false;
    if (const char *why = adjacency_request_refusal(V, T_, indices, tri_offsets, capacity_incidence, tri_items, nbr_offsets, capacity_neighbors, nbr_items, vertex_flags,
                                                    totals, &unsupported))
        return refusal(name, why, unsupported);
    Call call(m, name, on_device);
    if ((rc = call.run(V, T_, indices, nullptr, 0, false, totals))) return rc;
    const Totals &T = call.T;
    const AdjacencyView &X = call.X;
    if (const char *why = adjacency_capacity_refusal(T.incidences, T.neighbors, capacity_incidence, tri_items, capacity_neighbors, nbr_items)) {
        copy_totals(T, totals);  // (the caller can retry)
        return refusal(name, why, false);
    }
    // ---- the caller's arrays: copies of the scratch, and the compacted neighbour rows
    int32_t *d_ti = T.incidences ? tri_items : nullptr, *d_ni = T.neighbors ? nbr_items : nullptr, *d_fl = V ? vertex_flags : nullptr;
    if (tri_offsets || d_ti || nbr_offsets || d_ni || d_fl) {
        Staging out(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
        const size_t offsets = ((size_t)V + 1) * sizeof(int32_t);
        out.out(tri_offsets, offsets);
        out.out(d_ti, (size_t)T.incidences * sizeof(int32_t));
        out.out(nbr_offsets, offsets);
        out.out(d_ni, (size_t)T.neighbors * sizeof(int32_t));
        out.out(d_fl, (size_t)V * sizeof(int32_t));
        HIP_TRY(out.begin());
        hipError_t e = hipSuccess;
        const auto copy = [&](int32_t *to, const int *from, size_t bytes) {
            if (to && e == hipSuccess) e = hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, m->stream);
        };
        copy(tri_offsets, X.tri_off, offsets);
        copy(d_ti, X.tri_items, (size_t)T.incidences * sizeof(int32_t));
        copy(nbr_offsets, X.nbr_off, offsets);
        copy(d_fl, X.flags, (size_t)V * sizeof(int32_t));
        if (d_ni && e == hipSuccess) {
            hipLaunchKernelGGL(adjacency_compact_kernel, dim3(tiles(V)), dim3(COMPONENTS_TILE), 0, m->stream, X, d_ni);
            e = hipGetLastError();
        }
        e = out.finish(e);
        if (e != hipSuccess) return hip_failure(name, e);
    }
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

int run_normals(chisel_hip_map *m, const char *name, int64_t V, int64_t T_, const int32_t *indices, const float *vertices, int on_device, float *normals,
                chisel_hip_adjacency_totals *totals) {
    int rc = begin_on_one_device(m, name);
    if (rc) return rc;
    bool unsupported = false;
    if (const char *why = normals_request_refusal(V, T_, indices, vertices, normals, totals, &unsupported)) return refusal(name, why, unsupported);
    Call call(m, name, on_device);
    if ((rc = call.run(V, T_, indices, normals ? vertices : nullptr, 0, false, totals))) return rc;  // (the positions are read only where normals are written)
    float *d_normals = V ? normals : nullptr;
    if (d_normals) {
        Staging out(m->stream, on_device != 0);
        out.out(d_normals, (size_t)V * 3 * sizeof(float));
        HIP_TRY(out.begin());
        launch_normals(m, call.X, call.d_vertices, d_normals);
        const hipError_t e = out.finish(hipGetLastError());
        if (e != hipSuccess) return hip_failure(name, e);
    }
    copy_totals(call.T, totals);
    return CHISEL_HIP_OK;
}

int run_smooth(chisel_hip_map *m, const char *name, int64_t V, int64_t T_, const int32_t *indices, const float *vertices, int64_t iterations, float lambda, float mu,
               int pin_flags, int on_device, float *out_vertices, float *out_normals, chisel_hip_adjacency_totals *totals) {
    int rc = begin_on_one_device(m, name);
    if (rc) return rc;
    bool unsupported = false;
    if (const char *why = smooth_request_refusal(V, T_, indices, vertices, iterations, lambda, mu, pin_flags, out_vertices, out_normals, totals, &unsupported))
        return refusal(name, why, unsupported);
    const int64_t passes = smooth_passes(iterations, mu);
    if (out_vertices && V && passes > 1) {  // the other buffer of the ping-pong
        if ((rc = grow_buffer(m->adjacency_mem.positions, 3 * (size_t)V, m->stream))) return rc;
    }
    Call call(m, name, on_device);
    if ((rc = call.run(V, T_, indices, out_vertices ? vertices : nullptr, pin_flags, true, totals))) return rc;
    float *d_out = V ? out_vertices : nullptr, *d_normals = V ? out_normals : nullptr;
    if (d_out) {
        const size_t bytes = (size_t)V * 3 * sizeof(float);
        Staging out(m->stream, on_device != 0);
        out.out(d_out, bytes);
        out.out(d_normals, bytes);
        HIP_TRY(out.begin());
        hipError_t e = hipSuccess;
        if (passes == 0) e = hipMemcpyAsync(d_out, call.d_vertices, bytes, hipMemcpyDeviceToDevice, m->stream);
        const float *from = call.d_vertices;
        float *other = m->adjacency_mem.positions.get();
        for (int64_t j = 0; j < passes; j++) {  // a pass reads only what the pass before it wrote; the last one writes the caller's array
            float *to = smooth_pass_writes_out(j, passes) ? d_out : other;
            const float f = mu != 0.0f && (j & 1) ? mu : lambda;
            hipLaunchKernelGGL(mesh_smooth_pass_kernel, dim3(tiles(V)), dim3(COMPONENTS_TILE), 0, m->stream, call.X, from, to, f);
            from = to;
        }
        if (d_normals) launch_normals(m, call.X, d_out, d_normals);
        if (e == hipSuccess) e = hipGetLastError();
        e = out.finish(e);
        if (e != hipSuccess) return hip_failure(name, e);
    }
    copy_totals(call.T, totals);
    return CHISEL_HIP_OK;
}

}  // namespace adjacency
}  // namespace

extern "C" {

int chisel_hip_mesh_adjacency(chisel_hip_map *m, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, int on_device, int32_t *tri_offsets,
                              int64_t capacity_incidence, int32_t *tri_items, int32_t *nbr_offsets, int64_t capacity_neighbors, int32_t *nbr_items, int32_t *vertex_flags,
                              chisel_hip_adjacency_totals *totals) {
    static_assert(sizeof(chisel_hip_adjacency_totals) == 96, "chisel_hip_adjacency_totals is 96 bytes");
    if (m && !m->is_group) SETTLE(m);
    return adjacency::run_adjacency(m, "chisel_hip_mesh_adjacency", n_vertices, n_triangles, indices, on_device, tri_offsets, capacity_incidence, tri_items, nbr_offsets,
                                    capacity_neighbors, nbr_items, vertex_flags, totals);
}

int chisel_hip_mesh_vertex_normals(chisel_hip_map *m, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, const float *vertices, int on_device,
                                   float *normals, chisel_hip_adjacency_totals *totals) {
    if (m && !m->is_group) SETTLE(m);
    return adjacency::run_normals(m, "chisel_hip_mesh_vertex_normals", n_vertices, n_triangles, indices, vertices, on_device, normals, totals);
}

int chisel_hip_smooth_mesh(chisel_hip_map *m, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, const float *vertices, int iterations, float lambda,
                           float mu, int pin_flags, int on_device, float *out_vertices, float *out_normals, chisel_hip_adjacency_totals *totals) {
    if (m && !m->is_group) SETTLE(m);
    return adjacency::run_smooth(m, "chisel_hip_smooth_mesh", n_vertices, n_triangles, indices, vertices, iterations, lambda, mu, pin_flags, on_device, out_vertices,
                                 out_normals, totals);
}

}  // extern "C"

// host_indexed.h -- chisel_hip_indexed_mesh (included by chisel_hip.hip; the kernels: kernels_indexed.h; the request checks, the
// extras and the size arithmetic: indexed_checks.h; the definition: DESIGN.md 3.15).  A reader with the coarse mesh's frame
// (host_coarse.h), whose selection, stride and stages it takes: the map is only read; everything is queued on the map's stream behind
// what was queued before.  The entry reads top to bottom: refusals, the selection, the OWNERS (the selected chunks, then the + neighbours
// that are not selected, ascending -- candidates: whether one is resident is looked up on the device and read with the totals), the
// scratch, mark / rows / scan, THE WAIT for the totals (pinned memory), the capacities, then vertices, indices and shade -- with device
// pointers nothing is waited for behind them; host arrays are staged through one owned device buffer and are complete on return.
// The frame's steps are the coarse mesh's own functions (coarse::begin, wait_for_totals, shade_and_finish, copy_rows); what stands
// written out here is what only this entry does.
//
// Waits: a list of ids costs the one wait for the totals; "every resident chunk" and a box also wait for the listing of the resident
// chunks (chunks::select), as the coarse mesh does.
//
// Scratch the map owns (chisel_hip_map::indexed_mem; ids and slots: chunk_mem), grown on demand, freed with the map.
#pragma once

namespace {
namespace indexed {

struct Totals {
    int64_t chunks, owners, cubes_meshed, vertices, triangles;
};

// the scratch of a call of n selected chunks and n_owners owners with `words` mask words (doubled when it grows)
int ensure_memory(chisel_hip_map *m, size_t n, size_t n_owners, size_t words) {
    chisel_hip_map::IndexedMemory &X = m->indexed_mem;
    auto doubled = [](size_t need, size_t have) { return need <= have ? have : std::max<size_t>(std::max<size_t>(need, 2 * have), 1024); };
    int rc = grow_buffer(X.counts, 2 * doubled(n, X.counts.size() / 2), m->stream);  // (waits for the stream before it replaces a buffer)
    if (!rc) rc = grow_buffer(X.tri_first, doubled(n, X.tri_first.size()), m->stream);
    if (!rc) rc = grow_buffer(X.owner_counts, doubled(n_owners, X.owner_counts.size()), m->stream);
    if (!rc) rc = grow_buffer(X.owner_first, doubled(n_owners, X.owner_first.size()), m->stream);
    if (!rc) rc = grow_buffer(X.owner_of_slot, (size_t)std::max(m->view.committed, 1), m->stream);
    if (!rc) rc = grow_buffer(X.masks, doubled(words, X.masks.size()), m->stream);
    if (!rc) rc = grow_buffer(X.prefix, doubled(words, X.prefix.size()), m->stream);
    if (rc) return rc;
    HIP_TRY(X.host.ensure(INDEXED_HOST_WORDS + 2 * n + 2 * n_owners, m->stream));
    return CHISEL_HIP_OK;
}

int run(chisel_hip_map *m, const char *name, const chisel_hip_coarse_request *req, int64_t capacity_vertices, int64_t capacity_triangles, float *vertices,
        int32_t *indices, float *normals, float *colors, int on_device, int64_t *chunk_table, int64_t *owner_table, int *owner_ids_xyz,
        chisel_hip_indexed_totals *totals) {
    // ---- refusals that need no device
    int rc = query_refusal(m, name, "takes the ends of an edge on a + face from the neighbour chunk");
    if (rc) return rc;
    int64_t bad_id = -1;
    if (const char *why = indexed_request_refusal(req, m->N, capacity_vertices, capacity_triangles, vertices, indices, normals, colors, chunk_table, owner_table,
                                                  owner_ids_xyz, m->cfg.use_color != 0, ID_BIAS - 2, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, chunks::with_index(name, bad_id, why));
    const bool query = capacity_vertices == 0 && capacity_triangles == 0;
    rc = coarse::begin(m, name, query, totals != nullptr);
    if (rc) return rc;

    // ---- the selection and the owners: ids on the host, slots by a look-up queued in front of the mark
    const chisel_hip_chunk_request *sel = &req->chunks;
    const bool listed = sel->ids_xyz != nullptr;
    std::vector<int> ids;
    int64_t n = listed ? sel->n_ids : 0;
    if (!listed) {  // (the listing is sorted on the host: a wait of its own)
        std::vector<int> slots;
        bool table_ready = false;
        rc = chunks::select(m, name, sel, ids, slots, table_ready);
        if (rc) return rc;
        n = (int64_t)slots.size();
    }
    if (n > CHUNK_MAX_CHUNKS / 8) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": more chunks than one call takes (2^28 - 1)");
    if (listed) ids.assign(sel->ids_xyz, sel->ids_xyz + 3 * (size_t)n);
    Totals T{n, n, 0, 0, 0};
    if (n == 0) {  // an empty map, a box without chunks: nothing is launched
        copy_totals(T, totals);
        return CHISEL_HIP_OK;
    }
    if (listed || sel->use_box) {  // ("every resident chunk" has no extras: a resident neighbour is selected)
        const std::vector<int> extras = indexed_extras(ids.data(), n, ID_BIAS - 2);
        ids.insert(ids.end(), extras.begin(), extras.end());
    }
    const int64_t n_owners = (int64_t)(ids.size() / 3);
    const int s = req->stride;
    const int rows = (int)indexed_rows(m->N, s);
    const int64_t words = indexed_row_words(n_owners, m->N, s);
    if (words < 0) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": more than 2^31 - 1 edge rows in one call");
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    rc = chunks::ensure_memory(m, (size_t)n_owners);
    if (rc) return rc;
    rc = ensure_memory(m, (size_t)n, (size_t)n_owners, (size_t)words);
    if (rc) return rc;
    rc = chunks::upload_ints(m, ids.data(), 3 * (size_t)n_owners, O.ids.get());
    if (rc) return rc;
    chisel_hip_map::IndexedMemory &X = m->indexed_mem;
    const int pool = (int)X.owner_of_slot.size();
    const unsigned per_owner = (unsigned)((n_owners + 255) / 256);
    HIP_TRY(hipMemsetAsync(O.ctl.get(), 0, CK_INTS * sizeof(int), m->stream));
    HIP_TRY(hipMemsetAsync(X.owner_of_slot.get(), 0xff, (size_t)pool * sizeof(int), m->stream));
    HIP_TRY(hipMemsetAsync(X.masks.get(), 0, (size_t)words * sizeof(unsigned), m->stream));
    hipLaunchKernelGGL(chunks_classify_kernel, dim3(per_owner), dim3(256), 0, m->stream, m->view, (const int *)O.ids.get(), (int)n_owners, O.slots.get(), O.ctl.get());
    hipLaunchKernelGGL(indexed_owner_kernel, dim3(per_owner), dim3(256), 0, m->stream, (const int *)O.slots.get(), (int)n_owners, X.owner_of_slot.get(), pool);

    // ---- mark, rows, scan, the wait
    const dim3 grid((unsigned)coarse_grid(n)), owner_grid((unsigned)coarse_grid(n_owners));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(indexed_mark_kernel<N>, grid, dim3(COARSE_THREADS), 0, m->stream, m->view, (const int *)O.slots.get(), (int)n, s,
                                            (const int *)X.owner_of_slot.get(), pool, X.masks.get(), X.counts.get()));
    hipLaunchKernelGGL(indexed_rows_kernel, owner_grid, dim3(COARSE_THREADS), 0, m->stream, (const unsigned *)X.masks.get(), (int)n_owners, rows, X.prefix.get(), X.owner_counts.get());
    hipLaunchKernelGGL(indexed_scan_kernel, dim3(1), dim3(COARSE_THREADS), 0, m->stream, (const int *)O.slots.get(), (const int *)X.counts.get(), (int)n,
                       (const int *)X.owner_counts.get(), (int)n_owners, X.owner_first.get(), X.tri_first.get(), X.host.dev());
    volatile long long *words_h = X.host.get();
    rc = coarse::wait_for_totals(m, name, words_h, IX_ABSENT, listed);
    if (rc) return rc;
    volatile long long *owner_rows = words_h + INDEXED_HOST_WORDS + 2 * n;
    T.owners = 0;
    for (int64_t o = 0; o < n_owners; o++) T.owners += owner_rows[2 * o + 1] >= 0 ? 1 : 0;  // (an extra that is not resident is no owner; it has no vertex)
    T.cubes_meshed = words_h[IX_CUBES];
    T.vertices = words_h[IX_VERTICES];
    T.triangles = words_h[IX_TRIANGLES];
    if (const char *why = indexed_size_refusal(T.vertices, T.triangles)) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": " + why);
    if (!query) {
        if (const char *why = indexed_capacity_refusal(T.vertices, T.triangles, capacity_vertices, capacity_triangles)) {
            copy_totals(T, totals);  // (the caller can retry)
            return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
        }
        // ---- vertices, indices, shade
        if (T.vertices > 0 && vertices) {
            const size_t f3 = (size_t)T.vertices * 3 * sizeof(float), i3 = (size_t)T.triangles * 3 * sizeof(int32_t);
            float *dv = vertices, *dn = normals, *dc = colors;
            int32_t *di = indices;
            Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
            st.out(dv, f3);
            st.out(di, i3);
            st.out(dn, f3);
            st.out(dc, f3);
            HIP_TRY(st.begin());
            rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
            if (rc) return rc;
            const MeshParams P = mesh_params(m);
            FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(indexed_vertex_kernel<N>, owner_grid, dim3(COARSE_THREADS), 0, m->stream, m->view, P, (const int *)O.slots.get(), (int)n_owners, s,
                                                    (const unsigned *)X.masks.get(), (const unsigned *)X.prefix.get(), (const int *)X.owner_counts.get(),
                                                    (const long long *)X.owner_first.get(), dv));
            if (di && T.triangles > 0)
                FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(indexed_index_kernel<N>, grid, dim3(COARSE_THREADS), 0, m->stream, m->view, (const int *)O.slots.get(), (int)n, s,
                                                        (const int *)X.owner_of_slot.get(), pool, (const unsigned *)X.masks.get(), (const unsigned *)X.prefix.get(),
                                                        (const long long *)X.owner_first.get(), (const long long *)X.tri_first.get(), (const int *)X.counts.get(), di));
            hipError_t e = hipGetLastError();
            if (e == hipSuccess && dn) e = hipMemsetAsync(dn, 0, f3, m->stream);  // (zeros where the gradient look-up fails)
            rc = coarse::shade_and_finish(m, name, st, e, P, req->stages, T.vertices, dv, dn, dc);
            if (rc) return rc;
        }
    }
    // ---- what the host owns
    coarse::copy_rows(words_h + INDEXED_HOST_WORDS, n, chunk_table);
    int64_t at = 0;
    for (int64_t o = 0; o < n_owners; o++) {
        if (owner_rows[2 * o + 1] < 0) continue;
        if (owner_table) { owner_table[2 * at] = owner_rows[2 * o]; owner_table[2 * at + 1] = owner_rows[2 * o + 1]; }
        if (owner_ids_xyz) memcpy(owner_ids_xyz + 3 * at, ids.data() + 3 * o, 3 * sizeof(int));
        at++;
    }
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // namespace indexed
}  // namespace

extern "C" {

int chisel_hip_indexed_mesh(chisel_hip_map *m, const chisel_hip_coarse_request *req, int64_t capacity_vertices, int64_t capacity_triangles, float *vertices,
                            int32_t *indices, float *normals, float *colors, int on_device, int64_t *chunk_table, int64_t *owner_table, int *owner_ids_xyz,
                            chisel_hip_indexed_totals *totals) {
    SETTLE(m);
    return indexed::run(m, "chisel_hip_indexed_mesh", req, capacity_vertices, capacity_triangles, vertices, indices, normals, colors, on_device, chunk_table,
                        owner_table, owner_ids_xyz, totals);
}

}  // extern "C"

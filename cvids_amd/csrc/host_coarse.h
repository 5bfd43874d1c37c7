// host_coarse.h -- chisel_hip_coarse_mesh (included by chisel_hip.hip; the kernels: kernels_coarse.h; the stride rule, the request
// checks and the float arithmetic: coarse_checks.h; the definition: DESIGN.md 3.14).  A reader with chisel_hip_gather_chunks' frame
// (host_chunks.h), whose selection it takes: the map is only read; everything is queued on the map's stream behind what was queued
// before.  The entry reads top to bottom: refusals, the selection, the scratch, count and scan, THE WAIT for the totals (pinned
// memory), the capacity, then emit and shade -- with device pointers nothing is waited for behind them; host arrays are staged
// through one owned device buffer, copied out once each with exactly their live data, and are complete on return.
//
// Waits: a list of ids costs the one wait for the totals -- its slot look-up is queued in front of the count, and an id that is not
// resident is reported with the totals.  "Every resident chunk" and a box also wait for the listing of the resident chunks
// (chunks::select), which is sorted on the host, before the count can be queued: two waits.
//
// Scratch the map owns (chisel_hip_map::coarse_mem; the slot list: chunk_mem), grown on demand, freed with the map.
//
// The steps that chisel_hip_indexed_mesh (host_indexed.h) repeats are functions of this file, as host_rewrite.h's are for the
// entries that rewrite voxels: begin, wait_for_totals, shade_and_finish, copy_rows.  The pinned words are a PinnedWords
// (host_buffer.h), the totals leave through copy_totals (chisel_hip.hip), which the mesh gather uses too.
#pragma once

namespace {
namespace coarse {

struct Totals {
    int64_t chunks, chunks_nonempty, cubes_meshed, vertices;
};

// ---- the steps of the frame that the indexed mesh (host_indexed.h) takes as they are

// what both entries refuse behind their request checks (`query`: both capacities are 0), then the device and the recompute in flight
int begin(chisel_hip_map *m, const char *name, bool query, bool has_totals) {
    if (query && !has_totals) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": the size query without totals");
    HIP_TRY(hipSetDevice(m->device));
    return check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
}

// THE WAIT of a call, behind its scan kernel: `words` are complete; a listed id that is not resident is refused with its index
int wait_for_totals(chisel_hip_map *m, const char *name, volatile long long *words, int absent_word, bool listed) {
    if (int rc = wait_for_words(m)) return rc;
    if (listed && words[absent_word] >= 0)
        return fail(CHISEL_HIP_ERR_NOT_FOUND, chunks::with_index(name, (int64_t)words[absent_word], "chunk not resident (ChunkManager::GetChunk would throw std::out_of_range)"));
    return CHISEL_HIP_OK;
}

// The tail behind the entry's own kernels (`e`: what their launches said): zeros for colours without their stage, as the mesher
// leaves them, shade_vertices_kernel for the stages asked for, and the staged arrays' way out.
int shade_and_finish(chisel_hip_map *m, const char *name, Staging &st, hipError_t e, const MeshParams &P, int stages, int64_t n_vertices, const float *dv, float *dn, float *dc) {
    if (e == hipSuccess && dc && !(stages & 2)) e = hipMemsetAsync(dc, 0, (size_t)n_vertices * 3 * sizeof(float), m->stream);
    float *sn = (stages & 1) ? dn : nullptr, *sc = (stages & 2) ? dc : nullptr;
    if (e == hipSuccess && (sn || sc)) {
        const dim3 per_vertex((unsigned)((n_vertices + 255) / 256));
        FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(shade_vertices_kernel<N>, per_vertex, dim3(256), 0, m->stream, m->view, P, dv, (long long)n_vertices, sn, sc, stages));
        e = hipGetLastError();
    }
    e = st.finish(e);
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

// n rows of a pinned table (first, count) into the caller's, when it asked for it
inline void copy_rows(volatile const long long *rows, int64_t n, int64_t *out) {
    for (int64_t i = 0; out && i < 2 * n; i++) out[i] = rows[i];
}

// ---- the entry

// counts, firsts and the pinned words for a call of n chunks (doubled when they grow)
int ensure_memory(chisel_hip_map *m, size_t n) {
    chisel_hip_map::CoarseMemory &C = m->coarse_mem;
    const size_t want = std::max<size_t>(std::max<size_t>(n, 2 * C.first.size()), 1024);
    if (2 * n > C.counts.size() || n > C.first.size()) {
        int rc = grow_buffer(C.counts, 2 * want, m->stream);  // (waits for the stream before it replaces a buffer)
        if (rc) return rc;
        rc = grow_buffer(C.first, want, m->stream);
        if (rc) return rc;
    }
    HIP_TRY(C.host.ensure(COARSE_HOST_WORDS + 2 * n, m->stream));
    return CHISEL_HIP_OK;
}

int run(chisel_hip_map *m, const char *name, const chisel_hip_coarse_request *req, int64_t capacity_vertices, float *vertices, float *normals, float *colors,
        int on_device, int64_t *chunk_table, int *chunk_ids_xyz, chisel_hip_coarse_totals *totals) {
    // ---- refusals that need no device
    int rc = query_refusal(m, name, "takes the corners of a cube on a + face from the neighbour chunk");
    if (rc) return rc;
    int64_t bad_id = -1;
    if (const char *why = coarse_request_refusal(req, m->N, capacity_vertices, vertices, normals, colors, chunk_table, chunk_ids_xyz, m->cfg.use_color != 0, ID_BIAS - 2, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, chunks::with_index(name, bad_id, why));
    rc = begin(m, name, capacity_vertices == 0, totals != nullptr);
    if (rc) return rc;

    // ---- the selection: its slots into chunk_mem.slots
    const chisel_hip_chunk_request *sel = &req->chunks;
    const bool listed = sel->ids_xyz != nullptr;
    std::vector<int> ids, slots;
    int64_t n = 0;
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    if (listed) {  // (queued: the look-up's result is read with the totals)
        n = sel->n_ids;
        if (n > CHUNK_MAX_CHUNKS) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": more chunks than one call takes (2^31 - 1)");
        rc = chunks::ensure_memory(m, (size_t)n);
        if (rc) return rc;
        rc = chunks::upload_ints(m, sel->ids_xyz, 3 * (size_t)n, O.ids.get());
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(O.ctl.get(), 0, CK_INTS * sizeof(int), m->stream));
        hipLaunchKernelGGL(chunks_classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, m->view, (const int *)O.ids.get(), (int)n, O.slots.get(), O.ctl.get());
    } else {  // (the listing is sorted on the host: a wait of its own)
        bool table_ready = false;
        rc = chunks::select(m, name, sel, ids, slots, table_ready);
        if (rc) return rc;
        n = (int64_t)slots.size();
        if (n) {
            rc = chunks::ensure_memory(m, (size_t)n);
            if (rc) return rc;
            rc = chunks::upload_ints(m, slots.data(), (size_t)n, O.slots.get());
            if (rc) return rc;
        }
    }
    Totals T{n, 0, 0, 0};
    if (n == 0) {  // an empty map, a box without chunks: nothing is launched
        copy_totals(T, totals);
        return CHISEL_HIP_OK;
    }

    // ---- count, scan, the wait
    rc = ensure_memory(m, (size_t)n);
    if (rc) return rc;
    chisel_hip_map::CoarseMemory &C = m->coarse_mem;
    const int s = req->stride;
    const dim3 grid((unsigned)coarse_grid(n));
    FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(coarse_count_kernel<N>, grid, dim3(COARSE_THREADS), 0, m->stream, m->view, (const int *)O.slots.get(), (int)n, s, C.counts.get()));
    hipLaunchKernelGGL(coarse_scan_kernel, dim3(1), dim3(COARSE_THREADS), 0, m->stream, (const int *)O.slots.get(), (const int *)C.counts.get(), (int)n, C.first.get(), C.host.dev());
    volatile long long *words = C.host.get();
    rc = wait_for_totals(m, name, words, CO_ABSENT, listed);
    if (rc) return rc;
    T.chunks_nonempty = words[CO_NONEMPTY];
    T.cubes_meshed = words[CO_CUBES];
    T.vertices = words[CO_VERTICES];
    if (const char *why = coarse_floats_refusal(T.vertices)) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": " + why);
    if (capacity_vertices != 0) {
        if (const char *why = coarse_capacity_refusal(T.vertices, capacity_vertices)) {
            copy_totals(T, totals);  // (the caller can retry)
            return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
        }
        // ---- emit and shade
        if (T.vertices > 0 && vertices) {
            const size_t f3 = (size_t)T.vertices * 3 * sizeof(float);
            float *dv = vertices, *dn = normals, *dc = colors;
            Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
            st.out(dv, f3);
            st.out(dn, f3);
            st.out(dc, f3);
            HIP_TRY(st.begin());
            rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
            if (rc) return rc;
            const MeshParams P = mesh_params(m);
            FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(coarse_emit_kernel<N>, grid, dim3(COARSE_THREADS), 0, m->stream, m->view, P, (const int *)O.slots.get(), (int)n, s,
                                                    (const long long *)C.first.get(), (const int *)C.counts.get(), dv, dn));
            rc = shade_and_finish(m, name, st, hipGetLastError(), P, req->stages, T.vertices, dv, dn, dc);
            if (rc) return rc;
        }
    }
    // ---- what the host owns
    copy_rows(words + COARSE_HOST_WORDS, n, chunk_table);
    if (chunk_ids_xyz) memcpy(chunk_ids_xyz, listed ? sel->ids_xyz : ids.data(), (size_t)n * 3 * sizeof(int));
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // namespace coarse
}  // namespace

extern "C" {

int chisel_hip_coarse_mesh(chisel_hip_map *m, const chisel_hip_coarse_request *req, int64_t capacity_vertices, float *vertices, float *normals, float *colors,
                           int on_device, int64_t *chunk_table, int *chunk_ids_xyz, chisel_hip_coarse_totals *totals) {
    static_assert(sizeof(chisel_hip_coarse_request) == 56, "chisel_hip_coarse_request is 56 bytes");
    SETTLE(m);
    return coarse::run(m, "chisel_hip_coarse_mesh", req, capacity_vertices, vertices, normals, colors, on_device, chunk_table, chunk_ids_xyz, totals);
}

}  // extern "C"

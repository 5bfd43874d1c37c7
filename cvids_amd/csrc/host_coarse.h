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
#pragma once

namespace {
namespace coarse {

struct Totals {
    int64_t chunks, chunks_nonempty, cubes_meshed, vertices;
};

inline void copy_totals(const Totals &T, chisel_hip_coarse_totals *out) {
    static_assert(sizeof(chisel_hip_coarse_totals) == sizeof(Totals), "chisel_hip_coarse_totals and Totals are one layout");
    if (out) memcpy(out, &T, sizeof(T));
}

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
    if (COARSE_HOST_WORDS + 2 * n > C.host_words) {
        HIP_TRY(hipStreamSynchronize(m->stream));  // (a scan of an earlier call may still write the block that goes)
        C.host_words = 0;
        HIP_TRY(C.host.alloc(COARSE_HOST_WORDS + 2 * want));
        C.host_words = COARSE_HOST_WORDS + 2 * want;
    }
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
    if (capacity_vertices == 0 && !totals) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": the size query without totals");
    HIP_TRY(hipSetDevice(m->device));
    rc = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
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
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));  // the wait of a coarse mesh
    note_stream_idle(m);
    std::atomic_thread_fence(std::memory_order_acquire);
    volatile long long *words = C.host.get();
    if (listed && words[CO_ABSENT] >= 0)
        return fail(CHISEL_HIP_ERR_NOT_FOUND, chunks::with_index(name, (int64_t)words[CO_ABSENT], "chunk not resident (ChunkManager::GetChunk would throw std::out_of_range)"));
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
            hipError_t e = hipGetLastError();
            const int stages = req->stages;
            if (e == hipSuccess && dc && !(stages & 2)) e = hipMemsetAsync(dc, 0, f3, m->stream);  // (colours without their stage: zeros, as the mesher leaves them)
            float *sn = (stages & 1) ? dn : nullptr, *sc = (stages & 2) ? dc : nullptr;
            if (e == hipSuccess && (sn || sc)) {
                const dim3 per_vertex((unsigned)((T.vertices + 255) / 256));
                FOR_CHUNK_SIZE(m->N, hipLaunchKernelGGL(shade_vertices_kernel<N>, per_vertex, dim3(256), 0, m->stream, m->view, P, (const float *)dv, (long long)T.vertices, sn, sc, stages));
                e = hipGetLastError();
            }
            e = st.finish(e);
            if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
        }
    }
    // ---- what the host owns
    if (chunk_table)
        for (int64_t i = 0; i < 2 * n; i++) chunk_table[i] = words[COARSE_HOST_WORDS + i];
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

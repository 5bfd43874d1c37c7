// host_chunks.h -- chisel_hip_gather_chunks, chisel_hip_scatter_chunks, and chisel_hip_save_map / chisel_hip_load_map, which are fed by
// them in bounded blocks (included by chisel_hip.hip; the kernels: kernels_chunks.h; the request checks, the byte arithmetic and the
// "all" selection: chunk_checks.h; the definition: DESIGN.md 3.13).
//
// The gather is a reader with chisel_hip_query_points' frame (host_query.h): the map is only read; with device pointers the one
// launch goes on the map's stream behind whatever was queued before and nothing is waited for; host arrays are staged through one
// owned device buffer and are complete on return.  Its one wait is for the selection.  The scatter rewrites the map with the merge's
// frame (host_merge.h): classify, ONE wait for the absent count and the free slots, the pool sized -- a fixed pool that cannot take
// the absent ids refuses before anything is created --, create, copy, the slots' notes.  The per-call tables (ids, slots) are device
// scratch the map owns (chisel_hip_map::chunk_mem), grown on demand, freed with the map; they go up from pinned blocks that outlive
// the call (take_upload).
#pragma once

namespace {
namespace chunks {

constexpr int64_t FILE_BLOCK_BYTES = 64ll << 20;  // payload of one block of a save or a load

// what the entries refuse about the map: a group's chunks sit on several devices (one shard of several is served with its own)
int map_refusal(const chisel_hip_map *m, const char *name, bool null_argument, const char *what_null) {
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": a group's chunks sit on several devices (call a map of one shard)");
    if (!m || null_argument) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + what_null);
    return CHISEL_HIP_OK;
}

std::string with_index(const char *name, int64_t bad_id, const char *why) {
    return std::string(name) + ": " + (bad_id >= 0 ? "id " + std::to_string(bad_id) + " of the list: " : std::string()) + why;
}

// the map's scratch for a call of n chunks: ids and slots (doubled when they grow), the control words
int ensure_memory(chisel_hip_map *m, size_t n) {
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    if (!O.host) {
        HIP_TRY(O.host.alloc(CK_INTS));
        HIP_TRY(O.ctl.alloc(CK_INTS));
    }
    if (n <= O.slots.size() && 3 * n <= O.ids.size()) return CHISEL_HIP_OK;  // (both: one of them may have failed to grow before)
    const size_t want = std::max<size_t>(std::max<size_t>(n, 2 * O.slots.size()), 1024);
    int rc = grow_buffer(O.ids, 3 * want, m->stream);  // (waits for the stream before it replaces a buffer)
    if (rc) return rc;
    return grow_buffer(O.slots, want, m->stream);
}

// n ints from the host into a table of the map, through a pinned block that outlives the call
int upload_ints(chisel_hip_map *m, const int *src, size_t n, int *dst) {
    UploadBlock<int> *up = nullptr;
    int rc = take_upload(m->chunk_mem.uploads, n, &up);
    if (rc) return rc;
    memcpy(up->host.get(), src, n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(dst, up->host.get(), n * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipEventRecord(up->copied, m->stream));
    return CHISEL_HIP_OK;
}

// The selection of a gather, in its order: ids and slots on the host (the one wait of a gather).  table_ready: the slots are in
// chunk_mem.slots already (a list: the look-up left them there).
int select(chisel_hip_map *m, const char *name, const chisel_hip_chunk_request *req, std::vector<int> &ids, std::vector<int> &slots, bool &table_ready) {
    table_ready = false;
    if (!req->ids_xyz) {
        std::vector<int> all, all_slots;
        int rc = fetch_listed(m, false, all, &all_slots);
        if (rc) return rc;
        note_stream_idle(m);
        const std::vector<int64_t> order = chunk_select_sorted(all.data(), (int64_t)all_slots.size(), req->use_box != 0, req->box_lo, req->box_hi);
        ids.resize(order.size() * 3);
        slots.resize(order.size());
        for (size_t j = 0; j < order.size(); j++) {
            for (int a = 0; a < 3; a++) ids[3 * j + a] = all[3 * (size_t)order[j] + a];
            slots[j] = all_slots[(size_t)order[j]];
        }
        return CHISEL_HIP_OK;
    }
    const size_t n = (size_t)req->n_ids;
    if ((int64_t)n > CHUNK_MAX_CHUNKS) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": more chunks than one call takes (2^31 - 1)");
    int rc = ensure_memory(m, n);
    if (rc) return rc;
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    rc = upload_ints(m, req->ids_xyz, 3 * n, O.ids.get());
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(O.ctl.get(), 0, CK_INTS * sizeof(int), m->stream));
    hipLaunchKernelGGL(chunks_classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, m->view, (const int *)O.ids.get(), (int)n, O.slots.get(), O.ctl.get());
    HIP_TRY(hipGetLastError());
    slots.resize(n);
    HIP_TRY(hipMemcpyAsync(slots.data(), O.slots.get(), n * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    note_stream_idle(m);
    for (size_t i = 0; i < n; i++)
        if (slots[i] < 0)
            return fail(CHISEL_HIP_ERR_NOT_FOUND, with_index(name, (int64_t)i, "chunk not resident (ChunkManager::GetChunk would throw std::out_of_range)"));
    ids.assign(req->ids_xyz, req->ids_xyz + 3 * n);
    table_ready = true;
    return CHISEL_HIP_OK;
}

// the sizes of a packed set of n of the map's chunks, or the refusal
int sizes_of(const chisel_hip_map *m, const char *name, int64_t n, ChunkSizes &Z) {
    if (const char *why = chunk_sizes(n, (int64_t)m->V, &Z)) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": " + why);
    return CHISEL_HIP_OK;
}

// The copy out: n chunks, whose slots are `slots` in the selection's order (null: chunk_mem.slots holds them already), into the
// arrays that are given.
int copy_out(chisel_hip_map *m, const char *name, const int *slots, int64_t n, float *sdf, float *weight, uint8_t *rgbw, int on_device) {
    ChunkSizes Z;
    int rc = sizes_of(m, name, n, Z);
    if (rc) return rc;
    if (n == 0) return CHISEL_HIP_OK;
    rc = ensure_memory(m, (size_t)n);
    if (rc) return rc;
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    if (slots) {
        rc = upload_ints(m, slots, (size_t)n, O.slots.get());
        if (rc) return rc;
    }
    Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
    st.out(sdf, (size_t)Z.bytes_per_array);
    st.out(weight, (size_t)Z.bytes_per_array);
    st.out(rgbw, (size_t)Z.bytes_per_array);
    HIP_TRY(st.begin());
    rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
    if (rc) return rc;
    ChunkCopyArrays A{};
    unsigned arrays = 0;
    if (sdf) { A.pool[arrays] = m->view.sdf; A.packed[arrays++] = sdf; }
    if (weight) { A.pool[arrays] = m->view.wgt; A.packed[arrays++] = weight; }
    if (rgbw) { A.pool[arrays] = m->view.rgbw; A.packed[arrays++] = rgbw; }
    hipLaunchKernelGGL(chunk_copy_kernel<false>, dim3((unsigned)Z.tiles, arrays), dim3(CHUNK_COPY_THREADS), 0, m->stream, A, (const int *)O.slots.get(), (long long)n, Z.quad_shift);
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    return CHISEL_HIP_OK;
}

int gather(chisel_hip_map *m, const char *name, const chisel_hip_chunk_request *req, int64_t capacity_chunks, float *sdf, float *weight, uint8_t *rgbw,
           int on_device, int *chunk_ids_xyz, int64_t *n_chunks) {
    // ---- refusals that need no device
    int rc = map_refusal(m, name, !req, "null map or request");
    if (rc) return rc;
    int64_t bad_id = -1;
    if (const char *why = chunk_gather_refusal(req, capacity_chunks, sdf, weight, rgbw, chunk_ids_xyz, on_device != 0, m->cfg.use_color != 0, ID_BIAS - 2, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, with_index(name, bad_id, why));
    if (capacity_chunks == 0 && !n_chunks) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": the size query without n_chunks");
    // ---- the selection (the one wait)
    HIP_TRY(hipSetDevice(m->device));
    rc = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
    if (rc) return rc;
    std::vector<int> ids, slots;
    bool table_ready = false;
    rc = select(m, name, req, ids, slots, table_ready);
    if (rc) return rc;
    const int64_t n = (int64_t)slots.size();
    if (capacity_chunks == 0) {  // the size query
        *n_chunks = n;
        return CHISEL_HIP_OK;
    }
    if (const char *why = chunk_capacity_refusal(n, capacity_chunks)) {
        if (n_chunks) *n_chunks = n;  // (the caller can retry)
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    }
    // ---- the launch
    if (sdf || weight || rgbw) {
        rc = copy_out(m, name, table_ready ? nullptr : slots.data(), n, sdf, weight, rgbw, on_device);
        if (rc) return rc;
    }
    // ---- what the host owns
    if (chunk_ids_xyz && n) memcpy(chunk_ids_xyz, ids.data(), (size_t)n * 3 * sizeof(int));
    if (n_chunks) *n_chunks = n;
    return CHISEL_HIP_OK;
}

// headroom: a growable pool also keeps a quarter free for the integration that follows, as a merge leaves it (chisel_hip_load_map, which
// has made room for its whole file before the first block, passes false: a load commits what it committed before, never more)
int scatter(chisel_hip_map *m, const char *name, const int *ids_xyz, int64_t n, const float *sdf, const float *weight, const uint8_t *rgbw, int on_device,
            int mark_updated, int64_t *n_created, bool headroom = true) {
    // ---- refusals: the map is not touched by a refused call
    int rc = map_refusal(m, name, false, "null map");
    if (rc) return rc;
    if (const char *why = chunk_scatter_refusal(ids_xyz, n, sdf, weight, rgbw, on_device != 0, m->cfg.use_color != 0))
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    if (n_created) *n_created = 0;
    if (n == 0) return CHISEL_HIP_OK;
    ChunkSizes Z;
    rc = sizes_of(m, name, n, Z);
    if (rc) return rc;
    int64_t bad_id = -1;
    const chisel_hip_config &cfg = m->cfg;
    if (const char *why = chunk_scatter_ids_refusal(ids_xyz, n, ID_BIAS - 2, [&](int x, int y, int z) { return chunk_owner(x, y, z, cfg.n_shards, cfg.shard_block); }, cfg.shard_rank, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, with_index(name, bad_id, why));
    HIP_TRY(hipSetDevice(m->device));
    { m->topology_epoch++; m->dirty_tail_queued = false; }  // (where chisel_hip_upload_chunk does)
    rc = check_mesh_totals(m);  // a recompute in flight reads the voxels as they are
    if (rc) return rc;

    // ---- ids up, classify, the one wait
    rc = ensure_memory(m, (size_t)n);
    if (rc) return rc;
    chisel_hip_map::ChunkMemory &O = m->chunk_mem;
    rc = upload_ints(m, ids_xyz, 3 * (size_t)n, O.ids.get());
    if (rc) return rc;
    const dim3 per_chunk((unsigned)((n + 255) / 256));
    HIP_TRY(hipMemsetAsync(O.ctl.get(), 0, CK_INTS * sizeof(int), m->stream));
    hipLaunchKernelGGL(chunks_classify_kernel, per_chunk, dim3(256), 0, m->stream, m->view, (const int *)O.ids.get(), (int)n, O.slots.get(), O.ctl.get());
    hipLaunchKernelGGL(report_words_kernel<int>, dim3(1), dim3(1), 0, m->stream, (const int *)O.ctl.get(), O.host.dev(), CK_INTS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));  // the one wait of a scatter
    note_stream_idle(m);
    std::atomic_thread_fence(std::memory_order_acquire);
    volatile int *words = O.host.get();
    const int64_t n_absent = words[CK_ABSENT], n_free = words[CK_FREE];

    // ---- the pool: decided before the first chunk is created (as a merge decides it)
    if (n_absent > n_free) {
        const int64_t want = (int64_t)m->view.committed + (n_absent - n_free);
        if (!m->growable || want > m->view.max_chunks)
            return fail(CHISEL_HIP_ERR_POOL_FULL, std::string(name) + ": the chunk pool cannot take the chunks the call would create: raise chisel_hip_config.max_chunks");
    }
    if (m->growable && n_absent > 0) {  // (and a quarter of the pool free afterwards, for the integration that follows)
        const int64_t used_after = (int64_t)m->view.committed - n_free + n_absent;
        if (n_absent > n_free || (headroom && (int64_t)m->view.committed - used_after < (int64_t)m->view.committed / 4)) {
            const int before = m->view.committed;
            rc = grow_pool(m, headroom ? std::max<int64_t>(2 * (int64_t)m->view.committed, used_after + used_after / 2) : used_after);
            if (rc) return rc;
            if ((int64_t)(m->view.committed - before) + n_free < n_absent) return fail(CHISEL_HIP_ERR_POOL_FULL, std::string(name) + ": the chunk pool is at its limit");
        }
    }

    // ---- create, copy, the slots' notes
    if (n_absent > 0) hipLaunchKernelGGL(chunks_create_kernel, per_chunk, dim3(256), 0, m->stream, (const MapView *)m->view_dev.get(), (const int *)O.ids.get(), (int)n, O.slots.get());
    Staging st(m->stream, on_device != 0);
    st.in(sdf, (size_t)Z.bytes_per_array);
    st.in(weight, (size_t)Z.bytes_per_array);
    st.in(rgbw, (size_t)Z.bytes_per_array);
    HIP_TRY(st.begin());
    rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the payload is ready behind it
    if (rc) return rc;
    ChunkCopyArrays A{};
    unsigned arrays = 0;
    A.pool[arrays] = m->view.sdf; A.packed[arrays++] = const_cast<float *>(sdf);
    A.pool[arrays] = m->view.wgt; A.packed[arrays++] = const_cast<float *>(weight);
    if (m->view.rgbw) { A.pool[arrays] = m->view.rgbw; A.packed[arrays++] = const_cast<uint8_t *>(rgbw); }  // (null: zeros)
    hipLaunchKernelGGL(chunk_copy_kernel<true>, dim3((unsigned)Z.tiles, arrays), dim3(CHUNK_COPY_THREADS), 0, m->stream, A, (const int *)O.slots.get(), (long long)n, Z.quad_shift);
    hipLaunchKernelGGL(chunks_note_kernel, per_chunk, dim3(256), 0, m->stream, m->view, (const int *)O.slots.get(), (int)n, mark_updated);
    const hipError_t e = st.finish(hipGetLastError());
    if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    if (mark_updated) m->mesh_mark_needed = true;  // the 27-neighbourhoods join the job list at the next recompute (mesh_mark_kernel)
    HIP_TRY(note_map_mutation(m));
    if (n_created) *n_created = n_absent;
    return CHISEL_HIP_OK;
}

// chunks per block of a save or a load: 64 MiB of payload, or what CHISEL_HIP_MAP_BLOCK_CHUNKS says (test hook, read at call time)
int64_t file_block_chunks(const chisel_hip_map *m) {
    if (const char *e = getenv("CHISEL_HIP_MAP_BLOCK_CHUNKS")) {
        const long long v = atoll(e);
        if (v > 0) return (int64_t)v;
    }
    return chunk_block_chunks((int64_t)m->V, m->view.rgbw != nullptr, FILE_BLOCK_BYTES);
}

// the pinned arrays one block of a save or a load passes through
struct FileBlock {
    PinnedBuffer<float> sdf, wgt;
    PinnedBuffer<uint8_t> col;
    hipError_t alloc(size_t chunks, size_t V, bool color) {
        hipError_t e = sdf.alloc(chunks * V);
        if (e == hipSuccess) e = wgt.alloc(chunks * V);
        if (e == hipSuccess && color) e = col.alloc(chunks * V * 4);
        return e;
    }
};

}  // namespace chunks
}  // namespace

extern "C" {

int chisel_hip_gather_chunks(chisel_hip_map *m, const chisel_hip_chunk_request *req, int64_t capacity_chunks, float *sdf, float *weight, uint8_t *rgbw,
                             int on_device, int *chunk_ids_xyz, int64_t *n_chunks) {
    static_assert(sizeof(chisel_hip_chunk_request) == 48, "chisel_hip_chunk_request is 48 bytes");
    SETTLE(m);
    return chunks::gather(m, "chisel_hip_gather_chunks", req, capacity_chunks, sdf, weight, rgbw, on_device, chunk_ids_xyz, n_chunks);
}

int chisel_hip_scatter_chunks(chisel_hip_map *m, const int *ids_xyz, int64_t n, const float *sdf, const float *weight, const uint8_t *rgbw, int on_device,
                              int mark_updated, int64_t *n_created) {
    SETTLE(m);
    return chunks::scatter(m, "chisel_hip_scatter_chunks", ids_xyz, n, sdf, weight, rgbw, on_device, mark_updated, n_created);
}

// the file: chisel_hip.h.  Records ascending by id, fed by gathers of bounded blocks through pinned memory.
int chisel_hip_save_map(chisel_hip_map *m, const char *path) {
    const char *name = "chisel_hip_save_map";
    SETTLE(m);
    if (m && m->is_group) return group::save_map(m, path);
    if (!m || !path) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    int rc = check_device_error(m);  // waits for the queued batches
    if (rc) return rc;
    std::vector<int> ids, slots;
    bool table_ready = false;
    const chisel_hip_chunk_request all{};
    rc = chunks::select(m, name, &all, ids, slots, table_ready);
    if (rc) return rc;
    const size_t n = slots.size();
    std::ofstream out(path, std::ios::binary);
    if (!out) return fail(CHISEL_HIP_ERR_IO, std::string("cannot open ") + path);
    MapFileHeader h;
    memcpy(h.magic, "CHSLHIP1", 8);
    h.chunk_edge = m->N;
    h.resolution = m->cfg.voxel_resolution;
    h.has_color = m->view.rgbw ? 1 : 0;
    h.spare = 0;
    h.n_chunks = (int64_t)n;
    out.write(reinterpret_cast<const char *>(&h), sizeof(h));
    const size_t V = (size_t)m->V;
    const size_t block = (size_t)std::min<int64_t>(chunks::file_block_chunks(m), (int64_t)std::max<size_t>(n, 1));
    chunks::FileBlock B;
    if (n) HIP_TRY(B.alloc(block, V, h.has_color != 0));
    for (size_t first = 0; first < n; first += block) {
        const size_t cnt = std::min(block, n - first);
        rc = chunks::copy_out(m, name, slots.data() + first, (int64_t)cnt, B.sdf.get(), B.wgt.get(), h.has_color ? B.col.get() : nullptr, 0);
        if (rc) return rc;
        for (size_t i = 0; i < cnt; i++) {
            out.write(reinterpret_cast<const char *>(&ids[3 * (first + i)]), 3 * sizeof(int));
            out.write(reinterpret_cast<const char *>(B.sdf.get() + i * V), (std::streamsize)(V * sizeof(float)));
            out.write(reinterpret_cast<const char *>(B.wgt.get() + i * V), (std::streamsize)(V * sizeof(float)));
            if (h.has_color) out.write(reinterpret_cast<const char *>(B.col.get() + i * 4 * V), (std::streamsize)(4 * V));
        }
    }
    out.flush();
    if (!out) return fail(CHISEL_HIP_ERR_IO, std::string("write failed: ") + path);
    return CHISEL_HIP_OK;
}

// The accepted records go to the map block by block (chunks::scatter).  A record that ends the load -- a truncated one, an id out of
// range -- leaves the map holding the records in front of it.
int chisel_hip_load_map(chisel_hip_map *m, const char *path) {
    const char *name = "chisel_hip_load_map";
    if (m && m->is_group) return group::for_all(m, [&](chisel_hip_map *s) { return chisel_hip_load_map(s, path); });  // every shard takes the chunks it owns
    if (!m || !path) return fail(CHISEL_HIP_ERR_INVALID, "null argument");
    std::ifstream in(path, std::ios::binary);
    if (!in) return fail(CHISEL_HIP_ERR_IO, std::string("cannot open ") + path);
    MapFileHeader h;
    in.read(reinterpret_cast<char *>(&h), sizeof(h));
    if (!in || memcmp(h.magic, "CHSLHIP1", 8) != 0) return fail(CHISEL_HIP_ERR_IO, "not a chisel-hip map file");
    if (h.chunk_edge != m->N || h.resolution != m->cfg.voxel_resolution || (h.has_color != 0) != (m->view.rgbw != nullptr))
        return fail(CHISEL_HIP_ERR_INVALID, "map file was written with another chunk size, resolution or colour setting");
    if (h.n_chunks < 0 || h.n_chunks > m->view.max_chunks) return fail(CHISEL_HIP_ERR_POOL_FULL, "map file holds more chunks than max_chunks");
    int rc = chisel_hip_reset(m);
    if (rc) return rc;
    rc = ensure_free_exact(m, h.n_chunks);  // (a growable pool: room for the file's chunks)
    if (rc) return rc;
    const size_t V = (size_t)m->V;
    const size_t block = (size_t)std::min<int64_t>(chunks::file_block_chunks(m), std::max<int64_t>(h.n_chunks, 1));
    chunks::FileBlock B;
    if (h.n_chunks) HIP_TRY(B.alloc(block, V, h.has_color != 0));
    std::vector<int> ids;
    std::unordered_set<uint64_t, IdHash> in_block;  // (a file that repeats an id: the later record wins, as it did chunk by chunk)
    auto flush = [&]() {
        const int64_t cnt = (int64_t)ids.size() / 3;
        if (cnt == 0) return (int)CHISEL_HIP_OK;
        SETTLE(m);
        const int rc_s = chunks::scatter(m, name, ids.data(), cnt, B.sdf.get(), B.wgt.get(), h.has_color ? B.col.get() : nullptr, 0, 0, nullptr, false);
        ids.clear();
        in_block.clear();
        return rc_s;
    };
    for (int64_t i = 0; i < h.n_chunks; i++) {
        const size_t at = ids.size() / 3;
        int id[3];
        in.read(reinterpret_cast<char *>(id), sizeof(id));
        in.read(reinterpret_cast<char *>(B.sdf.get() + at * V), (std::streamsize)(V * sizeof(float)));
        in.read(reinterpret_cast<char *>(B.wgt.get() + at * V), (std::streamsize)(V * sizeof(float)));
        if (h.has_color) in.read(reinterpret_cast<char *>(B.col.get() + at * 4 * V), (std::streamsize)(4 * V));
        if (!in) {
            rc = flush();
            return rc ? rc : fail(CHISEL_HIP_ERR_IO, std::string("truncated map file: ") + path);
        }
        if (!chunk_id_in_range(id)) {
            rc = flush();
            return rc ? rc : fail(CHISEL_HIP_ERR_INVALID, std::string("map file names a ") + kIdOutOfRange);
        }
        if (chunk_owner(id[0], id[1], id[2], m->cfg.n_shards, m->cfg.shard_block) != m->cfg.shard_rank) continue;  // another shard's chunk
        if (!in_block.insert(pack_id(id[0], id[1], id[2])).second) {
            // the record sits behind the block's last one: flush what is in front of it, then move it to the block's start
            std::vector<float> s(B.sdf.get() + at * V, B.sdf.get() + (at + 1) * V), w(B.wgt.get() + at * V, B.wgt.get() + (at + 1) * V);
            std::vector<uint8_t> c;
            if (h.has_color) c.assign(B.col.get() + at * 4 * V, B.col.get() + (at + 1) * 4 * V);
            rc = flush();
            if (rc) return rc;
            memcpy(B.sdf.get(), s.data(), V * sizeof(float));
            memcpy(B.wgt.get(), w.data(), V * sizeof(float));
            if (h.has_color) memcpy(B.col.get(), c.data(), 4 * V);
            in_block.insert(pack_id(id[0], id[1], id[2]));
        }
        ids.insert(ids.end(), id, id + 3);
        if (ids.size() / 3 == block) {
            rc = flush();
            if (rc) return rc;
        }
    }
    return flush();
}

}  // extern "C"

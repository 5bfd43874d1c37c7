// host_gather.h -- chisel_hip_gather_meshes, _gather_meshes_size and chisel_hip_save_ply_binary (included by chisel_hip.hip; the kernel:
// kernels_gather.h; the request check and the segment table: gather_checks.h; the definition: DESIGN.md 3.12).  The frame is
// chisel_hip_query_points' own (host_query.h): the map is only read; with device pointers the one launch goes on the map's stream
// behind whatever was queued before and nothing is waited for; host arrays are staged through one owned device buffer and are
// complete on return.  The entries read top to bottom: refusals, the selection (the one wait: resolve_pending_meshes), the plan,
// scratch and table, the launch, the host-side bookkeeping.
//
// Arena lifetime needs nothing new: the kernel reads arenas on the map's stream.  An arena whose last mesh is replaced afterwards goes
// to arena_pool (free_arena) and is rewritten only by a later recompute, which is queued on the same stream behind this launch
// (take_arena_buffer hands out pooled buffers to recompute_meshes alone); the pool's overflow and the map's end release with hipFree,
// which waits for the device.
#pragma once

namespace {
namespace gather {

// what the entries refuse about the map: a group's meshes sit on several devices (one shard of several is served: its meshes are its own)
int map_refusal(const chisel_hip_map *m, const char *name, bool null_argument) {
    if (m && m->is_group) return fail(CHISEL_HIP_ERR_UNSUPPORTED, std::string(name) + ": a group's meshes sit on several devices (gather from a map of one shard)");
    if (!m || null_argument) return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": null map or request");
    return CHISEL_HIP_OK;
}

// the selection as the map's bookkeeping has it (after resolve_pending_meshes); NOT_FOUND names the index of an id without a mesh
int select(chisel_hip_map *m, const char *name, const chisel_hip_mesh_request *req, std::vector<GatherSource> &src, std::vector<uint64_t> &keys) {
    if (!req->ids_xyz) {
        keys = sorted_mesh_keys(m);
    } else {
        keys.resize((size_t)req->n_ids);
        for (int64_t i = 0; i < req->n_ids; i++) keys[(size_t)i] = pack_id(req->ids_xyz[3 * i], req->ids_xyz[3 * i + 1], req->ids_xyz[3 * i + 2]);
    }
    src.resize(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        auto it = m->meshes.find(keys[i]);
        if (it == m->meshes.end())
            return fail(CHISEL_HIP_ERR_NOT_FOUND, std::string(name) + ": id " + std::to_string(i) + " of the list has no mesh (ChunkManager::GetMesh would throw std::out_of_range)");
        const MeshRef &r = it->second;
        GatherSource &s = src[i];
        s = GatherSource{r.arena, (int64_t)r.v_off, (int64_t)r.n_v, (int64_t)r.g_off, (int64_t)r.n_g, 0, false};
        if (r.arena >= 0) {
            s.arena_nv = (int64_t)m->arenas[r.arena].nv;
            s.arena_color = m->arenas[r.arena].color;
        }
    }
    return CHISEL_HIP_OK;
}

int run(chisel_hip_map *m, const char *name, const chisel_hip_mesh_request *req, int64_t capacity_vertices, int64_t capacity_grids, float *const outputs[GATHER_ARRAYS],
        int on_device, int64_t *mesh_table, int *mesh_ids_xyz, chisel_hip_mesh_totals *totals) {
    // ---- refusals that need no device
    int rc = map_refusal(m, name, !req);
    if (rc) return rc;
    GatherOutputs want;
    for (int a = 0; a < GATHER_ARRAYS; a++) want.want[a] = outputs[a] != nullptr;
    int64_t bad_id = -1;
    if (const char *why = gather_request_refusal(req, true, want, m->cfg.use_color != 0, ID_BIAS - 2, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + (bad_id >= 0 ? "id " + std::to_string(bad_id) + ": " : std::string()) + why);
    // ---- the selection and its plan
    HIP_TRY(hipSetDevice(m->device));
    rc = resolve_pending_meshes(m);  // the one wait: the job records of a recompute still in flight
    if (rc) return rc;
    std::vector<GatherSource> src;
    std::vector<uint64_t> keys;
    rc = select(m, name, req, src, keys);
    if (rc) return rc;
    GatherPlan plan;
    int code = 0;
    if (const char *why = gather_plan(src.data(), (int64_t)src.size(), want, true, true, capacity_vertices, capacity_grids, &plan, &code)) {
        if (code == GATHER_REFUSED_INVALID) copy_totals(plan.totals, totals);  // (the capacity: the caller can retry)
        return fail(code == GATHER_REFUSED_UNSUPPORTED ? CHISEL_HIP_ERR_UNSUPPORTED : CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    }
    const GatherTotals &T = plan.totals;
    const size_t n_segs = plan.segments.size();
    if (n_segs) {
        // ---- scratch, staging, the table
        chisel_hip_map::GatherMemory &O = m->gather_mem;
        rc = grow_buffer(O.table, n_segs, m->stream);
        if (rc) return rc;
        UploadBlock<GatherSeg> *up = nullptr;
        rc = take_upload(O.uploads, n_segs, &up);
        if (rc) return rc;
        float *dev[GATHER_ARRAYS];
        for (int a = 0; a < GATHER_ARRAYS; a++) dev[a] = outputs[a];
        const size_t bytes[GATHER_ARRAYS] = {(size_t)T.vertices * 12, (size_t)T.vertices * 12, (size_t)T.vertices * 12, (size_t)T.vertices * 16, (size_t)T.grids * 12};
        Staging st(m->stream, on_device != 0);  // (device outputs are left on the map's stream: nothing is waited for)
        for (int a = 0; a < GATHER_ARRAYS; a++) st.out(dev[a], bytes[a]);  // (each array goes out in one copy of exactly its live data)
        HIP_TRY(st.begin());
        rc = wait_for_input(m, m->stream);  // chisel_hip_wait_event / _order_map_after_stream: the outputs may be written behind it
        if (rc) return rc;
        GatherSeg *S = up->host.get();
        for (size_t i = 0; i < n_segs; i++) {
            const GatherSegment &g = plan.segments[i];
            S[i] = GatherSeg{m->arenas[g.arena].dev + g.src, dev[g.array] + g.dst, (long long)g.start, g.len, g.kind};
        }
        HIP_TRY(hipMemcpyAsync(O.table.get(), S, n_segs * sizeof(GatherSeg), hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipEventRecord(up->copied, m->stream));
        // ---- the launch: one workgroup per tile of the concatenated outputs
        GatherLights L{};
        if (req->marker_colors) {
            for (int a = 0; a < 3; a++) {
                L.l0[a] = req->light0[a];
                L.l1[a] = req->light1[a];
            }
            L.diffuse = req->diffuse;
            L.ambient = req->ambient;
        }
        const dim3 grid((unsigned)T.tiles);  // (<= 5 (2^31 - 1) / 4096)
        hipLaunchKernelGGL(gather_meshes_kernel, grid, dim3(GATHER_THREADS), 0, m->stream, (const GatherSeg *)O.table.get(), (int)n_segs, (long long)plan.floats, L);
        const hipError_t e = st.finish(hipGetLastError());
        if (e != hipSuccess) return fail(CHISEL_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    }
    // ---- the bookkeeping the host owns
    if (mesh_table && !plan.table.empty()) memcpy(mesh_table, plan.table.data(), plan.table.size() * sizeof(int64_t));
    if (mesh_ids_xyz)
        for (size_t i = 0; i < keys.size(); i++) unpack_id(keys[i], mesh_ids_xyz[3 * i], mesh_ids_xyz[3 * i + 1], mesh_ids_xyz[3 * i + 2]);
    copy_totals(T, totals);
    return CHISEL_HIP_OK;
}

}  // namespace gather
}  // namespace

extern "C" {

int chisel_hip_gather_meshes(chisel_hip_map *m, const chisel_hip_mesh_request *req, int64_t capacity_vertices, int64_t capacity_grids, float *vertices,
                             float *normals, float *colors, float *rgba, float *grids, int on_device, int64_t *mesh_table, int *mesh_ids_xyz,
                             chisel_hip_mesh_totals *totals) {
    SETTLE(m);
    float *const outputs[GATHER_ARRAYS] = {vertices, normals, colors, rgba, grids};
    return gather::run(m, "chisel_hip_gather_meshes", req, capacity_vertices, capacity_grids, outputs, on_device, mesh_table, mesh_ids_xyz, totals);
}

int chisel_hip_gather_meshes_size(chisel_hip_map *m, const chisel_hip_mesh_request *req, chisel_hip_mesh_totals *totals) {
    const char *name = "chisel_hip_gather_meshes_size";
    SETTLE(m);
    int rc = gather::map_refusal(m, name, !req || !totals);
    if (rc) return rc;
    GatherOutputs could{{true, true, m->cfg.use_color != 0, req->marker_colors != 0, true}};
    int64_t bad_id = -1;
    if (const char *why = gather_request_refusal(req, false, could, m->cfg.use_color != 0, ID_BIAS - 2, &bad_id))
        return fail(CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + (bad_id >= 0 ? "id " + std::to_string(bad_id) + ": " : std::string()) + why);
    HIP_TRY(hipSetDevice(m->device));
    rc = resolve_pending_meshes(m);
    if (rc) return rc;
    std::vector<GatherSource> src;
    std::vector<uint64_t> keys;
    rc = gather::select(m, name, req, src, keys);
    if (rc) return rc;
    GatherPlan plan;
    int code = 0;
    if (const char *why = gather_plan(src.data(), (int64_t)src.size(), could, false, false, 0, 0, &plan, &code))
        return fail(code == GATHER_REFUSED_UNSUPPORTED ? CHISEL_HIP_ERR_UNSUPPORTED : CHISEL_HIP_ERR_INVALID, std::string(name) + ": " + why);
    copy_totals(plan.totals, totals);
    return CHISEL_HIP_OK;
}

// write_ply's header and records (host_mesh.h) in binary: x y z as float, the colours as uchar, a face as uchar 3 + three int
int chisel_hip_save_ply_binary(chisel_hip_map *m, const char *path) {
    const char *name = "chisel_hip_save_ply_binary";
    SETTLE(m);
    int rc = gather::map_refusal(m, name, !path);
    if (rc) return rc;
    std::ofstream stream(path, std::ios::binary);
    if (!stream) return fail(CHISEL_HIP_ERR_IO, std::string("cannot open ") + path);
    chisel_hip_mesh_request req{};
    chisel_hip_mesh_totals T{};
    rc = chisel_hip_gather_meshes_size(m, &req, &T);
    if (rc) return rc;
    const bool any_color = m->cfg.use_color != 0 && T.vertices > 0;
    std::vector<float> v((size_t)T.vertices * 3), c(any_color ? (size_t)T.vertices * 3 : 0);
    if (T.vertices) {  // (nothing has changed the map since the size call: one host-side gather)
        float *const outputs[GATHER_ARRAYS] = {v.data(), nullptr, any_color ? c.data() : nullptr, nullptr, nullptr};
        rc = gather::run(m, name, &req, T.vertices, 0, outputs, 0, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    const size_t numPoints = (size_t)T.vertices;
    stream << "ply\n" << "format binary_little_endian 1.0\n" << "element vertex " << numPoints << "\n";
    stream << "property float x\nproperty float y\nproperty float z\n";
    if (any_color) stream << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    stream << "element face " << numPoints / 3 << "\n" << "property list uchar int vertex_index\n" << "end_header\n";
    std::vector<char> rec;
    const size_t vb = any_color ? 15 : 12;
    rec.resize(numPoints * vb + (numPoints / 3) * 13);
    char *p = rec.data();
    for (size_t i = 0; i < numPoints; i++) {
        memcpy(p, &v[3 * i], 12);
        p += 12;
        if (any_color)
            for (int k = 0; k < 3; k++) *p++ = (char)(unsigned char)static_cast<int>(c[3 * i + k] * 255.0f);  // (write_ply's conversion)
    }
    for (size_t f = 0; f < numPoints / 3; f++) {
        *p++ = 3;
        const int32_t idx[3] = {(int32_t)(3 * f), (int32_t)(3 * f + 1), (int32_t)(3 * f + 2)};
        memcpy(p, idx, 12);
        p += 12;
    }
    stream.write(rec.data(), (std::streamsize)rec.size());
    stream.close();
    if (!stream) return fail(CHISEL_HIP_ERR_IO, std::string("write failed: ") + path);
    return CHISEL_HIP_OK;
}

}  // extern "C"

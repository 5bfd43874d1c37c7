// facade_gather.cpp -- chisel::ChunkManager::GatherMeshes and chisel::Chisel::SaveAllMeshesToPLYBinary on a map built from three frames
// (facade_smoke.cpp's wall, depth only): the markers of ChiselServer::PublishMeshes filled from ONE gather are checked equal, float for
// float, to the per-mesh walk over GetAllMeshes(); the marker colours against FillMarkerTopicWithMeshes' own arithmetic with
// ChiselServer's lights.  tests/test_gpu_mesh_gather.py runs it.
#include <open_chisel/Chisel.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace chisel;

static bool same_floats(const float *a, const Vec3 &b) {
    const float v[3] = {b(0), b(1), b(2)};
    return memcmp(a, v, sizeof(v)) == 0;
}

int main(int argc, char **argv) {
    const int W = 64, H = 48, N = 8;
    const float res = 0.05f;
    try {
        Chisel map(Eigen::Vector3i(N, N, N), res, false);
        TruncatorPtr trunc(new InverseTruncator(2.0f));
        WeighterPtr weigh(new ConstantWeighter(1.0f));
        ProjectionIntegrator integ(trunc, weigh, 0.05f, true, map.GetChunkManager().GetCentroids());
        PinholeCamera cam;
        Intrinsics K;
        K.SetFx(52.5f); K.SetFy(52.5f); K.SetCx(31.5f); K.SetCy(23.5f);
        cam.SetIntrinsics(K);
        cam.SetWidth(W); cam.SetHeight(H);
        cam.SetNearPlane(0.05f); cam.SetFarPlane(5.0f);
        std::shared_ptr<DepthImage<float>> depth(new DepthImage<float>(W, H));
        for (int k = 0; k < 3; k++) {
            // a wall at z = 1.5 + 0.1 k metres, tilted a little so that the normals vary; camera at the origin looking along +z
            for (int v = 0; v < H; v++)
                for (int u = 0; u < W; u++) depth->SetDataAt(v, u, 1.5f + 0.1f * k + 0.004f * u - 0.003f * v);
            Transform T;  // identity
            map.IntegrateDepthScan<float>(integ, depth, T, cam);
        }
        for (int k = 0; k < 10; k++) map.UpdateMeshes();  // (the recompute runs on every 10th call, Chisel.cpp:53-58)
        const ChunkManager &cm = map.GetChunkManager();
        // the per-mesh walk (ChiselServer.cpp:613-716) ...
        const MeshMap &meshMap = cm.GetAllMeshes();
        // ... and one gather
        const ChunkManager::MarkerLights lights;
        const ChunkManager::PackedMeshes P = cm.GatherMeshes(ChunkIDList(), true, true, true, lights);
        if ((size_t)P.totals.meshes != meshMap.size() || P.totals.meshes < 4 || P.totals.vertices < 300) return 2;
        size_t vertices = 0, grids = 0;
        for (int64_t i = 0; i < P.totals.meshes; i++) {
            const ChunkID id(P.ids[3 * i], P.ids[3 * i + 1], P.ids[3 * i + 2]);
            const MeshPtr &mesh = meshMap.at(id);
            const int64_t *row = &P.table[4 * i];
            if (mesh->vertices.empty() && mesh->grids.empty()) {
                if (row[0] || row[1] || row[2] || row[3]) return 3;
                continue;
            }
            if ((size_t)row[1] != mesh->vertices.size() || (size_t)row[3] != mesh->grids.size() || (size_t)row[0] != vertices || (size_t)row[2] != grids) return 3;
            for (size_t k = 0; k < mesh->vertices.size(); k++) {
                const size_t at = (size_t)row[0] + k;
                if (!same_floats(&P.vertices[3 * at], mesh->vertices[k]) || !same_floats(&P.normals[3 * at], mesh->normals[k])) return 4;
                // FillMarkerTopicWithMeshes' colour of a vertex with a normal (ChiselServer.cpp:690-700), operation by operation
                const Vec3 &n = mesh->normals[k];
                const float d0 = (n(0) * lights.light0(0) + n(1) * lights.light0(1)) + n(2) * lights.light0(2);
                const float d1 = (n(0) * lights.light1(0) + n(1) * lights.light1(1)) + n(2) * lights.light1(2);
                const float s0 = fmaxf(d0, 0.0f) * lights.diffuse, s1 = fmaxf(d1, 0.0f) * lights.diffuse;
                const float c = fminf((s0 + s1) + lights.ambient, 1.0f);
                const float want[4] = {c, c, c, 1.0f};
                if (memcmp(&P.rgba[4 * at], want, sizeof(want)) != 0) return 5;
            }
            for (size_t k = 0; k < mesh->grids.size(); k++)
                if (!same_floats(&P.grids[3 * ((size_t)row[2] + k)], mesh->grids[k])) return 6;
            vertices += mesh->vertices.size();
            grids += mesh->grids.size();
        }
        if (vertices != (size_t)P.totals.vertices || grids != (size_t)P.totals.grids || P.vertices.size() != 3 * vertices || P.rgba.size() != 4 * vertices) return 7;
        printf("gather: %lld meshes, %zu vertices, %zu grids, %lld arenas, %lld tiles\n", (long long)P.totals.meshes, vertices, grids,
               (long long)P.totals.arenas_read, (long long)P.totals.tiles);
        // a selection in the caller's order, vertices alone; an id without a mesh throws as GetMesh does
        ChunkIDList two;
        two.push_back(ChunkID(P.ids[3], P.ids[4], P.ids[5]));
        two.push_back(ChunkID(P.ids[0], P.ids[1], P.ids[2]));
        const ChunkManager::PackedMeshes Q = cm.GatherMeshes(two, false, false, false);
        if (Q.totals.meshes != 2 || Q.table[1] != P.table[5] || Q.table[5] != P.table[1] || !Q.normals.empty() || !Q.grids.empty()) return 8;
        if (Q.table[1] && memcmp(Q.vertices.data(), &P.vertices[3 * (size_t)P.table[4]], (size_t)Q.table[1] * 12) != 0) return 8;
        bool threw = false;
        try {
            ChunkIDList none;
            none.push_back(ChunkID(1000, 1000, 1000));
            cm.GatherMeshes(none);
        } catch (const std::out_of_range &) {
            threw = true;
        }
        if (!threw) return 9;
        if (argc > 1 && !map.SaveAllMeshesToPLYBinary(argv[1])) return 10;
        if (map.SaveAllMeshesToPLYBinary("/no/such/directory/x.ply")) return 11;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_gather: %s\n", e.what());
        return 1;
    }
    printf("facade_gather ok\n");
    return 0;
}

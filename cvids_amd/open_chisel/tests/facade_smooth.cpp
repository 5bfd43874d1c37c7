// facade_smooth.cpp -- chisel::ChunkManager::SmoothMesh and chisel::Chisel::SaveSmoothMeshToPLY on a map built from three frames
// (facade_indexed.cpp's wall, with colour): the indexed mesh of every chunk after 0, 10, 3 and 5 iterations of Taubin smoothing at two
// strides, with and without the open rim pinned.  A smoothed mesh has its input's indices and colours and one unit normal per vertex
// with a triangle of some area; no iteration is the identity; negative iterations throw.  Counts and a checksum per array are printed
// for tests/test_gpu_mesh_adjacency.py, which builds the same map through the Python mirror and compares.
#include <open_chisel/Chisel.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace chisel;

// sum of (index + 1) x word over the list's 32-bit words (x, y, z of every entry in turn), modulo 2^64
static unsigned long long checksum(const Vec3List &list) {
    unsigned long long s = 0;
    size_t i = 0;
    for (const Vec3 &v : list)
        for (int k = 0; k < 3; k++) {
            const float f = v(k);
            uint32_t w;
            memcpy(&w, &f, 4);
            s += (unsigned long long)(++i) * w;
        }
    return s;
}

int main(int argc, char **argv) {
    const int W = 64, H = 48, N = 8;
    const float res = 0.05f;
    try {
        Chisel map(Eigen::Vector3i(N, N, N), res, true);
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
        std::shared_ptr<ColorImage<uint8_t>> color(new ColorImage<uint8_t>(W, H, 3));
        for (int v = 0; v < H; v++)
            for (int u = 0; u < W; u++)
                for (int c = 0; c < 3; c++) color->GetMutableData()[(v * W + u) * 3 + c] = (uint8_t)((7 * u + 13 * v + 50 * c) & 255);
        for (int k = 0; k < 3; k++) {
            for (int v = 0; v < H; v++)
                for (int u = 0; u < W; u++) depth->SetDataAt(v, u, 1.5f + 0.25f * k + 0.0078125f * u - 0.00390625f * v);  // (every term exact in binary)
            Transform T;  // identity
            map.IntegrateDepthScanColor<float, uint8_t>(integ, depth, T, cam, color, T, cam);
        }
        const ChunkManager &cm = map.GetChunkManager();
        const struct { int stride, iterations, pin; } runs[] = {{1, 0, 3}, {1, 10, 3}, {2, 3, 0}, {2, 5, 3}};
        for (const auto &r : runs) {
            Mesh whole, mesh;
            cm.GenerateIndexedMesh(r.stride, &whole);
            mesh.grids.push_back(Vec3(1.0f, 2.0f, 3.0f));  // (a mesh that held something: it is cleared)
            chisel_hip_adjacency_totals totals{};
            cm.SmoothMesh(whole, r.iterations, 0.5f, -0.53f, r.pin, &mesh, &totals);
            const size_t n = mesh.vertices.size(), t3 = mesh.indices.size();
            if (n != whole.vertices.size() || mesh.indices != whole.indices || mesh.normals.size() != n || mesh.colors.size() != n || !mesh.grids.empty()) return 2;
            if ((int64_t)n != totals.vertices || (int64_t)t3 != 3 * totals.triangles || totals.invalid_triangles != 0 || totals.isolated_vertices != 0) return 3;
            if (totals.max_incident > CHISEL_HIP_MESH_MAX_INCIDENT || totals.nonmanifold_vertices != 0 || totals.boundary_vertices == 0) return 4;
            if (checksum(mesh.colors) != checksum(whole.colors)) return 5;
            if ((checksum(mesh.vertices) == checksum(whole.vertices)) != (r.iterations == 0)) return 6;
            size_t moved = 0;
            for (size_t i = 0; i < n; i++) moved += (mesh.vertices[i] - whole.vertices[i]).norm() > 0.0f ? 1 : 0;
            if (r.iterations && (moved == 0 || (int64_t)moved > totals.vertices - totals.pinned_vertices)) return 7;
            unsigned long long sx = 0;
            for (size_t i = 0; i < t3; i++) sx += (unsigned long long)(i + 1) * (uint32_t)mesh.indices[i];
            printf("stride%d_iterations%d_pin%d %lld %lld %lld %lld %lld %lld %llx %llx %llx %llx\n", r.stride, r.iterations, r.pin, (long long)totals.vertices,
                   (long long)totals.triangles, (long long)totals.incidences, (long long)totals.neighbors, (long long)totals.boundary_vertices,
                   (long long)totals.pinned_vertices, checksum(mesh.vertices), checksum(mesh.normals), checksum(mesh.colors), sx);
            cm.SmoothMesh(mesh, 0, 0.5f, -0.53f, r.pin, &mesh);  // in place, no iteration: the same mesh
            if (mesh.vertices.size() != n || mesh.indices != whole.indices) return 8;
        }
        bool threw = false;
        try {
            Mesh whole, mesh;
            cm.GenerateIndexedMesh(2, &whole);
            cm.SmoothMesh(whole, -1, 0.5f, -0.53f, 3, &mesh);
        } catch (const std::exception &) {
            threw = true;
        }
        if (!threw) return 9;
        if (argc > 1 && !map.SaveSmoothMeshToPLY(argv[1], 2, 5, 16)) return 10;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_smooth: %s\n", e.what());
        return 1;
    }
    printf("facade_smooth ok\n");
    return 0;
}

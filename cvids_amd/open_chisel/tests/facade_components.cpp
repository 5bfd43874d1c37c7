// facade_components.cpp -- chisel::ChunkManager::FilterMesh and chisel::Chisel::SaveCleanMeshToPLY on a map built from three frames
// (facade_indexed.cpp's wall, with colour): the indexed mesh of every chunk without its small connected components, at two strides,
// thresholds of 1, 16 and 64 triangles and the largest component alone.  A filtered mesh names only its own vertices, every vertex is
// referenced, and filtering it again changes nothing; a threshold below 1 throws.  Counts and a checksum per array are printed for
// tests/test_gpu_mesh_components.py, which builds the same map through the Python mirror and compares.
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
        const struct { int stride; int64_t minTriangles; bool largest; } runs[] = {{1, 1, false}, {1, 64, false}, {2, 16, false}, {2, 1, true}};
        for (const auto &r : runs) {
            Mesh whole, mesh, again;
            cm.GenerateIndexedMesh(r.stride, &whole);
            mesh.grids.push_back(Vec3(1.0f, 2.0f, 3.0f));  // (a mesh that held something: it is cleared)
            chisel_hip_components_totals totals{}, second{};
            cm.FilterMesh(whole, r.minTriangles, r.largest, &mesh, &totals);
            const size_t n = mesh.vertices.size(), t3 = mesh.indices.size();
            if (t3 % 3 != 0 || mesh.normals.size() != n || mesh.colors.size() != n || !mesh.grids.empty()) return 2;
            if ((int64_t)n != totals.kept_vertices || (int64_t)t3 != 3 * totals.kept_triangles || totals.invalid_triangles != 0) return 3;
            if (n > whole.vertices.size() || t3 > whole.indices.size() || totals.vertices != (int64_t)whole.vertices.size()) return 4;
            std::vector<char> referenced(n, 0);
            unsigned long long sx = 0;
            for (size_t i = 0; i < t3; i++) {
                if (mesh.indices[i] >= n) return 5;
                referenced[mesh.indices[i]] = 1;
                sx += (unsigned long long)(i + 1) * (uint32_t)mesh.indices[i];
            }
            for (size_t i = 0; i < n; i++)
                if (!referenced[i]) return 6;
            if (r.largest && !(totals.kept_components == 1 && totals.kept_triangles == totals.largest_triangles)) return 7;
            cm.FilterMesh(mesh, r.minTriangles, r.largest, &again, &second);  // idempotent
            if (again.vertices.size() != n || again.indices != mesh.indices || checksum(again.vertices) != checksum(mesh.vertices) ||
                checksum(again.colors) != checksum(mesh.colors) || second.components != totals.kept_components)
                return 8;
            printf("stride%d_min%lld_largest%d %lld %lld %lld %lld %lld %llx %llx %llx %llx\n", r.stride, (long long)r.minTriangles, r.largest ? 1 : 0,
                   (long long)totals.components, (long long)totals.largest_triangles, (long long)totals.kept_components, (long long)totals.kept_vertices,
                   (long long)totals.kept_triangles, checksum(mesh.vertices), checksum(mesh.normals), checksum(mesh.colors), sx);
        }
        bool threw = false;
        try {
            Mesh whole, mesh;
            cm.GenerateIndexedMesh(2, &whole);
            cm.FilterMesh(whole, 0, false, &mesh);
        } catch (const std::exception &) {
            threw = true;
        }
        if (!threw) return 9;
        if (argc > 1 && !map.SaveCleanMeshToPLY(argv[1], 2, 16)) return 10;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_components: %s\n", e.what());
        return 1;
    }
    printf("facade_components ok\n");
    return 0;
}

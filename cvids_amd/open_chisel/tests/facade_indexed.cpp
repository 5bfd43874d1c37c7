// facade_indexed.cpp -- chisel::ChunkManager::GenerateIndexedMesh and chisel::Chisel::SaveIndexedMeshToPLY on a map built from three
// frames (facade_coarse.cpp's wall, with colour): the indexed mesh of every chunk at strides 1, 2, 4 and 8.  At every stride the
// triangles are GenerateCoarseMesh's (three times as many soup vertices), every index is below the vertex count and every vertex is
// referenced; a stride that does not divide the chunk size throws.  Counts and a checksum per array are printed for
// tests/test_gpu_indexed_mesh.py, which builds the same map through the Python mirror and compares.
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
        for (int stride = 1; stride <= N; stride *= 2) {
            Mesh mesh, soup;
            mesh.grids.push_back(Vec3(1.0f, 2.0f, 3.0f));  // (a mesh that held something: it is cleared)
            cm.GenerateIndexedMesh(stride, &mesh);
            cm.GenerateCoarseMesh(stride, &soup);
            const size_t n = mesh.vertices.size(), t3 = mesh.indices.size();
            if (t3 % 3 != 0 || mesh.normals.size() != n || mesh.colors.size() != n || !mesh.grids.empty()) return 2;
            if (t3 != soup.vertices.size()) return 3;
            std::vector<char> referenced(n, 0);
            unsigned long long sx = 0;
            for (size_t i = 0; i < t3; i++) {
                if (mesh.indices[i] >= n) return 4;
                referenced[mesh.indices[i]] = 1;
                sx += (unsigned long long)(i + 1) * (uint32_t)mesh.indices[i];
            }
            for (size_t i = 0; i < n; i++)
                if (!referenced[i]) return 5;
            if (stride == 1 && !(n > 0 && 2 * n < t3)) return 6;  // (far fewer vertices than the soup's)
            printf("stride%d %zu %zu %llx %llx %llx %llx\n", stride, n, t3 / 3, checksum(mesh.vertices), checksum(mesh.normals), checksum(mesh.colors), sx);
        }
        bool threw = false;
        try {
            Mesh mesh;
            cm.GenerateIndexedMesh(3, &mesh);
        } catch (const std::exception &) {
            threw = true;
        }
        if (!threw) return 7;
        if (argc > 1 && !map.SaveIndexedMeshToPLY(argv[1], 2)) return 8;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_indexed: %s\n", e.what());
        return 1;
    }
    printf("facade_indexed ok\n");
    return 0;
}

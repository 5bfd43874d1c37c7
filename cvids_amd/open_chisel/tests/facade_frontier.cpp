// facade_frontier.cpp -- chisel::Chisel::Frontiers on a map built from three frames (facade_distance.cpp's wall, depth only): prints
// the totals and an FNV-1a checksum of label, voxels and table, which tests/test_gpu_frontier.py compares with the Python host path's
// on the same frames.
#include <open_chisel/Chisel.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace chisel;

static unsigned long long fnv1a(const void *data, size_t bytes) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

int main() {
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
            // a wall at z = 1.5 + 0.1 k metres, camera at the origin looking along +z
            for (int v = 0; v < H; v++)
                for (int u = 0; u < W; u++) depth->SetDataAt(v, u, 1.5f + 0.1f * k);
            Transform T;  // identity
            map.IntegrateDepthScan<float>(integ, depth, T, cam);
        }
        std::vector<uint8_t> state;
        std::vector<int32_t> label, voxels;
        std::vector<int64_t> table;
        std::vector<double> centres;
        const Eigen::Vector3i origin(-12, -10, 22), dims(24, 20, 18);
        const chisel_hip_frontier_totals t = map.Frontiers(origin, dims, 1, 26, 2, 0.0f, &state, &label, &voxels, &table, &centres);
        if (state.size() != (size_t)24 * 20 * 18 || label.size() != state.size()) return 2;
        if (voxels.size() != (size_t)t.kept_voxels * 4 || table.size() != (size_t)t.kept_clusters * 12 || centres.size() != (size_t)t.kept_clusters * 3) return 3;
        if (t.unknown + t.free + t.occupied != (int64_t)state.size() || !t.unknown || !t.free || !t.frontier || !t.kept_clusters) return 4;
        printf("totals unknown %lld free %lld occupied %lld frontier %lld clusters %lld largest %lld kept_clusters %lld kept_voxels %lld\n", (long long)t.unknown,
               (long long)t.free, (long long)t.occupied, (long long)t.frontier, (long long)t.clusters, (long long)t.largest_voxels, (long long)t.kept_clusters,
               (long long)t.kept_voxels);
        printf("checksum label %016llx voxels %016llx table %016llx\n", fnv1a(label.data(), label.size() * sizeof(int32_t)),
               fnv1a(voxels.data(), voxels.size() * sizeof(int32_t)), fnv1a(table.data(), table.size() * sizeof(int64_t)));
        printf("centre0 %.17g %.17g %.17g\n", centres[0], centres[1], centres[2]);
        // the state is DistanceField's; a refusal throws as the other calls do and the map answers afterwards
        std::vector<uint8_t> field;
        map.DistanceField(origin, dims, 1, false, 0.0f, &field, nullptr, nullptr);
        if (field != state) return 5;
        bool threw = false;
        try {
            map.Frontiers(origin, dims, 7, 26, 1, 0.0f, nullptr, &label, nullptr, nullptr);
        } catch (const std::exception &) {
            threw = true;
        }
        std::vector<int32_t> again;
        map.Frontiers(origin, dims, 1, 26, 2, 0.0f, nullptr, &again, nullptr, nullptr);
        if (!threw || again != label) return 6;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_frontier: %s\n", e.what());
        return 1;
    }
    printf("facade_frontier ok\n");
    return 0;
}

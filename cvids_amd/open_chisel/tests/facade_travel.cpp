// facade_travel.cpp -- chisel::Chisel::TravelField and TravelPath on a map built from three frames (facade_distance.cpp's wall, depth
// only), the kept frontier voxels of the window as targets: prints the totals (without the implementation's diagnostics) and an FNV-1a
// checksum of cost, step, the group table and the path from the costliest voxel, which tests/test_gpu_travel.py compares with the
// Python host path's on the same frames.
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
        const Eigen::Vector3i origin(-12, -10, 2), dims(24, 20, 38), costs(10, 14, 17);
        const size_t n = (size_t)24 * 20 * 38;
        std::vector<int32_t> voxels;
        std::vector<int64_t> clusters;
        const chisel_hip_frontier_totals f = map.Frontiers(origin, dims, 1, 26, 2, 0.0f, nullptr, nullptr, &voxels, &clusters);
        // the seed: the first voxel of the central column (x = 12, y = 10) that is traversable at clearance 1 -- the frames leave the
        // voxels near the camera unobserved
        std::vector<uint8_t> seen;
        std::vector<int32_t> dist2;
        map.DistanceField(origin, dims, 1, false, 0.0f, &seen, &dist2, nullptr);
        int seed_z = -1;
        for (int z = 0; z < 38 && seed_z < 0; z++)
            if (seen[((size_t)z * 20 + 10) * 24 + 12] == 1 && dist2[((size_t)z * 20 + 10) * 24 + 12] == -1) seed_z = z;
        if (seed_z < 0) return 8;
        const std::vector<int32_t> seeds = {12, 10, seed_z};
        std::vector<int32_t> cost;
        std::vector<uint8_t> step, state;
        std::vector<int64_t> table;
        const chisel_hip_travel_totals t =
            map.TravelField(origin, dims, seeds, 26, costs, 1 << 30, 1, false, 0.0f, &cost, &step, &state, &voxels, f.kept_clusters, &table);
        if (cost.size() != n || step.size() != n || state.size() != n || table.size() != (size_t)f.kept_clusters * 4) return 2;
        if (t.unknown + t.free + t.occupied != (int64_t)n || t.seeds_used != 1 || t.reached < 2 || !f.kept_clusters) return 3;
        printf("seed 12 10 %d\n", seed_z);
        printf("totals unknown %lld free %lld occupied %lld traversable %lld seeds_used %lld seeds_ignored %lld reached %lld largest_cost %lld "
               "targets_reached %lld targets_ignored %lld\n",
               (long long)t.unknown, (long long)t.free, (long long)t.occupied, (long long)t.traversable, (long long)t.seeds_used, (long long)t.seeds_ignored,
               (long long)t.reached, (long long)t.largest_cost, (long long)t.targets_reached, (long long)t.targets_ignored);
        size_t far = 0;  // the first voxel of the largest cost
        for (size_t i = 0; i < n; i++)
            if (cost[i] > cost[far]) far = i;
        if ((int64_t)cost[far] != t.largest_cost) return 4;
        const Eigen::Vector3i start((int)(far % 24), (int)((far / 24) % 20), (int)(far / (24 * 20)));
        const std::vector<int32_t> path = Chisel::TravelPath(step, dims, start);
        if (path.size() < 6 || path[path.size() - 3] != 12 || path[path.size() - 2] != 10 || path[path.size() - 1] != seed_z) return 5;
        printf("checksum cost %016llx step %016llx table %016llx path %016llx\n", fnv1a(cost.data(), cost.size() * sizeof(int32_t)), fnv1a(step.data(), step.size()),
               fnv1a(table.data(), table.size() * sizeof(int64_t)), fnv1a(path.data(), path.size() * sizeof(int32_t)));
        // the state is DistanceField's; a refusal throws as the other calls do and the map answers afterwards
        std::vector<uint8_t> field;
        map.DistanceField(origin, dims, 1, false, 0.0f, &field, nullptr, nullptr);
        if (field != state) return 6;
        bool threw = false;
        try {
            map.TravelField(origin, dims, seeds, 7, costs, 1 << 30, 0, false, 0.0f, &cost, nullptr);
        } catch (const std::exception &) {
            threw = true;
        }
        bool threw_path = false;
        try {
            Chisel::TravelPath(step, dims, Eigen::Vector3i(24, 0, 0));
        } catch (const std::exception &) {
            threw_path = true;
        }
        std::vector<int32_t> again;
        map.TravelField(origin, dims, seeds, 26, costs, 1 << 30, 1, false, 0.0f, &again, nullptr);
        if (!threw || !threw_path || again != cost) return 7;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_travel: %s\n", e.what());
        return 1;
    }
    printf("facade_travel ok\n");
    return 0;
}

// facade_distance.cpp -- chisel::Chisel::DistanceField on a map built from three frames (facade_smoke.cpp's wall, depth only): prints
// the window's reach and an FNV-1a checksum of each output, which tests/test_gpu_distance.py compares with the Python host path's on
// the same frames.
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
        std::vector<int32_t> dist2;
        std::vector<float> distance;
        const Eigen::Vector3i origin(-12, -10, 22), dims(24, 20, 18);
        map.DistanceField(origin, dims, 6, false, 0.0f, &state, &dist2, &distance);
        size_t n_state[3] = {0, 0, 0}, none = 0;
        for (uint8_t s : state) n_state[s < 3 ? s : 0]++;
        for (int32_t d : dist2) none += d < 0;
        if (state.size() != (size_t)24 * 20 * 18 || dist2.size() != state.size() || distance.size() != state.size()) return 2;
        if (!n_state[0] || !n_state[1] || !n_state[2] || !none || none == dist2.size()) return 3;
        printf("window %zu voxels: unknown %zu free %zu occupied %zu without an obstacle %zu\n", state.size(), n_state[0], n_state[1], n_state[2], none);
        printf("checksum state %016llx dist2 %016llx distance %016llx\n", fnv1a(state.data(), state.size()), fnv1a(dist2.data(), dist2.size() * sizeof(int32_t)),
               fnv1a(distance.data(), distance.size() * sizeof(float)));
        // state alone, and a refusal: the call throws as the other calls do and the map answers afterwards
        std::vector<uint8_t> alone;
        map.DistanceField(origin, dims, 6, true, 0.0f, &alone, nullptr, nullptr);
        if (alone != state) return 4;
        bool threw = false;
        try {
            map.DistanceField(origin, dims, 65, false, 0.0f, &alone, nullptr, nullptr);
        } catch (const std::exception &) {
            threw = true;
        }
        map.DistanceField(origin, dims, 1, false, 0.0f, &alone, nullptr, nullptr);
        if (!threw || alone != state) return 5;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_distance: %s\n", e.what());
        return 1;
    }
    printf("facade_distance ok\n");
    return 0;
}

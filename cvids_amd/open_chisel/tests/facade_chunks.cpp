// facade_chunks.cpp -- chisel::ChunkManager::GatherChunks and ScatterChunks on a map built from three frames (facade_gather.cpp's wall,
// with colour): the packed set of one gather is checked equal, voxel for voxel, to the walk over GetChunks(); it is scattered into
// a second chisel::Chisel, whose own gather must give it back; an absent id throws std::out_of_range as GetChunk does.  The ids and a
// checksum per array are printed for tests/test_gpu_chunks.py, which builds the same map through the Python mirror and compares.
#include <open_chisel/Chisel.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace chisel;

// sum of (index + 1) x word over the array's 32-bit words, modulo 2^64
static unsigned long long checksum(const void *data, size_t bytes) {
    const uint32_t *w = static_cast<const uint32_t *>(data);
    unsigned long long s = 0;
    for (size_t i = 0; i < bytes / 4; i++) s += (unsigned long long)(i + 1) * w[i];
    return s;
}

int main() {
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
        const size_t V = (size_t)N * N * N;
        // the per-chunk walk ...
        const ChunkMap &chunks = cm.GetChunks();
        // ... and one gather
        const ChunkManager::PackedChunks P = cm.GatherChunks();
        const size_t n = P.ids.size() / 3;
        if (n != chunks.size() || n < 8 || P.sdf.size() != n * V || P.weight.size() != n * V || P.rgbw.size() != 4 * n * V) return 2;
        for (size_t i = 0; i < n; i++) {
            const ChunkID id(P.ids[3 * i], P.ids[3 * i + 1], P.ids[3 * i + 2]);
            if (i && !(P.ids[3 * i - 3] < id(0) || (P.ids[3 * i - 3] == id(0) && (P.ids[3 * i - 2] < id(1) || (P.ids[3 * i - 2] == id(1) && P.ids[3 * i - 1] < id(2)))))) return 3;
            const ChunkPtr &chunk = chunks.at(id);
            const std::vector<DistVoxel> &dv = chunk->GetVoxels();
            const std::vector<ColorVoxel> &cv = chunk->GetColorVoxels();
            for (size_t k = 0; k < V; k++) {
                if (memcmp(&dv[k].sdf, &P.sdf[i * V + k], 4) != 0 || memcmp(&dv[k].weight, &P.weight[i * V + k], 4) != 0) return 4;
                const uint8_t *c = &P.rgbw[4 * (i * V + k)];
                if (cv[k].red != c[0] || cv[k].green != c[1] || cv[k].blue != c[2] || cv[k].weight != c[3]) return 5;
            }
        }
        printf("ids");
        for (size_t i = 0; i < 3 * n; i++) printf(" %d", P.ids[i]);
        printf("\nsdf %llx\nweight %llx\nrgbw %llx\n", checksum(P.sdf.data(), P.sdf.size() * 4), checksum(P.weight.data(), P.weight.size() * 4),
               checksum(P.rgbw.data(), P.rgbw.size()));
        // a selection in the caller's order, with a duplicate
        ChunkIDList three;
        three.push_back(ChunkID(P.ids[3], P.ids[4], P.ids[5]));
        three.push_back(ChunkID(P.ids[0], P.ids[1], P.ids[2]));
        three.push_back(ChunkID(P.ids[3], P.ids[4], P.ids[5]));
        const ChunkManager::PackedChunks Q = cm.GatherChunks(three);
        if (Q.ids.size() != 9 || memcmp(Q.sdf.data(), &P.sdf[V], V * 4) != 0 || memcmp(&Q.sdf[V], P.sdf.data(), V * 4) != 0 || memcmp(&Q.sdf[2 * V], &P.sdf[V], V * 4) != 0 ||
            memcmp(&Q.rgbw[4 * V], P.rgbw.data(), 4 * V) != 0)
            return 6;
        // into a second map, and back out of it
        Chisel other(Eigen::Vector3i(N, N, N), res, true);
        ChunkManager &om = other.GetMutableChunkManager();
        if (om.ScatterChunks(P) != (int64_t)n || om.GetChunks().size() != n) return 7;
        const ChunkManager::PackedChunks R = om.GatherChunks();
        if (R.ids != P.ids || memcmp(R.sdf.data(), P.sdf.data(), P.sdf.size() * 4) != 0 || memcmp(R.weight.data(), P.weight.data(), P.weight.size() * 4) != 0 || R.rgbw != P.rgbw) return 8;
        if (!other.GetMeshesToUpdate().empty()) return 9;
        if (om.ScatterChunks(ChunkManager::PackedChunks()) != 0) return 9;  // an empty set: a no-op
        // marked as updated, the chunks and their neighbours are due for meshing
        ChunkManager::PackedChunks one;
        one.ids.assign(P.ids.begin(), P.ids.begin() + 3);
        one.sdf.assign(P.sdf.begin(), P.sdf.begin() + V);
        one.weight.assign(P.weight.begin(), P.weight.begin() + V);
        if (om.ScatterChunks(one, true) != 0 || other.GetMeshesToUpdate().size() != 27) return 10;
        bool threw = false;
        try {
            ChunkIDList none;
            none.push_back(ChunkID(P.ids[0], P.ids[1], P.ids[2]));
            none.push_back(ChunkID(1000, 1000, 1000));
            cm.GatherChunks(none);
        } catch (const std::out_of_range &) {
            threw = true;
        }
        if (!threw) return 11;
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_chunks: %s\n", e.what());
        return 1;
    }
    printf("facade_chunks ok\n");
    return 0;
}

// Stand-alone check of cvids_amd/csrc/host_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_host_checks.py: the planes the list kernel rejects chunks by must keep every chunk that holds a voxel the per-voxel
// rule can select (a voxel that projects onto the image in front of the camera, in the kernel's own fp32 arithmetic), for ordinary
// and for hostile cameras and poses; and the refusals -- the image check the alignment entries share with de-integration, and
// de-integration's own -- must say no to what the header says they refuse.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_checks.h"

using namespace chisel_hip;

static unsigned long long g_state = 88172645463325252ull;
static double uniform() {  // xorshift64
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

// the per-voxel projection as kernels_deintegrate.h: deintegrate_select does it
static bool on_image(const float pose[12], float fx, float fy, float cx, float cy, int W, int H, float px, float py, float pz) {
    const float dx = px - pose[3], dy = py - pose[7], dz = pz - pose[11];
    const float qx = pose[0] * dx + (pose[4] * dy + pose[8] * dz);
    const float qy = pose[1] * dx + (pose[5] * dy + pose[9] * dz);
    const float qz = pose[2] * dx + (pose[6] * dy + pose[10] * dz);
    const float iq = 1.0f / qz;
    const float u = fx * qx * iq + cx, v = fy * qy * iq + cy;
    return (u >= 0.0f) && (v >= 0.0f) && (u < (float)W) && (v < (float)H) && !(qz < 0.0f);
}

int main() {
    struct Camera { float fx, fy, cx, cy; int W, H; };
    const Camera cameras[] = {{525.f, 525.f, 319.5f, 239.5f, 640, 480}, {30.f, 70.f, 19.2f, 38.4f, 64, 48}, {52.5f, 52.5f, -25.6f, 62.4f, 64, 48},
                              {9.f, 11.f, 31.75f, 23.f, 64, 48}, {400.f, 390.f, 31.5f, 23.5f, 64, 48}, {-40.f, 40.f, 30.f, 20.f, 64, 48},
                              {3.3f, 3.3f, 0.9f, 53.6f, 3, 67}, {1.f, 1.f, 0.5f, 0.5f, 1, 1}};
    long kept = 0, dropped = 0, voxels = 0;
    for (const Camera &K : cameras)
        for (int trial = 0; trial < 40; trial++) {
            // a rotation from three angles, now and then scaled or sheared (the entry asks only for finite entries); translations out to 2 km
            const double a = 6.3 * uniform(), b = 6.3 * uniform(), c = 6.3 * uniform(), far = trial % 4 == 3 ? 2000.0 : 3.0;
            const double Rz[9] = {cos(a), -sin(a), 0, sin(a), cos(a), 0, 0, 0, 1}, Ry[9] = {cos(b), 0, sin(b), 0, 1, 0, -sin(b), 0, cos(b)},
                         Rx[9] = {1, 0, 0, 0, cos(c), -sin(c), 0, sin(c), cos(c)};
            double T[9], R[9];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) T[3 * i + j] = Rz[3 * i] * Ry[j] + Rz[3 * i + 1] * Ry[3 + j] + Rz[3 * i + 2] * Ry[6 + j];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[3 * i + j] = T[3 * i] * Rx[j] + T[3 * i + 1] * Rx[3 + j] + T[3 * i + 2] * Rx[6 + j];
            if (trial % 5 == 4) for (int i = 0; i < 9; i++) R[i] *= 1.7;
            if (trial % 7 == 6) R[1] += 0.4;
            float pose[12];
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) pose[4 * i + j] = (float)R[3 * i + j];
                pose[4 * i + 3] = (float)(far * (2.0 * uniform() - 1.0));
            }
            for (int N = 8; N <= 32; N *= 2) {
                const float res = N == 8 ? 0.05f : 0.02f, half = res * 0.5f;
                DeintegratePyramid Y;
                deintegrate_pyramid(pose, K.fx, K.fy, K.cx, K.cy, K.W, K.H, N, res, Y);
                const int base[3] = {(int)floor(pose[3] / Y.edge), (int)floor(pose[7] / Y.edge), (int)floor(pose[11] / Y.edge)};
                for (int cz = -3; cz <= 3; cz++)
                    for (int cy = -3; cy <= 3; cy++)
                        for (int cx = -3; cx <= 3; cx++) {
                            const int id[3] = {base[0] + cx, base[1] + cy, base[2] + cz};
                            const bool keep = deintegrate_keeps(Y, id[0], id[1], id[2]);
                            (keep ? kept : dropped)++;
                            if (keep) continue;
                            // a dropped chunk must hold no voxel on the image: its corners, its faces' voxels and a random sample
                            for (int s = 0; s < 96; s++) {
                                int v[3];
                                for (int k = 0; k < 3; k++) v[k] = s < 8 ? ((s >> k) & 1) * (N - 1) : (int)(uniform() * N) % N;
                                if (s >= 8 && s < 56) v[s % 3] = (s & 4) ? N - 1 : 0;
                                const float px = ((float)v[0] * res + half) + (float)(N * id[0]) * res, py = ((float)v[1] * res + half) + (float)(N * id[1]) * res,
                                            pz = ((float)v[2] * res + half) + (float)(N * id[2]) * res;
                                voxels++;
                                if (on_image(pose, K.fx, K.fy, K.cx, K.cy, K.W, K.H, px, py, pz)) {
                                    printf("FAIL: chunk (%d, %d, %d) of %d^3 dropped, voxel (%d, %d, %d) is on the image (camera fx %g, trial %d)\n", id[0], id[1], id[2], N,
                                           v[0], v[1], v[2], K.fx, trial);
                                    return 1;
                                }
                            }
                        }
            }
        }
    if (dropped < kept / 4 || kept < 1000) {
        printf("FAIL: the planes reject too little to be tested: kept %ld dropped %ld\n", kept, dropped);
        return 1;
    }
    // the refusals
    float depth[4] = {1, 1, 1, 1}, pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float inf = INFINITY, nan = NAN;
    int bad = 0;
    // the image check on its own, as the alignment entries call it: its verdicts, and that de-integration's refusal gives the same ones
    struct Image { const float *depth; int W, H; bool refused; };
    const Image images[] = {{depth, 2, 2, false}, {depth, 1, 1, false}, {depth, 46340, 46341, false}, {depth, INT32_MAX, 1, false},
                            {nullptr, 2, 2, true}, {depth, 0, 2, true}, {depth, 2, 0, true}, {depth, -3, -3, true}, {depth, INT32_MIN, 1, true},
                            {depth, 46341, 46341, true}, {depth, 1 << 16, 1 << 15, true}, {depth, INT32_MAX, INT32_MAX, true}};
    for (const Image &I : images) {
        const char *why = frame_image_refusal(I.depth, I.W, I.H);
        bad += (why != nullptr) != I.refused;
        bad += why != deintegrate_refusal(I.depth, I.W, I.H, pose, 1, 1, 1, 1, true, true, 4);  // (the same literal, or both null)
    }
    bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, 1, 1, true, true, 4) != nullptr;
    bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, 1, 1, false, false, 0) != nullptr;
    bad += deintegrate_refusal(nullptr, 2, 2, pose, 1, 1, 1, 1, true, true, 4) == nullptr;
    bad += deintegrate_refusal(depth, 0, 2, pose, 1, 1, 1, 1, true, true, 4) == nullptr;
    bad += deintegrate_refusal(depth, 2, -1, pose, 1, 1, 1, 1, true, true, 4) == nullptr;
    bad += deintegrate_refusal(depth, 1 << 16, 1 << 15, pose, 1, 1, 1, 1, true, true, 4) == nullptr;
    bad += deintegrate_refusal(depth, 46341, 46341, pose, 1, 1, 1, 1, true, true, 4) == nullptr;  // (overflows a 32-bit product)
    bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, 1, 1, true, true, -1) == nullptr;
    bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, 1, 1, false, true, 4) == nullptr;
    for (int i = 0; i < 12; i++)
        for (float v : {inf, -inf, nan}) {
            float p[12];
            memcpy(p, pose, sizeof(p));
            p[i] = v;
            bad += deintegrate_refusal(depth, 2, 2, p, 1, 1, 1, 1, true, true, 4) == nullptr;
        }
    for (float v : {inf, -inf, nan}) {
        bad += deintegrate_refusal(depth, 2, 2, pose, v, 1, 1, 1, true, true, 4) == nullptr;
        bad += deintegrate_refusal(depth, 2, 2, pose, 1, v, 1, 1, true, true, 4) == nullptr;
        bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, v, 1, true, true, 4) == nullptr;
        bad += deintegrate_refusal(depth, 2, 2, pose, 1, 1, 1, v, true, true, 4) == nullptr;
    }
    if (bad) {
        printf("FAIL: %d refusal verdicts are wrong\n", bad);
        return 1;
    }
    printf("ok: %ld chunks kept, %ld dropped, %ld voxels of dropped chunks projected, none on the image\n", kept, dropped, voxels);
    return 0;
}

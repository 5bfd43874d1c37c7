// kernels_gather.h -- chisel_hip_gather_meshes: a segmented copy from the mesh arenas into the caller's contiguous arrays (the host
// side: host_gather.h; the segment table: gather_checks.h; the definition: DESIGN.md 3.12).
//
// The destination space is the concatenation of all segments (every requested array of every selected mesh, array by array).  A
// workgroup owns one tile of GATHER_TILE_FLOATS consecutive floats of it, whatever meshes those belong to: it finds the segment that
// holds its first float by a binary search over the segments' starts and walks on from there, so a tile may hold dozens of tiny
// meshes and a mesh may span many tiles, and the load balance does not depend on mesh sizes.  The search and the walk read the table
// at addresses that depend on blockIdx alone: scalar loads, once per wave.  No atomics, no LDS, no scratch.
//
// Only 4-byte alignment is given (a mesh starts at a multiple of 9 floats in its arena and anywhere in the destination): the copy
// moves dwords.  Peeling a piece to 16-byte accesses where source and destination agree modulo 4 floats was built and measured, and
// was not faster (EXPERIMENTS.md).
#pragma once

namespace chisel_hip {

struct GatherSeg {      // one segment as the kernel takes it, 32 bytes
    const float *src;   // its first source float in the arena
    float *dst;         // its first float in the caller's array
    long long start;    // floats of all segments before it
    int len;            // destination floats
    int kind;           // GATHER_COPY, GATHER_RGBA_FROM_COLOR, GATHER_RGBA_FROM_NORMAL
};
static_assert(sizeof(GatherSeg) == 32, "GatherSeg is read with scalar loads of 32 bytes");

struct GatherLights {   // chisel_hip_mesh_request's, as given
    float l0[3], l1[3], diffuse, ambient;
};

constexpr int GATHER_THREADS = 256;
typedef __attribute__((address_space(1))) float GatherGlobalFloat;
typedef float GatherFloat4 __attribute__((ext_vector_type(4)));  // (a native vector: HIP's float4 is a struct, which takes no address space)
typedef __attribute__((address_space(1))) GatherFloat4 GatherGlobalFloat4;

// FillMarkerTopicWithMeshes' second branch (ChiselServer.cpp:676-690), every operation rounded on its own (-ffp-contract=off)
__device__ __forceinline__ float gather_lambert(float nx, float ny, float nz, const GatherLights &L) {
    const float d0 = (nx * L.l0[0] + ny * L.l0[1]) + nz * L.l0[2];
    const float d1 = (nx * L.l1[0] + ny * L.l1[1]) + nz * L.l1[2];
    const float s0 = fmaxf(d0, 0.0f) * L.diffuse;  // (fmaxf of a NaN and 0 is 0)
    const float s1 = fmaxf(d1, 0.0f) * L.diffuse;
    const float c = (s0 + s1) + L.ambient;
    return fminf(c, 1.0f);
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_meshes_kernel(const GatherSeg *__restrict__ segs, int n_segs, long long total, GatherLights L) {
    const long long t0 = (long long)blockIdx.x * GATHER_TILE_FLOATS;
    const long long t1 = t0 + GATHER_TILE_FLOATS < total ? t0 + GATHER_TILE_FLOATS : total;
    const int tid = (int)threadIdx.x;
    // the last segment that starts at or before the tile's first float (segs[0].start == 0)
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].start <= t0) lo = mid;
        else hi = mid - 1;
    }
    for (int s = lo; s < n_segs; s++) {
        const GatherSeg g = segs[s];
        if (g.start >= t1) break;
        // the piece of the segment inside the tile, in floats from the segment's start
        const int a = g.start < t0 ? (int)(t0 - g.start) : 0;
        const int b = g.start + g.len > t1 ? (int)(t1 - g.start) : g.len;
        // (pointers read from a table are generic to the compiler: said to be global, the accesses are global_load / global_store and a
        // store is not waited for before the next load)
        const GatherGlobalFloat *__restrict__ src = (const GatherGlobalFloat *)g.src;
        GatherGlobalFloat *__restrict__ dst = (GatherGlobalFloat *)g.dst;
        if (g.kind == GATHER_COPY) {
            // four loads in flight per lane, then their stores
            for (int i = a + tid; i < b; i += 4 * GATHER_THREADS) {
                float r[4];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i + k * GATHER_THREADS < b) r[k] = src[i + k * GATHER_THREADS];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i + k * GATHER_THREADS < b) dst[i + k * GATHER_THREADS] = r[k];
            }
        } else {
            // four floats per vertex from the three of its colour or normal; a tile edge may cut a vertex
            const bool whole_ok = ((unsigned long long)dst & 15) == 0;
            for (int v = (a >> 2) + tid; 4 * v < b; v += GATHER_THREADS) {
                const float x = src[3 * v], y = src[3 * v + 1], z = src[3 * v + 2];
                GatherFloat4 o;
                if (g.kind == GATHER_RGBA_FROM_COLOR) {
                    o.x = x; o.y = y; o.z = z;
                } else {
                    o.x = o.y = o.z = gather_lambert(x, y, z, L);
                }
                o.w = 1.0f;
                const int f = 4 * v;
                if (whole_ok && f >= a && f + 4 <= b) {
                    *(GatherGlobalFloat4 *)(dst + f) = o;
                } else {
                    if (f >= a && f < b) dst[f] = o.x;
                    if (f + 1 >= a && f + 1 < b) dst[f + 1] = o.y;
                    if (f + 2 >= a && f + 2 < b) dst[f + 2] = o.z;
                    if (f + 3 >= a && f + 3 < b) dst[f + 3] = o.w;
                }
            }
        }
    }
}

}  // namespace chisel_hip

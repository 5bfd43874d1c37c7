// gather_checks.h -- the host-side pieces of chisel_hip_gather_meshes that call nothing of HIP (included by chisel_hip.hip for host_gather.h and, on its
// own, by tests/gather_checks_check.cpp, which runs them under the address and undefined-behaviour sanitizers on the CPU): what the
// entry refuses about its request and its outputs, and the segment table of a selection -- where every requested array of every mesh
// sits in its arena, where it goes, the prefix over all segments, the tiles, the totals and the capacity and overflow checks.
// DESIGN.md 3.12 is the definition.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace chisel_hip {

constexpr int GATHER_TILE_FLOATS = 4096;                 // = CHISEL_HIP_GATHER_TILE_FLOATS: what one workgroup copies
constexpr int64_t GATHER_MAX_FLOATS = 0x7fffffffll;      // floats of one output array
constexpr int GATHER_REFUSED_INVALID = 1, GATHER_REFUSED_UNSUPPORTED = 5;  // = CHISEL_HIP_ERR_INVALID, CHISEL_HIP_ERR_UNSUPPORTED
enum { GATHER_VERTICES = 0, GATHER_NORMALS = 1, GATHER_COLORS = 2, GATHER_RGBA = 3, GATHER_GRIDS = 4, GATHER_ARRAYS = 5 };
// what a segment's floats are made from: copied as they are, or four per vertex from the three of its colour / of its normal
enum { GATHER_COPY = 0, GATHER_RGBA_FROM_COLOR = 1, GATHER_RGBA_FROM_NORMAL = 2 };

// the outputs asked for, in the order of the enum above
struct GatherOutputs {
    bool want[GATHER_ARRAYS];
    bool any() const { return want[0] || want[1] || want[2] || want[3] || want[4]; }
};

// what chisel_hip_gather_meshes refuses about its request and its outputs before it looks at the map's meshes, in the order of the
// header; null = go on.  Request: chisel_hip_mesh_request (a template, so that this header goes on including nothing of the
// library's).  id_limit: the largest |id| per axis the map can hold.  *bad_id: the index of an id out of range, else -1.
// check_outputs = false is chisel_hip_gather_meshes_size, which has none.
template <class Request>
inline const char *gather_request_refusal(const Request *r, bool check_outputs, const GatherOutputs &out, bool map_has_color, int id_limit, int64_t *bad_id) {
    *bad_id = -1;
    if (!r) return "null request";
    if (r->n_ids < 0) return "a negative number of ids";
    if (r->ids_xyz && r->n_ids == 0) return "an id list without a count";
    if (!r->ids_xyz && r->n_ids > 0) return "a count without an id list";
    for (int64_t i = 0; i < r->n_ids; i++)
        for (int a = 0; a < 3; a++)
            if (r->ids_xyz[3 * i + a] < -id_limit || r->ids_xyz[3 * i + a] > id_limit) {
                *bad_id = i;
                return "a chunk id outside the addressable range";
            }
    if (check_outputs && !out.any()) return "no output asked for";
    if (r->marker_colors) {
        for (int a = 0; a < 3; a++)
            if (!isfinite(r->light0[a]) || !isfinite(r->light1[a])) return "a light direction that is not finite";
        if (!isfinite(r->diffuse) || !isfinite(r->ambient)) return "diffuse or ambient is not finite";
    }
    if (check_outputs && out.want[GATHER_RGBA] && !r->marker_colors) return "rgba asked for without marker_colors";
    if (check_outputs && out.want[GATHER_COLORS] && !map_has_color) return "colours asked of a map without colour";
    return nullptr;
}

// one mesh of the selection, as the map's bookkeeping has it: its arena (-1: the mesh is empty), its first vertex and first grid
// entry there, its sizes, and the arena's own vertex count and colour flag (the arena is vertices | normals | colours | grids, 3 floats
// per entry: host_mesh.h, view_mesh)
struct GatherSource {
    int arena;
    int64_t v_off, n_v, g_off, n_g;
    int64_t arena_nv;
    bool arena_color;
};

// `len` floats of output array `array`, written from `dst` (floats from the array's start) on; made from the floats of arena `arena`
// at `src` on (kind COPY: as many; the RGBA kinds: len / 4 * 3).  `start`: the floats of all segments before this one.
struct GatherSegment {
    int64_t src, dst, start;
    int32_t len, arena, array, kind;
};

struct GatherTotals {  // = chisel_hip_mesh_totals
    int64_t meshes, meshes_nonempty, vertices, grids, arenas_read, tiles;
};

struct GatherPlan {
    std::vector<GatherSegment> segments;  // array by array in the enum's order, mesh by mesh inside; none of length 0
    std::vector<int64_t> table;           // 4 per mesh: first vertex, vertices, first grid, grids
    int64_t floats = 0;                   // of all segments: segments.back().start + .len
    GatherTotals totals{};
};

// The totals and the table of a selection over the arrays `out` names, and with `build` its segments (the size call names every array
// the map and the request could give and builds none).  Null = fine; otherwise *code says what kind of refusal it is.  The totals are complete also when the capacity is too small, so
// that the caller can retry; the table and the segments are then not to be used.  with_capacity = false: no capacity check.
inline const char *gather_plan(const GatherSource *src, int64_t n, const GatherOutputs &out, bool build, bool with_capacity,
                               int64_t capacity_vertices, int64_t capacity_grids, GatherPlan *plan, int *code) {
    *code = 0;
    plan->segments.clear();
    plan->table.assign((size_t)n * 4, 0);
    plan->floats = 0;
    GatherTotals &T = plan->totals;
    T = GatherTotals{n, 0, 0, 0, 0, 0};
    std::vector<int> arenas;  // the distinct arenas read (few: one per recompute that still has a live mesh)
    for (int64_t i = 0; i < n; i++) {
        const GatherSource &s = src[i];
        const bool empty = s.arena < 0 || s.n_v + s.n_g == 0;
        int64_t *row = plan->table.data() + 4 * i;
        row[0] = T.vertices;
        row[2] = T.grids;
        if (empty) {  // a row of zeros
            row[0] = row[2] = 0;
            continue;
        }
        row[1] = s.n_v;
        row[3] = s.n_g;
        T.meshes_nonempty++;
        T.vertices += s.n_v;  // (a mesh holds fewer than 2^31 / 9 vertices and n fits 63 bits together with it only if the list does: no overflow below 2^63 for any list that fits in memory)
        T.grids += s.n_g;
        bool seen = false;
        for (int a : arenas) seen = seen || a == s.arena;
        if (!seen) arenas.push_back(s.arena);
    }
    T.arenas_read = (int64_t)arenas.size();
    // floats per array, in 64 bits; one array beyond 2^31 - 1 floats is not served
    const int64_t per_vertex[GATHER_ARRAYS] = {3, 3, 3, 4, 0}, per_grid[GATHER_ARRAYS] = {0, 0, 0, 0, 3};
    int64_t all = 0;
    for (int a = 0; a < GATHER_ARRAYS; a++) {
        const int64_t f = T.vertices * per_vertex[a] + T.grids * per_grid[a];
        if (out.want[a] && f > GATHER_MAX_FLOATS) {
            *code = GATHER_REFUSED_UNSUPPORTED;
            return "the selection holds more than 2^31 - 1 floats in one array";
        }
        if (out.want[a]) all += f;
    }
    T.tiles = (all + GATHER_TILE_FLOATS - 1) / GATHER_TILE_FLOATS;
    // (a capacity speaks of the arrays that are asked for: grids alone need no room for vertices)
    const bool per_vertex_asked = out.want[GATHER_VERTICES] || out.want[GATHER_NORMALS] || out.want[GATHER_COLORS] || out.want[GATHER_RGBA];
    if (with_capacity && ((per_vertex_asked && capacity_vertices < T.vertices) || (out.want[GATHER_GRIDS] && capacity_grids < T.grids))) {
        *code = GATHER_REFUSED_INVALID;
        return "the capacity is below the selection's totals";
    }
    if (!build) return nullptr;
    int64_t start = 0;
    for (int a = 0; a < GATHER_ARRAYS; a++) {
        if (!out.want[a]) continue;
        for (int64_t i = 0; i < n; i++) {
            const GatherSource &s = src[i];
            if (s.arena < 0) continue;
            const int64_t *row = plan->table.data() + 4 * i;
            const int64_t nv3 = 3 * s.arena_nv;
            GatherSegment g;
            g.arena = s.arena;
            g.array = a;
            g.kind = GATHER_COPY;
            g.start = start;
            int64_t len = 3 * s.n_v;
            switch (a) {
                case GATHER_VERTICES: g.src = 3 * s.v_off; g.dst = 3 * row[0]; break;
                case GATHER_NORMALS: g.src = nv3 + 3 * s.v_off; g.dst = 3 * row[0]; break;
                case GATHER_COLORS:
                    if (!s.arena_color) continue;  // (refused before: a map with colour has it in every arena)
                    g.src = 2 * nv3 + 3 * s.v_off; g.dst = 3 * row[0];
                    break;
                case GATHER_RGBA:
                    g.kind = s.arena_color ? GATHER_RGBA_FROM_COLOR : GATHER_RGBA_FROM_NORMAL;
                    g.src = (s.arena_color ? 2 * nv3 : nv3) + 3 * s.v_off; g.dst = 4 * row[0];
                    len = 4 * s.n_v;
                    break;
                default:
                    g.src = nv3 * (s.arena_color ? 3 : 2) + 3 * s.g_off; g.dst = 3 * row[2];
                    len = 3 * s.n_g;
                    break;
            }
            if (len == 0) continue;
            g.len = (int32_t)len;  // (<= the array's floats <= 2^31 - 1)
            plan->segments.push_back(g);
            start += len;
        }
    }
    plan->floats = start;
    return nullptr;
}

}  // namespace chisel_hip

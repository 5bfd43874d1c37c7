"""Hand-built voxel fields for the mesh, query and ray kernels, and what they contain (TEST INFRASTRUCTURE, numpy only).

The suite's integrated scenes (wall, sphere_room, box_room with ConstantWeighter(1)) reach 29 of the 256 marching-cubes
configurations, no weight in (0, 0.5], no crossing edge with |s1 - s2| below 6.8e-5, no -0.0 and no denormal (DESIGN.md "What the mesh
tests cover").  The two families here are built to hit what those maps leave out.  A field is a dict
chunk id (x, y, z) -> (sdf[N^3], weight[N^3], rgbw[N^3, 4]) -- what Chisel.AddChunk and OracleMap.put_chunk take -- for a B x B x B block
of chunks based at a chunk id; voxel id = (z N + y) N + x (Chunk.h:81-84).  The voxels are drawn for the block as one (B N)^3 grid
and do not depend on the base, so the same field can be placed anywhere.

The predicates count what a field contains from the field alone (no kernel, no oracle): the cube configuration per section of the
reference's traversal, fully observed cubes, crossing edges whose difference is below InterpolateVertex's 1e-6, weight and value
classes, and the two branches of InterpolateColor by its eight residency look-ups.
"""
import numpy as np

F = np.float32
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))  # ChunkManager.cpp:67-69 (x, y, z)
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))  # MarchingCubes.cpp edgeIndexPairs
SECTIONS = ("interior", "max_x", "max_y", "max_z")  # ChunkManager.cpp:381-447, in the order GenerateMesh walks them
MIN_DIFF = F(1e-6)  # MarchingCubes.h:137

W_EDGE = F(1e-12)  # widens to less than the double 1e-12 GetSDF compares with (ChunkManager.cpp:489): reads as unobserved
W_EDGE_NEXT = np.nextafter(W_EDGE, F(1))  # ... and its successor as observed
W_HALF_NEXT = np.nextafter(F(0.5), F(1))  # the smallest weight a cube accepts (weight <= 0.5 rejects, ChunkManager.cpp:276)
HIGH_WEIGHTS = np.array([W_HALF_NEXT, 1.0, 2.5, 100.0], np.float32)
LOW_WEIGHTS = np.array([0.0, 1e-13, W_EDGE, W_EDGE_NEXT, 0.25, 0.5], np.float32)
assert float(W_EDGE) < 1e-12 < float(W_EDGE_NEXT)


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def _cut(grid_sdf, grid_w, grid_rgbw, N, B, base):
    """the (B N)^3 grids, indexed [z, y, x], cut into chunks"""
    out = {}
    for cz in range(B):
        for cy in range(B):
            for cx in range(B):
                sl = (slice(cz * N, (cz + 1) * N), slice(cy * N, (cy + 1) * N), slice(cx * N, (cx + 1) * N))
                cid = (int(base[0]) + cx, int(base[1]) + cy, int(base[2]) + cz)
                out[cid] = (np.ascontiguousarray(grid_sdf[sl]).reshape(-1), np.ascontiguousarray(grid_w[sl]).reshape(-1),
                            np.ascontiguousarray(grid_rgbw[sl]).reshape(-1, 4))
    return out


def block_ids(B, base=(0, 0, 0)):
    return [(int(base[0]) + x, int(base[1]) + y, int(base[2]) + z) for z in range(B) for y in range(B) for x in range(B)]


def dense(N, B, seed, res=0.05, base=(0, 0, 0)):
    """every weight 1, every sign independent with p = 0.5, |sdf| uniform in [0.05 res, res]: every cube inside the block is fully
    observed and its configuration is uniform over the 256"""
    rng = np.random.default_rng(seed)
    n = B * N
    mag = rng.uniform(0.05 * res, res, (n, n, n))
    sign = np.where(rng.random((n, n, n)) < 0.5, -1.0, 1.0)
    rgbw = rng.integers(0, 256, (n, n, n, 4), dtype=np.uint8)
    return _cut((sign * mag).astype(np.float32), np.ones((n, n, n), np.float32), rgbw, N, B, base)


def thresholds(N, B, seed, res=0.05, base=(0, 0, 0)):
    """value classes of |sdf| (sign random, so the zeros are +0.0 and -0.0): 50 % [0.05 res, res], 20 % [1e-8, 4e-7], 10 % 0.0,
    10 % denormal [1e-42, 1e-39], 10 % [1, 1e3].  Weights: 85 % from HIGH_WEIGHTS, 15 % from LOW_WEIGHTS.  No NaN, no infinity."""
    rng = np.random.default_rng(seed)
    n = B * N
    shape = (n, n, n)
    cls = rng.choice(5, shape, p=[0.5, 0.2, 0.1, 0.1, 0.1])
    u = rng.random(shape)
    lo = np.array([0.05 * res, 1e-8, 0.0, 1e-42, 1.0])[cls]
    hi = np.array([res, 4e-7, 0.0, 1e-39, 1e3])[cls]
    mag = (lo + u * (hi - lo)).astype(np.float32)
    sign = np.where(rng.random(shape) < 0.5, F(-1), F(1))
    sdf = (sign * mag).astype(np.float32)
    high = rng.random(shape) < 0.85
    w = np.where(high, HIGH_WEIGHTS[rng.integers(0, len(HIGH_WEIGHTS), shape)], LOW_WEIGHTS[rng.integers(0, len(LOW_WEIGHTS), shape)])
    rgbw = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    assert np.isfinite(sdf).all()
    return _cut(sdf, w.astype(np.float32), rgbw, N, B, base)


# ---- predicates ----------------------------------------------------------------------------------------------------------------------
class Cubes:
    """every cube of a field whose eight corners lie in resident chunks of the field: the corner values (8, n) in the order of
    CORNERS, the section of GenerateMesh's traversal that visits the cube, and the chunk that owns it."""

    def __init__(self, field, N):
        ids = np.array(sorted(field), np.int64).reshape(-1, 3)
        self.N = N
        self.lo = ids.min(0)
        dim = ids.max(0) - self.lo + 1
        gx, gy, gz = (int(d) * N for d in dim)
        self.sdf = np.zeros((gz, gy, gx), np.float32)
        self.wgt = np.zeros((gz, gy, gx), np.float32)
        present = np.zeros((gz, gy, gx), bool)
        for cid, (s, w, _) in field.items():
            x, y, z = (np.array(cid) - self.lo) * N
            self.sdf[z:z + N, y:y + N, x:x + N] = np.asarray(s, np.float32).reshape(N, N, N)
            self.wgt[z:z + N, y:y + N, x:x + N] = np.asarray(w, np.float32).reshape(N, N, N)
            present[z:z + N, y:y + N, x:x + N] = True
        corner = lambda a, c: a[c[2]:gz - 1 + c[2], c[1]:gy - 1 + c[1], c[0]:gx - 1 + c[0]]
        inside = np.all([corner(present, c) for c in CORNERS], axis=0)
        pick = np.nonzero(inside)  # (z, y, x) of the cube's corner 0, cubes in C order of (z, y, x)
        self.s = np.stack([corner(self.sdf, c)[pick] for c in CORNERS])
        self.w = np.stack([corner(self.wgt, c)[pick] for c in CORNERS])
        z, y, x = pick
        lx, ly, lz = x % N, y % N, z % N
        self.section = np.where(lz == N - 1, 3, np.where(lx == N - 1, 1, np.where(ly == N - 1, 2, 0)))
        self.chunk = np.stack([x // N, y // N, z // N], axis=1) + self.lo
        self.local = np.stack([lx, ly, lz], axis=1)
        self.config = sum(((self.s[i] < 0).astype(np.int64) << i) for i in range(8))  # MarchingCubes.h:108-118
        self.observed = (self.w > F(0.5)).all(0)  # ChunkManager.cpp:276, 356
        self.occupied = self.observed & (self.config != 0) & (self.config != 255)

    def configurations(self):
        """{section name: sorted configurations of the fully observed cubes of that section}"""
        return {name: np.unique(self.config[self.observed & (self.section == k)]) for k, name in enumerate(SECTIONS)}

    def rejected_only_by_small_weights(self):
        """cubes that are not fully observed although GetSDF would find all eight corners: every corner has a weight above 1e-12 (as
        a double) and at least one of them is 0.5 or below"""
        found = (self.w.astype(np.float64) > 1e-12).all(0)
        return int((found & ~self.observed).sum())

    def tiny_crossing_edges(self):
        """sign-changing edges of meshed cubes with |s1 - s2| < 1e-6 in float32 (MarchingCubes.h:135-146), an edge counted once per
        cube it belongs to"""
        total = 0
        for a, b in EDGES:
            s1, s2 = self.s[a], self.s[b]
            crossing = (s1 < 0) != (s2 < 0)
            total += int((self.occupied & crossing & (np.abs(s1 - s2) < MIN_DIFF)).sum())
        return total

    def observed_corners(self):
        """(denormal, -0.0) corners of fully observed cubes, a voxel counted once per cube it is a corner of"""
        s = self.s[:, self.observed]
        tiny = np.finfo(np.float32).tiny
        return int(((s != 0) & (np.abs(s) < tiny)).sum()), int(((s == 0) & np.signbit(s)).sum())

    def triangles(self, vertex_counts):
        """total triangles of the meshed cubes, given the table's vertex count per configuration"""
        return int(np.asarray(vertex_counts)[self.config[self.occupied]].sum()) // 3

    def traversal_order(self, cid):
        """the cubes of chunk `cid` as rows of this object, in GenerateMesh's order (ChunkManager.cpp:381-447): the interior z, y, x;
        the max-x plane z, y; the max-y plane z, x; the max-z plane y, x"""
        rows = np.flatnonzero((self.chunk == np.asarray(cid)).all(1))
        lx, ly, lz = self.local[rows].T
        sec = self.section[rows]
        # within a section the reference's loops are nested z, y, x (missing loops are constant)
        return rows[np.lexsort((lx, ly, lz, sec))]


def weight_classes(field):
    """{weight value: count} over the voxels of the field"""
    w = np.concatenate([np.asarray(v[1], np.float32) for v in field.values()])
    vals, counts = np.unique(w, return_counts=True)
    return {float(v): int(c) for v, c in zip(vals, counts)}


def value_classes(field):
    """{class name: count} over the distances of the field: "+0.0", "-0.0", "denormal" (non-zero below the smallest normal float32),
    "tiny" (normal, below 1e-6: two of them of opposite sign take InterpolateVertex's degenerate branch), "large" (1 and above),
    "band" (the rest), "negative" (sdf < 0, what the case index asks: -0.0 is not), and "non-finite"."""
    s = np.concatenate([np.asarray(v[0], np.float32) for v in field.values()])
    a = np.abs(s)
    smallest = np.finfo(np.float32).tiny
    fin = np.isfinite(s)
    zero, denormal, tiny, large = s == 0, (s != 0) & (a < smallest), (a >= smallest) & (a < MIN_DIFF), fin & (a >= 1)
    out = {"+0.0": zero & ~np.signbit(s), "-0.0": zero & np.signbit(s), "denormal": denormal, "tiny": tiny, "large": large,
           "band": fin & ~zero & ~denormal & ~tiny & ~large, "negative": s < 0, "non-finite": ~fin}
    return {k: int(v.sum()) for k, v in out.items()}


def check_dense(field, N):
    """the condition a dense field must meet: all 256 configurations in each of the four sections"""
    cubes = Cubes(field, N)
    assert cubes.observed.all()
    values = value_classes(field)
    assert values["band"] == sum(len(v[0]) for v in field.values()), values  # (nothing but [0.05 r, r])
    for name, seen in cubes.configurations().items():
        assert len(seen) == 256, "dense N = %d: %d of 256 configurations in section %s" % (N, len(seen), name)
    return cubes


def check_thresholds(field, N):
    """the conditions a thresholds field must meet"""
    cubes = Cubes(field, N)
    share = float(cubes.observed.mean())
    assert share >= 0.20, share
    assert cubes.rejected_only_by_small_weights() >= 1000
    assert cubes.tiny_crossing_edges() >= 1000
    denormal, negative_zero = cubes.observed_corners()
    assert denormal >= 1000 and negative_zero >= 500, (denormal, negative_zero)
    classes = weight_classes(field)
    assert float(W_EDGE) in classes and float(W_EDGE_NEXT) in classes
    values = value_classes(field)
    assert values["non-finite"] == 0 and all(values[k] > 0 for k in ("+0.0", "-0.0", "denormal", "tiny", "large", "band")), values
    return cubes


# ---- InterpolateColor's branch, by its residency look-ups alone -----------------------------------------------------------------------
def color_branch(index, vertices):
    """ChunkManager.cpp:501-573: the eight GetColorVoxel look-ups at the integer voxel indices of the vertex taken for metres (sic,
    :506-520).  -> (n,) bool: True = all eight voxels exist, the trilinear branch; False = the nearest-voxel fallback.
    index: a render_restated.VoxelIndex of the map (its chunk-id and linear-id computation is GetColorVoxel's, :588-607)."""
    from tests import query_restated as qr
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    i0 = np.floor(v / index.res).astype(np.int32)
    all_there = np.ones(len(v), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                pos = (i0 + np.array([dx, dy, dz], np.int32)).astype(np.float32)
                ok, _ = qr.sample_weight(index, pos)
                all_there &= ok
    return all_there

"""chisel_hip_align_terms, chisel_hip_align_solve and chisel_hip_align_depth restated in numpy (TEST INFRASTRUCTURE: DESIGN.md
"Aligning a frame to the map" is the definition), and the scenes the CPU and the GPU tests share.

Built on tests/render_restated.py: VoxelIndex.sample is ChunkManager::GetSDF, rays / hit_points are chisel_hip_render_view's.  The
per-pixel part is float32, one rounding per operation, in the order the definition writes it; the Jacobian, the sums, the solver and
the pose update are float64.  Every sum is taken by `pairwise`, the fixed tree of the definition."""
import math

import numpy as np

from cvids_amd import synth
from tests import render_restated as rr

F = np.float32
CONVERGED, ITERATION_LIMIT, TOO_FEW_PIXELS, DEGENERATE = 0, 1, 2, 3


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def voxel_centre(index, pos):
    """floorf(p / r) r + r / 2 per axis: where GetSDFAndGradient reads its distance"""
    r = index.res
    with np.errstate(invalid="ignore"):
        return (np.floor(pos / r) * r + r / F(2)).astype(np.float32)


def grad_sample(index, pos):
    """ChunkManager::GetSDFAndGradient as kernels_mesh.h: get_sdf_and_gradient<N> restates it, by seven VoxelIndex.sample calls:
    pos (n, 3) float32 -> (found (n,) bool, distance at the voxel centre (n,) float32, gradient (n, 3) float32, normalised as Eigen's
    normalized() does it: z = a0 a0 + (a1 a1 + a2 a2), a / sqrt(z) where z > 0).  Distance and gradient are meaningless where not
    found.  A position with a non-finite component is not found."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    fin = np.isfinite(pos).all(1)
    c = voxel_centre(index, np.where(fin[:, None], pos, F(0)))
    r = index.res
    found = fin.copy()
    d = []
    for axis, sign in ((None, 0), (0, 1), (1, 1), (2, 1), (0, -1), (1, -1), (2, -1)):
        q = c.copy()
        if axis is not None:
            q[:, axis] = c[:, axis] + r if sign > 0 else c[:, axis] - r
        obs, s, _ = index.sample(q)
        found &= obs
        d.append(s)
    a = np.stack([(d[1].astype(np.float64) - d[4].astype(np.float64)).astype(np.float32),
                  (d[2].astype(np.float64) - d[5].astype(np.float64)).astype(np.float32),
                  (d[3].astype(np.float64) - d[6].astype(np.float64)).astype(np.float32)], axis=1)
    z = a[:, 0] * a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where((z > 0)[:, None], a / np.sqrt(z)[:, None], a).astype(np.float32)
    return found, d[0], g


def pairwise(x):
    """the sum of the float64 values x in the order of the definition: padded with +0.0 to a multiple of 256, neighbours
    x[2j] + x[2j+1] added eight times in every group of 256, the same again over the group results until one value is left"""
    x = np.asarray(x, np.float64).reshape(-1)
    assert len(x) >= 1
    while True:
        pad = (-len(x)) % 256
        x = np.concatenate([x, np.zeros(pad, np.float64)]).reshape(-1, 256)
        for _ in range(8):
            x = x[:, 0::2] + x[:, 1::2]
        x = x.reshape(-1)
        if len(x) == 1:
            return x[0]


def pixel_terms(index, depth, pose, intr, near, far, max_residual=0.0):
    """-> (valid, used (n,) bool, J (n, 6) float64, rho (n,) float32, p (n, 3) float32) per pixel in row-major order"""
    depth = np.ascontiguousarray(depth, np.float32)
    z = depth.reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(z) & (F(near) <= z) & (z <= F(far))
        p = rr.hit_points(np.asarray(pose, np.float32), intr, depth)
    fin = valid & np.isfinite(p).all(1)
    found, d0, g = grad_sample(index, np.where(fin[:, None], p, F(0)))
    ok = fin & found
    with np.errstate(invalid="ignore"):
        e = p - voxel_centre(index, p)
        rho = d0 + ((g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1]) + g[:, 2] * e[:, 2])
        used = ok & (np.abs(rho) <= F(max_residual)) if max_residual > 0 else ok
        g64, p64 = g.astype(np.float64), p.astype(np.float64)
        J = np.stack([g64[:, 0], g64[:, 1], g64[:, 2],
                      p64[:, 1] * g64[:, 2] - p64[:, 2] * g64[:, 1],
                      p64[:, 2] * g64[:, 0] - p64[:, 0] * g64[:, 2],
                      p64[:, 0] * g64[:, 1] - p64[:, 1] * g64[:, 0]], axis=1)
    return valid, used, J, rho, p


def terms(index, depth, pose, intr, near, far, max_residual=0.0):
    """chisel_hip_align_terms: -> (32,) float64"""
    valid, used, J, rho, _ = pixel_terms(index, depth, pose, intr, near, far, max_residual)
    r64 = rho.astype(np.float64)
    zero = np.zeros(len(used), np.float64)
    out = np.zeros(32, np.float64)
    t = 0
    with np.errstate(invalid="ignore"):
        for a in range(6):
            for b in range(a, 6):
                out[t] = pairwise(np.where(used, J[:, a] * J[:, b], zero))
                t += 1
        for a in range(6):
            out[21 + a] = pairwise(np.where(used, J[:, a] * r64, zero))
        out[27] = pairwise(np.where(used, r64 * r64, zero))
    out[28] = pairwise(used.astype(np.float64))
    out[29] = pairwise(valid.astype(np.float64))
    return out


def solve(terms32, damping):
    """chisel_hip_align_solve, the Cholesky written out in Python floats (IEEE double, one rounding per operation): -> xi as a (6,)
    float64 array, or None where a pivot is refused"""
    T = [float(v) for v in terms32]
    damping = float(damping)
    A = [[0.0] * 6 for _ in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    t = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = T[t]
            t += 1
    add = damping * T[28]
    for j in range(6):
        A[j][j] += add
    largest = A[0][0]
    for j in range(1, 6):
        if A[j][j] > largest:
            largest = A[j][j]
    floor_s = 1e-12 * largest
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not s > floor_s:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        v = -T[21 + i]
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v / L[i][i]
    return np.array(x, np.float64)


def norm3(a):
    return math.sqrt((float(a[0]) * float(a[0]) + float(a[1]) * float(a[1])) + float(a[2]) * float(a[2]))


def apply(xi, pose):
    """pose <- exp(xi) pose (the left perturbation p' = p + v + w x p): R <- R_d R, t <- R_d t + v with Rodrigues' R_d; float64,
    -> (3, 4)"""
    xi = [float(v) for v in xi]
    P = np.asarray(pose, np.float64)[:3, :4]
    v, w = xi[:3], xi[3:]
    theta = norm3(w)
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    tiny = theta <= 1e-12
    a = 1.0 if tiny else math.sin(theta) / theta
    b = 0.0 if tiny else (1.0 - math.cos(theta)) / (theta * theta)
    Rd = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
            Rd[i][j] = ((1.0 if i == j else 0.0) + a * K[i][j]) + b * k2
    out = np.zeros((3, 4), np.float64)
    for i in range(3):
        for j in range(4):
            out[i, j] = (Rd[i][0] * float(P[0, j]) + Rd[i][1] * float(P[1, j])) + Rd[i][2] * float(P[2, j])
        out[i, 3] += v[i]
    return out


def align(index, depth, pose, intr, near, far, max_iterations=10, max_residual=0.0, damping=1e-3, min_translation=1e-5,
          min_rotation=1e-5, min_pixels=100):
    """chisel_hip_align_depth: the pose is kept in float64 and handed to `terms` rounded to float32"""
    P = np.asarray(pose, np.float32)[:3, :4].astype(np.float64)
    res = {"status": ITERATION_LIMIT, "iterations": 0, "xi_last": np.zeros(6), "terms_first": None, "terms_last": None, "poses": [P.copy()]}
    for it in range(max_iterations):
        T = terms(index, depth, P.astype(np.float32), intr, near, far, max_residual)
        if it == 0:
            res["terms_first"] = T
        res["terms_last"] = T
        if T[28] < min_pixels:
            res["status"] = TOO_FEW_PIXELS
            break
        xi = solve(T, damping)
        if xi is None:
            res["status"] = DEGENERATE
            break
        P = apply(xi, P)
        res["poses"].append(P.copy())
        res["xi_last"] = xi
        res["iterations"] = it + 1
        if norm3(xi[:3]) < min_translation and norm3(xi[3:]) < min_rotation:
            res["status"] = CONVERGED
            break
    res["pose"] = P
    return res


# ---- what the tests measure ------------------------------------------------------------------------------------------------------
def pose_errors(pose, true_pose):
    """-> (translation error [m], rotation error [degrees]) of a pose against the true one"""
    A, B = np.asarray(pose, np.float64)[:3, :4], np.asarray(true_pose, np.float64)[:3, :4]
    dR = A[:, :3] @ B[:, :3].T
    angle = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))))
    return float(np.linalg.norm(A[:, 3] - B[:, 3])), angle


def xi_of(tx, ty, tz, rx_deg, ry_deg, rz_deg):
    return np.array([tx, ty, tz, math.radians(rx_deg), math.radians(ry_deg), math.radians(rz_deg)], np.float64)


# ---- the scenes the CPU and the GPU tests share ----------------------------------------------------------------------------------
W, H = 160, 120
NEAR, FAR = 0.05, 5.0


def corner_pose(k):
    """yaw 38 + 0.5 k degrees about y, then pitch 22 degrees about x (R = R_y R_x), t = (0.6 + 0.01 k, 0.3, 0.9): from inside box_room
    this sees the x = 2 and z = 2.5 walls and a strip of the ceiling, so all six degrees of freedom are observable.  (A yaw-only
    trajectory sees one wall of box_room, sphere_room is centred on the camera, wall is a plane.)"""
    Ry = synth.pose_yaw(38.0 + 0.5 * k).astype(np.float64)[:3, :3]
    a = math.radians(22.0)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = (0.6 + 0.01 * k, 0.3, 0.9)
    return T.astype(np.float32)


# chunk edge, resolution, truncator of the two corner maps (box_room from corner_pose(0..7), carving on)
CORNER_MAPS = [(16, 0.02, ("inverse", 2.0)), (8, 0.03, ("constant", 0.1))]
CORNER_FRAMES = 8
CORNER_VIEW = 4  # the frame that is aligned: synth.render_depth at corner_pose(4)
# the three starts: the true pose left-multiplied by apply() of these (m, degrees)
CORNER_STARTS = [(0.012, -0.01, 0.012, 0.6, -0.6, 0.5), (-0.02, 0.015, 0.015, -0.9, 0.8, 0.9), (0.03, 0.03, -0.025, 1.2, 1.2, -1.0)]
# the wall: chunk edge, resolution, truncator, frames (trajectory poses 0..5), the view aligned, the start's offset
WALL_MAP = (16, 0.03, ("constant", 0.1), 6, 3)
WALL_START = (0.01, 0.0, 0.02, 0.5, 0.0, 0.0)


def corner_frames():
    """(depth, pose) of the corner maps' frames"""
    intr = synth.intrinsics(W, H)
    return [(synth.render_depth("box_room", corner_pose(k), intr, W, H), corner_pose(k)) for k in range(CORNER_FRAMES)]


def corner_frame():
    return synth.render_depth("box_room", corner_pose(CORNER_VIEW), synth.intrinsics(W, H), W, H)


def start_pose(true_pose, offset):
    return apply(xi_of(*offset), np.asarray(true_pose, np.float64))


def check_corner_run(poses, first_terms, true_pose, what):
    """the conditions a corner run is held to, on the CPU and on the GPU: translation and rotation error each end at most half of
    where they started, and at least 0.75 of the valid pixels are used in the first iteration"""
    t0, r0 = pose_errors(poses[0], true_pose)
    t1, r1 = pose_errors(poses[-1], true_pose)
    share = first_terms[28] / first_terms[29]
    print("%s: translation %.2f -> %.2f mm, rotation %.3f -> %.3f deg, used share %.3f" % (what, 1e3 * t0, 1e3 * t1, r0, r1, share))
    assert t1 <= 0.5 * t0, (what, t0, t1)
    assert r1 <= 0.5 * r0, (what, r0, r1)
    assert share >= 0.75, (what, share)

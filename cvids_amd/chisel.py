"""Host-side mirror of the reference's operator interface for the TSDF path, over the C ABI.

Names and argument meaning follow OpenChisel (open_chisel/include/open_chisel/*.h) so the parity
tests read like the reference's call sites (chisel_ros/src/ChiselServer.cpp:480-516):

    chisel = Chisel((16, 16, 16), 0.01, use_color=True)
    integrator = ProjectionIntegrator(InverseTruncator(1.0), ConstantWeighter(1), 0.05, True)
    chisel.IntegrateDepthScanColor(integrator, depth, pose, camera, color, pose, camera)
    chisel.UpdateMeshes()

Images may be numpy arrays (host, copied in by the library) or torch CUDA tensors (used in place).
Every call goes to libchisel_hip.so; nothing is computed in Python.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import ColorFrame, Config, DepthFrame, Integrator, check


# ---- strategy objects (truncation/*.h, weighting/ConstantWeighter.h) ---------------------------------
class ConstantTruncator:
    kind = capi.TRUNC_CONSTANT

    def __init__(self, value):
        self.param = float(value)


class InverseTruncator:
    kind = capi.TRUNC_INVERSE

    def __init__(self, scale):
        self.param = float(scale)


class QuadraticTruncator:
    kind = capi.TRUNC_QUADRATIC

    def __init__(self, scale):
        self.param = float(scale)


class ConstantWeighter:
    def __init__(self, weight):
        self.weight = float(weight)


class PinholeCamera:
    """camera/PinholeCamera.h:35-69 + Intrinsics.h:40-47"""

    def __init__(self, fx, fy, cx, cy, width, height, near_plane=0.05, far_plane=5.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.width, self.height = int(width), int(height)
        self.near_plane, self.far_plane = float(near_plane), float(far_plane)


class ProjectionIntegrator:
    """ProjectionIntegrator.h:43-44, 185-217 (centroids are implicit: the kernel recomputes them)."""

    def __init__(self, truncator=None, weighter=None, carving_dist=0.05, enable_carving=True):
        self.truncator = truncator or InverseTruncator(8.0)
        self.weighter = weighter or ConstantWeighter(1.0)
        self.carving_dist = float(carving_dist)
        self.enable_carving = bool(enable_carving)

    def SetTruncator(self, t):
        self.truncator = t

    def SetWeighter(self, w):
        self.weighter = w

    def SetCarvingDist(self, d):
        self.carving_dist = float(d)

    def SetCarvingEnabled(self, e):
        self.enable_carving = bool(e)

    def _struct(self):
        return Integrator(self.truncator.kind, self.truncator.param, self.weighter.weight, int(self.enable_carving),
                          self.carving_dist)


def _image_pointer(img, np_dtype):
    """-> (address, on_device, keepalive) for a numpy array or a torch tensor."""
    if isinstance(img, np.ndarray):
        a = np.ascontiguousarray(img, dtype=np_dtype)
        return a.ctypes.data, 0, a
    # torch tensor
    t = img.contiguous()
    if t.is_cuda:
        return t.data_ptr(), 1, t
    a = np.ascontiguousarray(t.numpy(), dtype=np_dtype)
    return a.ctypes.data, 0, a


def _pose12(pose):
    p = np.ascontiguousarray(np.asarray(pose, dtype=np.float32)[:3, :4]).reshape(12)
    return (C.c_float * 12)(*p.tolist())


def pack_rays(origins, directions, t_near, t_far):
    """-> (n, 8) float32, one chisel_hip_ray per row: origin, direction, t_near, t_far.  origins (3,) or (n, 3), directions (n, 3),
    t_near / t_far scalars or (n,)"""
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    rays = np.empty((len(d), 8), np.float32)
    rays[:, 0:3] = np.asarray(origins, np.float32)
    rays[:, 3:6] = d
    rays[:, 6] = np.asarray(t_near, np.float32)
    rays[:, 7] = np.asarray(t_far, np.float32)
    return rays


def depth_frame(depth, pose, camera):
    addr, dev, keep = _image_pointer(depth, np.float32)
    H, W = depth.shape[-2], depth.shape[-1]
    f = DepthFrame(addr, W, H, dev, _pose12(pose), camera.fx, camera.fy, camera.cx, camera.cy, camera.near_plane,
                   camera.far_plane)
    return f, keep


def color_frame(color, pose, camera):
    addr, dev, keep = _image_pointer(color, np.uint8)
    shp = tuple(color.shape)
    H, W = shp[0], shp[1]
    ch = 1 if len(shp) == 2 else shp[2]
    f = ColorFrame(addr, W, H, ch, dev, _pose12(pose), camera.fx, camera.fy, camera.cx, camera.cy)
    return f, keep


class PointCloud:
    """chisel::PointCloud (pointcloud/PointCloud.h:33-82): points in the sensor frame and, optionally, one colour per point."""

    def __init__(self, points=None, colors=None):
        self.points = np.zeros((0, 3), np.float32) if points is None else points
        self.colors = colors

    def HasColor(self):
        return self.colors is not None and len(self.colors) > 0

    def GetPoints(self):
        return self.points

    def GetColors(self):
        return self.colors

    def Clear(self):
        self.points = np.zeros((0, 3), np.float32)
        self.colors = None


def marker_light_dir():
    """ChiselServer::FillMarkerTopicWithMeshes' lightDir (chisel_ros/src/ChiselServer.cpp:652-655): (0.8, -0.2, 0.7) normalised twice
    with Eigen's Vector3f::normalize -- v / sqrt(squaredNorm), the sum of squares in order, every step in fp32 -> 3 float32"""
    v = np.array([0.8, -0.2, 0.7], np.float32)
    for _ in range(2):
        sq = v * v
        n2 = np.float32(np.float32(sq[0] + sq[1]) + sq[2])
        v = (v / np.sqrt(n2)).astype(np.float32)
    return tuple(float(x) for x in v)


class Chisel:
    """chisel::Chisel (Chisel.h:38-230) + the ChunkManager queries its callers use."""

    def __init__(self, chunk_size=(16, 16, 16), voxel_resolution=0.03, use_color=False, device_id=-1, max_chunks=0,
                 n_shards=1, shard_rank=0, shard_block=0, devices=None):
        """devices: a list of HIP device ordinals -> one map spread over these GPUs inside this process
        (chisel_hip_create_group: one shard per entry; an ordinal may repeat)."""
        self.L = capi.load_library()
        cs = (chunk_size,) * 3 if isinstance(chunk_size, int) else tuple(int(v) for v in chunk_size)
        self.chunk_size = cs
        self.V = cs[0] * cs[1] * cs[2]
        self.voxel_resolution = float(voxel_resolution)
        self.use_color = bool(use_color)
        cfg = Config((C.c_int * 3)(*cs), float(voxel_resolution), int(use_color), int(device_id), int(max_chunks),
                     int(n_shards), int(shard_rank), int(shard_block))
        self.h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            check(self.L.chisel_hip_create_group(C.byref(cfg), ids, len(devices), C.byref(self.h)))
        else:
            check(self.L.chisel_hip_create(C.byref(cfg), C.byref(self.h)))
        self._integrator = None
        self._keep = []

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.chisel_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Chisel.h ---------------------------------------------------------------------------------
    def _use(self, integrator):
        s = integrator._struct()
        check(self.L.chisel_hip_set_integrator(self.h, C.byref(s)))

    def IntegrateDepthScan(self, integrator, depth_image, extrinsic, camera):
        self._use(integrator)
        f, keep = depth_frame(depth_image, extrinsic, camera)
        check(self.L.chisel_hip_integrate_depth(self.h, C.byref(f)))
        self._keep = [keep]

    def IntegrateDepthScanColor(self, integrator, depth_image, depth_extrinsic, depth_camera, color_image,
                                color_extrinsic, color_camera):
        self._use(integrator)
        f, k1 = depth_frame(depth_image, depth_extrinsic, depth_camera)
        c, k2 = color_frame(color_image, color_extrinsic, color_camera)
        check(self.L.chisel_hip_integrate_depth_color(self.h, C.byref(f), C.byref(c)))
        self._keep = [k1, k2]

    def IntegrateBatch(self, integrator, frames, colors=None):
        """frames: list of (depth, pose, camera); colors: list of (color, pose, camera) or None."""
        self._use(integrator)
        n = len(frames)
        fa = (DepthFrame * n)()
        keep = []
        for i, (d, p, cam) in enumerate(frames):
            fa[i], k = depth_frame(d, p, cam)
            keep.append(k)
        ca = None
        if colors is not None:
            ca = (ColorFrame * n)()
            for i, (c, p, cam) in enumerate(colors):
                ca[i], k = color_frame(c, p, cam)
                keep.append(k)
        check(self.L.chisel_hip_integrate_batch(self.h, n, fa, ca))
        self._keep = keep

    def IntegratePointCloud(self, integrator, cloud, extrinsic, truncation, max_dist):
        """Chisel::IntegratePointCloud (Chisel.h:57, Chisel.cpp:107-157).  `cloud`: a PointCloud, or a tuple (points, colors or None);
        points (n, 3) in the sensor frame, colours (n, 3) in [0, 1]; numpy arrays or torch CUDA tensors."""
        self._use(integrator)
        points, colors = (cloud.points, cloud.colors) if isinstance(cloud, PointCloud) else cloud
        pa, pdev, k1 = _image_pointer(points, np.float32)
        n = int(np.prod(tuple(points.shape))) // 3
        ca, cdev, k2 = (None, pdev, None)
        if colors is not None and int(np.prod(tuple(colors.shape))) > 0:  # PointCloud::HasColor
            ca, cdev, k2 = _image_pointer(colors, np.float32)
            assert int(np.prod(tuple(colors.shape))) // 3 == n, "one colour per point"
        assert cdev == pdev, "points and colours must live in the same memory space"
        pc = capi.PointCloud(pa, ca, n, pdev, _pose12(extrinsic), float(truncation), float(max_dist))
        check(self.L.chisel_hip_integrate_pointcloud(self.h, C.byref(pc)))
        self._keep = [k1, k2]

    def CloudCandidates(self, cloud, extrinsic, truncation, max_dist):
        """ChunkManager::GetChunkIDsIntersecting(cloud, cameraTransform, truncation, maxDist, chunkList) (ChunkManager.cpp:214-257): ids of
        the chunks the cloud's truncated rays pass through, ascending."""
        points, colors = (cloud.points, cloud.colors) if isinstance(cloud, PointCloud) else cloud
        pa, pdev, k1 = _image_pointer(points, np.float32)
        n = int(np.prod(tuple(points.shape))) // 3
        pc = capi.PointCloud(pa, None, n, pdev, _pose12(extrinsic), float(truncation), float(max_dist))
        cnt = C.c_int64(0)
        check(self.L.chisel_hip_cloud_candidates(self.h, C.byref(pc), None, 0, C.byref(cnt)))
        ids = np.zeros((max(1, cnt.value), 3), np.int32)
        check(self.L.chisel_hip_cloud_candidates(self.h, C.byref(pc), ids.ctypes.data_as(C.POINTER(C.c_int)), cnt.value, C.byref(cnt)))
        return ids[:cnt.value]

    def GarbageCollect(self, chunk_ids):
        ids = np.ascontiguousarray(np.asarray(chunk_ids, dtype=np.int32).reshape(-1, 3))
        check(self.L.chisel_hip_garbage_collect(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), len(ids)))

    def UpdateMeshes(self, force=False):
        check(self.L.chisel_hip_update_meshes(self.h, int(force)))

    def Reset(self):
        check(self.L.chisel_hip_reset(self.h))

    # ---- meshing a sharded map with shells (chisel_hip.h "meshing a sharded map with shells") --------------------
    def DirtyIdsDevice(self, out):
        """out: torch int32 CUDA tensor of 1 + 4 * capacity elements -> [n, (x, y, z, flag) * n] (filled on the map's stream: no wait)"""
        check(self.L.chisel_hip_dirty_ids_device(self.h, out.data_ptr(), (out.numel() - 1) // 4))

    def DirtyEntries(self):
        """the same list on the host: (n, 4) int32"""
        import torch
        cap = 1 << 14
        while True:
            buf = torch.zeros((1 + 4 * cap,), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
            torch.cuda.current_stream().synchronize()  # the buffer is zero before the map's stream writes into it
            self.DirtyIdsDevice(buf)
            self.synchronize()
            h = buf.cpu().numpy()
            if h[0] <= cap:
                return h[1:1 + 4 * int(h[0])].reshape(-1, 4).copy()
            cap = 2 * int(h[0])

    # ---- the sharded recompute planned on the device (chisel_hip.h: chisel_hip_shell_plan_device ...) -------------------------------
    def PlanShellsDevice(self, gathered, world, cap):
        """gathered: int32 CUDA tensor, per rank 1 + 4 * cap ints (count, then (x, y, z, flag) entries).  -> dict: jobs (of this shard),
        max_count (largest per-rank count: > cap means entries were cut off and nothing else counts), send / recv: (world, 2) int64 arrays
        of (items, voxels) per peer.  Waits for those figures: the one host wait of a sharded recompute."""
        out = np.zeros(4 + 4 * world, np.int64)
        check(self.L.chisel_hip_shell_plan_device(self.h, gathered.data_ptr(), int(world), int(cap), out.ctypes.data_as(C.POINTER(C.c_int64))))
        self._plan_keep = gathered  # (read by the plan kernels, which the call has waited for; kept for symmetry with the buffers below)
        self._packed_keep = []      # the previous recompute's buffers: its drop kernel ran before the wait above returned
        return {"jobs": int(out[0]), "ghosts_before": int(out[1]), "max_count": int(out[2]), "send_items": int(out[3]),
                "send": out[4:4 + 2 * world].reshape(world, 2).copy(), "recv": out[4 + 2 * world:4 + 4 * world].reshape(world, 2).copy()}

    def ShellSegmentBytes(self, items, voxels):
        return int(self.L.chisel_hip_shell_segment_bytes(self.h, int(items), int(voxels)))

    def ExportShellsPacked(self, out):
        """out: uint8 CUDA tensor of the plan's send size; nothing is waited for (record_event orders the collective)"""
        check(self.L.chisel_hip_export_shells_packed(self.h, out.data_ptr() if out.numel() else None, int(out.numel())))
        self._packed_keep = getattr(self, "_packed_keep", []) + [out]

    def ImportShellsPacked(self, buf):
        """buf: uint8 CUDA tensor holding the received segments (read in place behind wait_event; kept until the next plan)"""
        check(self.L.chisel_hip_import_shells_packed(self.h, buf.data_ptr() if buf.numel() else None, int(buf.numel())))
        self._packed_keep = getattr(self, "_packed_keep", []) + [buf]

    # ---- ... and its wait-free form (chisel_hip.h: chisel_hip_shell_plan_queue ...): every tensor below stays the caller's until ShellCommit
    def PlanShellsQueue(self, gathered, world, cap, stride, status, out, send_items_hint=0):
        """queues the plan, the export of `world` segments of `stride` bytes into `out` (uint8 CUDA tensor) and this rank's status (int32 CUDA
        tensor of SHELL_STATUS_INTS entries); nothing is waited for"""
        check(self.L.chisel_hip_shell_plan_queue(self.h, gathered.data_ptr(), int(world), int(cap), int(stride), status.data_ptr(), out.data_ptr(), int(send_items_hint)))

    def ImportShellsFixed(self, buf, stride, status, jobs_hint=0, items_hint=0):
        """buf: the received segments; status: the ALL-REDUCED status vector (word 0 != 0: nothing below happens on the device)"""
        check(self.L.chisel_hip_import_shells_fixed(self.h, buf.data_ptr(), int(stride), status.data_ptr(), int(jobs_hint), int(items_hint)))

    def ShellCommit(self, aborted):
        check(self.L.chisel_hip_shell_commit(self.h, int(bool(aborted))))

    SHELL_STATUS_INTS = 8

    def UpdateMeshesPlanned(self):
        check(self.L.chisel_hip_update_meshes_planned(self.h))

    def DropGhostChunks(self):
        check(self.L.chisel_hip_drop_ghost_chunks(self.h))

    def UpdateMeshesOf(self, ids):
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 3))
        check(self.L.chisel_hip_update_meshes_of(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), len(ids)))

    def SaveMap(self, filename):
        """binary dump of every resident chunk (chisel_hip_save_map): checkpoint"""
        check(self.L.chisel_hip_save_map(self.h, str(filename).encode()))

    def LoadMap(self, filename):
        """replace the map's contents by a dump written by SaveMap: resume"""
        check(self.L.chisel_hip_load_map(self.h, str(filename).encode()))

    def SaveAllMeshesToPLY(self, filename):
        rc = self.L.chisel_hip_save_ply(self.h, str(filename).encode())
        if rc == 6:
            return False
        check(rc)
        return True

    def GetMeshesToUpdate(self):
        n = C.c_int64(0)
        check(self.L.chisel_hip_meshes_to_update(self.h, None, 0, C.byref(n)))
        ids = np.zeros((n.value, 3), np.int32)
        if n.value:
            check(self.L.chisel_hip_meshes_to_update(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
        return ids

    def PrefetchMeshesToUpdate(self, cursor):
        """chisel_hip_meshes_to_update_prefetch: queue the listing behind the integration just issued (no wait)"""
        check(self.L.chisel_hip_meshes_to_update_prefetch(self.h, cursor))

    def GetMeshesToUpdateSince(self, cursor, capacity=8192):
        """chisel_hip_meshes_to_update_since: (ids that joined the set since `cursor` [n, 3], cleared) -- `cursor` is a (C.c_uint64 * 2)
        the caller keeps (zero before the first call); what the C++ facade's GetMeshesToUpdate is built on"""
        n, cleared = C.c_int64(0), C.c_int(0)
        while True:
            ids = np.zeros((capacity, 3), np.int32)
            check(self.L.chisel_hip_meshes_to_update_since(self.h, cursor, ids.ctypes.data_as(C.POINTER(C.c_int)), capacity, C.byref(n), C.byref(cleared)))
            if n.value <= capacity:
                return ids[:n.value], bool(cleared.value)
            capacity = n.value + 64

    # ---- ChunkManager.h -----------------------------------------------------------------------------
    def synchronize(self):
        check(self.L.chisel_hip_synchronize(self.h))

    def set_stream(self, hip_stream):
        check(self.L.chisel_hip_set_stream(self.h, C.c_void_p(hip_stream)))

    def wait_event(self, hip_event):
        """the device frames of the next Integrate* call are complete behind this hipEvent_t (e.g. torch.cuda.Event.cuda_event)"""
        check(self.L.chisel_hip_wait_event(self.h, C.c_void_p(hip_event)))

    def record_event(self, hip_event):
        """record the hipEvent_t behind everything queued on the map: after it the frames of earlier calls have been read"""
        check(self.L.chisel_hip_record_event(self.h, C.c_void_p(hip_event)))

    def order_stream_after_map(self, hip_stream):
        """whatever the hipStream_t is given next starts after what the map has queued so far (one call, the map's own event)"""
        check(self.L.chisel_hip_order_stream_after_map(self.h, C.c_void_p(hip_stream)))

    def order_map_after_stream(self, hip_stream):
        """the map's next call starts after what the hipStream_t has been given so far"""
        check(self.L.chisel_hip_order_map_after_stream(self.h, C.c_void_p(hip_stream)))

    def NumChunks(self):
        n = C.c_int64(0)
        check(self.L.chisel_hip_num_chunks(self.h, C.byref(n)))
        return n.value

    def GetChunkIDs(self):
        n = C.c_int64(0)
        check(self.L.chisel_hip_list_chunks(self.h, None, 0, C.byref(n)))
        ids = np.zeros((n.value, 3), np.int32)
        if n.value:
            check(self.L.chisel_hip_list_chunks(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
        return ids

    def HasChunk(self, cid):
        cid = (C.c_int * 3)(*[int(v) for v in cid])
        out = C.c_int(0)
        check(self.L.chisel_hip_has_chunk(self.h, cid, C.byref(out)))
        return bool(out.value)

    def GetChunk(self, cid):
        """-> (sdf[V], weight[V], rgbw[V,4] or None); raises KeyError like ChunkMap::at."""
        cid_c = (C.c_int * 3)(*[int(v) for v in cid])
        sdf = np.empty(self.V, np.float32)
        w = np.empty(self.V, np.float32)
        rgbw = np.empty((self.V, 4), np.uint8) if self.use_color else None
        rc = self.L.chisel_hip_download_chunk(self.h, cid_c, sdf.ctypes.data_as(C.POINTER(C.c_float)),
                                              w.ctypes.data_as(C.POINTER(C.c_float)),
                                              rgbw.ctypes.data_as(C.POINTER(C.c_uint8)) if rgbw is not None else None)
        if rc == 4:
            raise KeyError(tuple(int(v) for v in cid))
        check(rc)
        return sdf, w, rgbw

    def AddChunk(self, cid, sdf, weight, rgbw=None):
        cid_c = (C.c_int * 3)(*[int(v) for v in cid])
        s = np.ascontiguousarray(sdf, np.float32)
        w = np.ascontiguousarray(weight, np.float32)
        c = np.ascontiguousarray(rgbw, np.uint8) if rgbw is not None else None
        check(self.L.chisel_hip_upload_chunk(self.h, cid_c, s.ctypes.data_as(C.POINTER(C.c_float)),
                                             w.ctypes.data_as(C.POINTER(C.c_float)),
                                             c.ctypes.data_as(C.POINTER(C.c_uint8)) if c is not None else None))

    def fields(self):
        return {tuple(int(v) for v in cid): self.GetChunk(cid) for cid in self.GetChunkIDs()}

    def GetMeshIDs(self):
        n = C.c_int64(0)
        check(self.L.chisel_hip_list_meshes(self.h, None, 0, C.byref(n)))
        ids = np.zeros((n.value, 3), np.int32)
        if n.value:
            check(self.L.chisel_hip_list_meshes(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
        return ids

    def GetMesh(self, cid):
        cid_c = (C.c_int * 3)(*[int(v) for v in cid])
        nv, ng = C.c_int64(0), C.c_int64(0)
        rc = self.L.chisel_hip_mesh_size(self.h, cid_c, C.byref(nv), C.byref(ng))
        if rc == 4:
            raise KeyError(tuple(int(v) for v in cid))
        check(rc)
        v = np.zeros((nv.value, 3), np.float32)
        n = np.zeros((nv.value, 3), np.float32)
        c = np.zeros((nv.value, 3), np.float32) if self.use_color else None
        g = np.zeros((ng.value, 3), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        check(self.L.chisel_hip_download_mesh(self.h, cid_c, fp(v), fp(n), fp(c), fp(g)))
        return {"vertices": v, "normals": n, "colors": c, "grids": g}

    def GetSDF(self, pos):
        p = (C.c_float * 3)(*[float(v) for v in pos])
        d, found = C.c_double(0), C.c_int(0)
        check(self.L.chisel_hip_get_sdf(self.h, p, C.byref(d), C.byref(found)))
        return bool(found.value), d.value

    def GetSDFAndGradient(self, pos):
        p = (C.c_float * 3)(*[float(v) for v in pos])
        g = (C.c_float * 3)()
        d, found = C.c_double(0), C.c_int(0)
        check(self.L.chisel_hip_get_sdf_and_gradient(self.h, p, C.byref(d), g, C.byref(found)))
        return bool(found.value), d.value, np.array(list(g), np.float32)

    def RenderView(self, extrinsic, camera, step=0.0, normals=False, colors=False, out=None):
        """chisel_hip_render_view: what the map holds as `camera` at the camera->world pose `extrinsic` sees it (the pair
        IntegrateDepthScan takes); step: z-distance between two samples of a ray, <= 0 = the voxel resolution.
        -> {"depth": (H, W), "normals": (H, W, 3) or None, "colors": (H, W, 3) or None}, float32 numpy arrays with NaN where
        the ray hits nothing.  `out`: a dict of float32 torch CUDA tensors of those shapes ("depth" required) to fill in place on
        the map's stream, nothing waited for; it is returned."""
        H, W = camera.height, camera.width
        v = capi.View(W, H, _pose12(extrinsic), camera.fx, camera.fy, camera.cx, camera.cy, camera.near_plane, camera.far_plane,
                      float(step))
        if out is not None:
            import torch
            for name, t in out.items():
                want = (H, W) if name == "depth" else (H, W, 3)
                assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want), \
                    "out[%r]: a contiguous float32 CUDA tensor of shape %s" % (name, want)
            ptr = lambda t: t.data_ptr() if t is not None else None
            check(self.L.chisel_hip_render_view(self.h, C.byref(v), ptr(out["depth"]), ptr(out.get("normals")), ptr(out.get("colors")), 1))
            self._keep = [out]
            return out
        res = {"depth": np.empty((H, W), np.float32), "normals": np.empty((H, W, 3), np.float32) if normals else None,
               "colors": np.empty((H, W, 3), np.float32) if colors else None}
        ptr = lambda a: a.ctypes.data if a is not None else None
        check(self.L.chisel_hip_render_view(self.h, C.byref(v), ptr(res["depth"]), ptr(res["normals"]), ptr(res["colors"]), 0))
        return res

    _POINT_OUTPUTS = (("found", np.uint8, ()), ("sdf", np.float32, ()), ("weight", np.float32, ()), ("gradient", np.float32, (3,)),
                      ("colors", np.float32, (3,)))
    _RAY_OUTPUTS = (("t_hit", np.float32, ()), ("status", np.uint8, ()), ("normals", np.float32, (3,)), ("colors", np.float32, (3,)))

    @staticmethod
    def _device_outputs(out, spec, n):
        """addresses of the tensors of `out` in the order of `spec` (None where a name is missing), each checked"""
        import torch
        unknown = set(out) - {name for name, _, _ in spec}
        assert not unknown, "out: unknown outputs %s" % sorted(unknown)
        ptrs = []
        for name, dtype, tail in spec:
            t = out.get(name)
            want = torch.uint8 if dtype is np.uint8 else torch.float32
            assert t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == (n,) + tail), \
                "out[%r]: a contiguous %s CUDA tensor of shape %s" % (name, want, (n,) + tail)
            ptrs.append(t.data_ptr() if t is not None else None)
        return ptrs

    def QueryPoints(self, positions, sdf=True, weight=False, gradient=False, colors=False, out=None):
        """chisel_hip_query_points: the map at the n positions (n, 3) in one launch.  -> {"found": (n,) uint8 -- bit 0 GetSDF(p) true,
        bit 1 GetSDFAndGradient(p) true (only with gradient) --, "sdf": (n,), "weight": (n,), "gradient": (n, 3), "colors": (n, 3)}:
        numpy arrays, float32 but for "found", None for what was not asked for; NaN where the map has no answer.
        `out`: a dict of contiguous torch CUDA tensors of those shapes, with `positions` a contiguous float32 CUDA tensor that is
        complete on the map's stream: exactly the outputs named in it are filled in place on the map's stream, nothing is waited
        for; it is returned."""
        if out is not None:
            import torch
            assert positions.is_cuda and positions.dtype == torch.float32 and positions.is_contiguous() and positions.dim() == 2 and \
                positions.shape[1] == 3, "positions: a contiguous float32 CUDA tensor of shape (n, 3)"
            n = int(positions.shape[0])
            ptrs = self._device_outputs(out, self._POINT_OUTPUTS, n)
            if n:  # (an empty tensor has no address)
                check(self.L.chisel_hip_query_points(self.h, positions.data_ptr(), n, *ptrs, 1))
            self._keep = [positions, out]
            return out
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = len(p)
        asked = {"found": True, "sdf": sdf, "weight": weight, "gradient": gradient, "colors": colors}
        res = {name: (np.empty((n,) + tail, dtype) if asked[name] else None) for name, dtype, tail in self._POINT_OUTPUTS}
        ptr = lambda a: a.ctypes.data if a is not None else None
        check(self.L.chisel_hip_query_points(self.h, ptr(p), n, *[ptr(res[name]) for name, _, _ in self._POINT_OUTPUTS], 0))
        return res

    def CastRays(self, origins, directions, t_near, t_far, step=0.0, status=True, normals=False, colors=False, out=None):
        """chisel_hip_cast_rays: RenderView's march along n rays of the caller's own.  origins, directions: (n, 3) (an origin of
        shape (3,) serves every ray); t_near, t_far: scalars or (n,); the samples are origin + t direction for t = t_near + k step,
        the direction as given (unit directions: t is Euclidean range); step <= 0 = the voxel resolution.
        -> {"t_hit": (n,) float32, NaN without a hit, "status": (n,) uint8 -- 1 hit, 2 the ray came up behind a surface, 0 it never
        ended --, "normals": (n, 3), "colors": (n, 3)}, None for what was not asked for.
        `out`: a dict of contiguous torch CUDA tensors of those shapes ("t_hit" required), with origins, directions (and t_near,
        t_far, where they are not scalars) float32 CUDA tensors: the rays are packed on torch's current stream, the map's stream is
        ordered behind it (and torch's stream behind the kernel, which reads a buffer of this call's own), the outputs named in
        `out` are filled in place and nothing is waited for by the host; `out` is returned.  Rays
        that are packed already -- a (n, 8) tensor origin, direction, t_near, t_far per row -- go in as `origins` with
        directions None."""
        if out is not None:
            import torch
            if directions is None:
                rays = origins
            else:
                n = int(directions.shape[0])
                rays = torch.empty((n, 8), dtype=torch.float32, device=directions.device)
                rays[:, 0:3] = origins
                rays[:, 3:6] = directions
                rays[:, 6] = t_near
                rays[:, 7] = t_far
            assert rays.is_cuda and rays.dtype == torch.float32 and rays.is_contiguous() and rays.dim() == 2 and rays.shape[1] == 8, \
                "packed rays: a contiguous float32 CUDA tensor of shape (n, 8)"
            n = int(rays.shape[0])
            ptrs = self._device_outputs(out, self._RAY_OUTPUTS, n)
            assert out.get("t_hit") is not None, "out['t_hit'] is required"
            if n:
                if directions is not None:  # (packed just now, on torch's stream)
                    self.order_map_after_stream(torch.cuda.current_stream().cuda_stream)
                check(self.L.chisel_hip_cast_rays(self.h, rays.data_ptr(), n, float(step), *ptrs, 1))
                if directions is not None:
                    # the packed rays are this call's own: when the tensor is released its block goes back to torch's stream, so that
                    # stream is ordered behind the kernel that reads it (the caller's own tensors are the caller's to keep)
                    self.order_stream_after_map(torch.cuda.current_stream().cuda_stream)
            self._keep = [rays, out]
            return out
        rays = pack_rays(origins, directions, t_near, t_far)
        n = len(rays)
        asked = {"t_hit": True, "status": status, "normals": normals, "colors": colors}
        res = {name: (np.empty((n,) + tail, dtype) if asked[name] else None) for name, dtype, tail in self._RAY_OUTPUTS}
        ptr = lambda a: a.ctypes.data if a is not None else None
        check(self.L.chisel_hip_cast_rays(self.h, ptr(rays), n, float(step), *[ptr(res[name]) for name, _, _ in self._RAY_OUTPUTS], 0))
        return res

    _DISTANCE_OUTPUTS = (("state", np.uint8), ("dist2", np.int32), ("distance", np.float32))

    def DistanceWindow(self, lo_m, hi_m):
        """(origin, dims) of the voxels whose centres ((g + 0.5) res per axis, g the global voxel index) lie in the closed metric box
        lo_m ... hi_m: what DistanceField takes.  Computed in float64; a box that holds no centre on some axis gives a dim below 1."""
        res = float(np.float32(self.voxel_resolution))
        lo = np.ceil(np.asarray(lo_m, np.float64) / res - 0.5).astype(np.int64)
        hi = np.floor(np.asarray(hi_m, np.float64) / res - 0.5).astype(np.int64)
        return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)

    def DistanceField(self, origin, dims, radius, unknown_is_obstacle=False, surface_offset=0.0, state=True, dist2=True, distance=False, out=None):
        """chisel_hip_distance_field: over the window of dims = (nx, ny, nz) voxels whose first voxel has the global index `origin`
        (chunk id * N + voxel coordinate per axis), the truncated exact Euclidean distance transform of DESIGN.md 3.11.
        -> {"state": uint8 -- 0 unknown, 1 free, 2 occupied (observed with sdf < surface_offset) --, "dist2": int32, the squared
        distance in voxels to the nearest obstacle of the map within `radius` (1 ... 64), -1 without one, "distance": float32, metres,
        +inf without one}: numpy arrays of shape (nz, ny, nx), None for what was not asked for.  Obstacles are the occupied voxels,
        with unknown_is_obstacle the unknown ones too.
        `out`: a dict of contiguous torch CUDA tensors of that shape and those types: exactly the outputs named in it are filled in
        place on the map's stream, nothing is waited for; it is returned."""
        w = capi.DistanceWindow()
        w.origin[:] = [int(v) for v in origin]
        w.dims[:] = [int(v) for v in dims]
        w.radius, w.unknown_is_obstacle, w.surface_offset = int(radius), int(bool(unknown_is_obstacle)), float(surface_offset)
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        if out is not None:
            import torch
            unknown = set(out) - {name for name, _ in self._DISTANCE_OUTPUTS}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            ptrs = []
            for name, dtype in self._DISTANCE_OUTPUTS:
                t = out.get(name)
                want = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}[dtype]
                assert t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == shape), \
                    "out[%r]: a contiguous %s CUDA tensor of shape %s" % (name, want, shape)
                ptrs.append(t.data_ptr() if t is not None and t.numel() else None)
            check(self.L.chisel_hip_distance_field(self.h, C.byref(w), *ptrs, 1))
            self._keep = [out]
            return out
        asked = {"state": state, "dist2": dist2, "distance": distance}
        ok = all(d >= 1 for d in shape) and shape[0] * shape[1] * shape[2] <= 1 << 30  # (a window the library refuses by its size allocates nothing here either)
        res = {name: (np.empty(shape if ok else (0, 0, 0), dtype) if asked[name] else None) for name, dtype in self._DISTANCE_OUTPUTS}
        ptr = lambda a: a.ctypes.data if a is not None else None
        check(self.L.chisel_hip_distance_field(self.h, C.byref(w), *[ptr(res[name]) for name, _ in self._DISTANCE_OUTPUTS], 0))
        return res

    def _frontier_window(self, origin, dims, min_unknown_faces, connectivity, min_voxels, surface_offset):
        w = capi.FrontierWindow()
        w.origin[:] = [int(v) for v in origin]
        w.dims[:] = [int(v) for v in dims]
        w.min_unknown_faces, w.connectivity, w.surface_offset = int(min_unknown_faces), int(connectivity), float(surface_offset)
        w.min_voxels = max(min(int(min_voxels), (1 << 31) - 1), -1)  # (no cluster has 2^31 - 1 voxels: none is kept)
        return w

    def _frontier_call(self, w, state, label, capacity_voxels, voxels, capacity_clusters, table, on_device):
        """chisel_hip_frontiers -> the totals; a refused capacity raises with the totals in the error's `totals`"""
        totals = capi.FrontierTotals()
        rc = self.L.chisel_hip_frontiers(self.h, C.byref(w), state, label, int(capacity_voxels), voxels, int(capacity_clusters),
                                         self._table_ptr(table, C.c_int64), int(on_device), C.byref(totals))
        if rc:
            try:
                check(rc)
            except capi.ChiselHipError as e:
                e.totals = self._totals_dict(totals)
                raise
        return self._totals_dict(totals)

    def FrontiersSize(self, origin, dims, min_unknown_faces=1, connectivity=26, min_voxels=1, surface_offset=0.0):
        """chisel_hip_frontiers as the size query: the totals of Frontiers -- {"unknown", "free", "occupied", "frontier", "clusters",
        "largest_voxels", "kept_clusters", "kept_voxels"} -- with nothing else written"""
        w = self._frontier_window(origin, dims, min_unknown_faces, connectivity, min_voxels, surface_offset)
        return self._frontier_call(w, None, None, 0, None, 0, None, 0)

    def FrontierCentres(self, origin, table):
        """the centres of the clusters of a Frontiers table, (K, 3) float64 metres: ((origin + sum / voxels) + 0.5) * resolution"""
        table = np.asarray(table, np.int64).reshape(-1, 12)
        res = float(np.float32(self.voxel_resolution))
        mean = table[:, 2:5].astype(np.float64) / np.maximum(table[:, 1:2], 1).astype(np.float64)
        return ((np.asarray(origin, np.float64)[None, :] + mean) + 0.5) * res

    def Frontiers(self, origin, dims, min_unknown_faces=1, connectivity=26, min_voxels=1, surface_offset=0.0, state=False, label=True, voxels=True, out=None):
        """chisel_hip_frontiers: over the window of dims = (nx, ny, nz) voxels whose first voxel has the global index
        `origin`, the FRONTIER voxels -- free, with at least min_unknown_faces (1 ... 6) of the six face neighbours unknown; states as
        DistanceField's, neighbours read from the map beyond the window's rim too --, their clusters under `connectivity` 6, 18 or 26
        inside the window, numbered by ascending smallest linear index, and of those the ones with at least min_voxels voxels.
        -> {"state": uint8 (nz, ny, nx), "label": int32 (nz, ny, nx) -- the kept cluster's number, -1 not a frontier voxel, -2 a
        frontier voxel of a dropped cluster --, "voxels": int32 (kept voxels, 4) -- x, y, z (window-relative), cluster, in ascending
        linear index --, None for what was not asked for; "table": int64 (K, 12) -- capi.FRONTIER_TABLE_COLUMNS: root, voxels, the
        sums, minima and maxima of x, y, z, the sum of unknown faces --, "centres": float64 (K, 3) metres, "totals"}.
        `out`: a dict of contiguous torch CUDA tensors "state", "label" (of that shape) and / or "voxels" ((rows, 4) int32 with at
        least kept_voxels rows): exactly those are filled in place on the map's stream; it is returned with "table", "centres" and
        "totals" (host) added.  The sizes come from a size query in front of the call; the map is only read."""
        w = self._frontier_window(origin, dims, min_unknown_faces, connectivity, min_voxels, surface_offset)
        size = self._frontier_call(w, None, None, 0, None, 0, None, 0)
        K, kept = size["kept_clusters"], size["kept_voxels"]
        table = np.zeros((K, 12), np.int64)
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        if out is not None:
            import torch
            unknown = set(out) - {"state", "label", "voxels"}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            ptrs = []
            for name, want in (("state", torch.uint8), ("label", torch.int32)):
                t = out.get(name)
                assert t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == shape), \
                    "out[%r]: a contiguous %s CUDA tensor of shape %s" % (name, want, shape)
                ptrs.append(t.data_ptr() if t is not None else None)
            rows = out.get("voxels")
            cap = int(rows.shape[0]) if rows is not None else 0
            self._device_rows(rows, "out['voxels']", "int32", 4, 0)  # (kind and shape; the rows are the capacity)
            list_ptr = rows.data_ptr() if rows is not None and rows.numel() else None
            totals = self._frontier_call(w, ptrs[0], ptrs[1], cap if list_ptr else 0, list_ptr, K, table, 1)
            self._keep = [out]
            res = dict(out)
        else:
            res = {"state": np.empty(shape, np.uint8) if state else None, "label": np.empty(shape, np.int32) if label else None,
                   "voxels": np.empty((kept, 4), np.int32) if voxels else None}
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None
            totals = self._frontier_call(w, ptr(res["state"]), ptr(res["label"]), kept if voxels else 0, ptr(res["voxels"]), K, table, 0)
        assert totals == size, "the map changed between the size query and the call"
        res.update(table=table, centres=self.FrontierCentres(origin, table), totals=totals)
        return res

    def TravelField(self, origin, dims, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30, clearance=0, unknown_is_obstacle=False,
                    surface_offset=0.0, cost=True, step=True, state=False, targets=None, n_groups=0, out=None):
        """chisel_hip_travel_field: over the window of dims = (nx, ny, nz) voxels whose first voxel has the global index
        `origin`, the least travel cost from the `seeds` ((n, 3) window-relative x, y, z) to every TRAVERSABLE voxel -- free, and with
        clearance r >= 1 no obstacle of the map within r voxels (DistanceField's dist2 == -1 at radius r) -- over the moves of
        `connectivity` 6, 18 or 26, a move with k non-zero coordinates costing step_cost[k - 1], up to max_cost.
        -> {"cost": int32 (nz, ny, nx), -1 unreached; "step": uint8, 13 at a seed, 255 unreached, else the smallest code
        (dz + 1) 9 + (dy + 1) 3 + (dx + 1) of a move that leads back towards a seed; "state": uint8, DistanceField's; None for what was
        not asked for; "table": int64 (n_groups, 4) -- capi.TRAVEL_TABLE_COLUMNS: rows, reached rows, least cost, the smallest linear
        index with it, -1 without a reached row -- when `targets` ((n, 4) int32 x, y, z, group: the "voxels" of Frontiers; a numpy
        array or a torch CUDA tensor) are given, else None; "totals": capi.TRAVEL_TOTALS, "rounds" and "tile_visits" diagnostics}.
        `out`: a dict of contiguous torch CUDA tensors "cost", "step", "state" of that shape: exactly those are filled in place on the
        map's stream; it is returned with "table" and "totals" (host) added; numpy targets are uploaded first.  The map is only read."""
        w = capi.TravelWindow()
        w.origin[:] = [int(v) for v in origin]
        w.dims[:] = [int(v) for v in dims]
        w.step_cost[:] = [int(v) for v in step_cost]
        w.connectivity, w.max_cost, w.clearance = int(connectivity), int(max_cost), int(clearance)
        w.unknown_is_obstacle, w.surface_offset = int(bool(unknown_is_obstacle)), float(surface_offset)
        seeds = np.ascontiguousarray(np.asarray(seeds, np.int32).reshape(-1, 3))
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        on_device = out is not None
        is_tensor = targets is not None and not isinstance(targets, np.ndarray) and hasattr(targets, "data_ptr")
        if is_tensor:
            self._device_rows(targets, "targets", "int32", 4, 0)
            n_targets = int(targets.shape[0])
            if not on_device:
                targets = targets.cpu().numpy()
                is_tensor = False
        if targets is not None and not is_tensor:
            targets = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(-1, 4))
            n_targets = int(targets.shape[0])
            if on_device:
                import torch
                targets = torch.from_numpy(targets).cuda()
                is_tensor = True
        if targets is None:
            n_targets = 0
        target_ptr = None
        if n_targets:
            target_ptr = targets.data_ptr() if is_tensor else targets.ctypes.data
        table = np.zeros((int(n_groups), 4), np.int64) if n_targets else None
        if on_device:
            import torch
            unknown = set(out) - {"cost", "step", "state"}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            ptrs = []
            for name, want in (("cost", torch.int32), ("step", torch.uint8), ("state", torch.uint8)):
                t = out.get(name)
                assert t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == shape), \
                    "out[%r]: a contiguous %s CUDA tensor of shape %s" % (name, want, shape)
                ptrs.append(t.data_ptr() if t is not None else None)
            self._keep = [out, targets]
            res = dict(out)
        else:
            res = {"cost": np.empty(shape, np.int32) if cost else None, "step": np.empty(shape, np.uint8) if step else None,
                   "state": np.empty(shape, np.uint8) if state else None}
            ptrs = [res[k].ctypes.data if res[k] is not None and res[k].size else None for k in ("cost", "step", "state")]
        totals = capi.TravelTotals()
        check(self.L.chisel_hip_travel_field(self.h, C.byref(w), seeds.ctypes.data_as(C.POINTER(C.c_int32)) if seeds.size else None, int(seeds.shape[0]),
                                             target_ptr, n_targets, int(n_groups), ptrs[0], ptrs[1], ptrs[2], self._table_ptr(table, C.c_int64),
                                             int(on_device), C.byref(totals)))
        res.update(table=table, totals=self._totals_dict(totals))
        return res

    def TravelPath(self, step, start):
        """chisel_hip_travel_path: the walk along the steps of TravelField (a numpy array or a torch tensor (nz, ny, nx) uint8) from
        the voxel `start` (x, y, z window-relative) to its seed -> (n, 3) int32 rows (x, y, z), both ends included"""
        if not isinstance(step, np.ndarray) and hasattr(step, "cpu"):
            step = step.cpu().numpy()
        step = np.ascontiguousarray(step, np.uint8)
        assert step.ndim == 3, "step: (nz, ny, nx)"
        dims = (C.c_int32 * 3)(step.shape[2], step.shape[1], step.shape[0])
        start = (C.c_int32 * 3)(*[int(v) for v in start])
        length = C.c_int64(0)
        path = np.empty((1, 3), np.int32)
        rc = self.L.chisel_hip_travel_path(step.ctypes.data, dims, start, 1, path.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(length))
        if rc and length.value > 1:  # (the capacity was short: the length is known now)
            path = np.empty((length.value, 3), np.int32)
            rc = self.L.chisel_hip_travel_path(step.ctypes.data, dims, start, length.value, path.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(length))
        check(rc)
        return path[:length.value]

    _GATHER_OUTPUTS = (("vertices", 3), ("normals", 3), ("colors", 3), ("rgba", 4), ("grids", 3))
    # ChiselServer's marker lights (chisel_ros/src/ChiselServer.cpp:652-655, :657-658): lightDir normalised twice, lightDir1 as it stands
    MARKER_LIGHTS = {"light0": marker_light_dir(), "light1": (-0.5, 0.2, 0.2), "diffuse": 0.5, "ambient": 0.2}

    def _mesh_request(self, ids, lights):
        """-> (chisel_hip_mesh_request, what it points at)"""
        req = capi.MeshRequest()
        keep = None
        if ids is not None:
            keep = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 3))
            req.ids_xyz = keep.ctypes.data_as(C.POINTER(C.c_int))
            req.n_ids = len(keep)
        if lights is not None:
            req.marker_colors = 1
            req.light0[:] = [float(v) for v in lights["light0"]]
            req.light1[:] = [float(v) for v in lights["light1"]]
            req.diffuse, req.ambient = float(lights["diffuse"]), float(lights["ambient"])
        return req, keep

    @staticmethod
    def _totals_dict(t):
        return {name: int(getattr(t, name)) for name, _ in t._fields_}

    def GatherMeshesSize(self, ids=None, lights=None):
        """chisel_hip_gather_meshes_size: the totals of a selection (GatherMeshes) without a launch -> {"meshes", "meshes_nonempty",
        "vertices", "grids", "arenas_read", "tiles"}"""
        req, keep = self._mesh_request(ids, lights)
        t = capi.MeshTotals()
        rc = self.L.chisel_hip_gather_meshes_size(self.h, C.byref(req), C.byref(t))
        if rc == 4:
            raise KeyError(self.L.chisel_hip_last_error().decode(errors="replace"))
        check(rc)
        return self._totals_dict(t)

    def GatherMeshes(self, ids=None, normals=True, colors=None, rgba=False, grids=True, lights=None, out=None):
        """chisel_hip_gather_meshes: the chunk meshes of `ids` ((n, 3), in that order, duplicates allowed; None: every mesh in
        GetMeshIDs' order) packed into contiguous arrays by one launch.  -> {"vertices": (V, 3), "normals": (V, 3), "colors":
        (V, 3), "rgba": (V, 4), "grids": (G, 3)} float32 numpy arrays, None for what was not asked for (colors=None: asked for iff
        the map holds colour), plus "table": (n, 4) int64 -- first vertex, vertices, first grid, grids of every mesh --, "ids":
        (n, 3) int32 and "totals".  Every float is the one GetMesh returns for that chunk.  rgba: FillMarkerTopicWithMeshes'
        colours with `lights` (None: Chisel.MARKER_LIGHTS, ChiselServer's own).
        `out`: a dict of contiguous torch CUDA float32 tensors of shape (rows, 3) -- (rows, 4) for "rgba" -- with at least V
        ("grids": G) rows: exactly the outputs named in it are filled in place on the map's stream, nothing is waited for; it is
        returned with "table", "ids" and "totals" (numpy, host) added.  KeyError for an id without a mesh."""
        want_rgba = rgba or (out is not None and "rgba" in out)
        req, keep = self._mesh_request(ids, (lights if lights is not None else self.MARKER_LIGHTS) if want_rgba else None)
        t = capi.MeshTotals()

        def call(cap_v, cap_g, ptrs, on_device, table, ids_out):
            rc = self.L.chisel_hip_gather_meshes(self.h, C.byref(req), cap_v, cap_g, *ptrs, on_device,
                                                 table.ctypes.data_as(C.POINTER(C.c_int64)) if table is not None else None,
                                                 ids_out.ctypes.data_as(C.POINTER(C.c_int)) if ids_out is not None else None, C.byref(t))
            if rc == 4:
                raise KeyError(self.L.chisel_hip_last_error().decode(errors="replace"))
            check(rc)

        size = self.GatherMeshesSize(ids)
        n, V, G = size["meshes"], size["vertices"], size["grids"]
        table, ids_out = np.zeros((n, 4), np.int64), np.zeros((n, 3), np.int32)
        if out is not None:
            import torch
            unknown = set(out) - {name for name, _ in self._GATHER_OUTPUTS}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            assert out, "out: no output named"
            ptrs, cap_v, cap_g = [], None, None
            for name, width in self._GATHER_OUTPUTS:
                tns = out.get(name)
                assert tns is None or (tns.is_cuda and tns.dtype == torch.float32 and tns.is_contiguous() and tns.dim() == 2 and tns.shape[1] == width), \
                    "out[%r]: a contiguous float32 CUDA tensor of shape (rows, %d)" % (name, width)
                if tns is not None:
                    rows = int(tns.shape[0])
                    if name == "grids":
                        cap_g = rows
                    else:
                        cap_v = rows if cap_v is None else min(cap_v, rows)
                # (an empty tensor has no address: it stands for its array only when there is nothing to write)
                ptrs.append(tns.data_ptr() if tns is not None and tns.numel() else None)
            if all(p is None for p in ptrs):
                assert V <= (cap_v if cap_v is not None else V) and G <= (cap_g if cap_g is not None else G), "out: tensors without room"
                res = dict(out)
                res.update(table=table, ids=ids_out, totals=size)
                return res
            call(cap_v if cap_v is not None else V, cap_g if cap_g is not None else G, ptrs, 1, table, ids_out)
            self._keep = [out]
            res = dict(out)
            res.update(table=table, ids=ids_out, totals=self._totals_dict(t))
            return res
        if colors is None:
            colors = self.use_color
        asked = {"vertices": True, "normals": normals, "colors": colors, "rgba": rgba, "grids": grids}
        res = {name: (np.empty((G if name == "grids" else V, width), np.float32) if asked[name] else None) for name, width in self._GATHER_OUTPUTS}
        # (an array without rows has nothing to receive: the library is told of the others)
        ptrs = [res[name].ctypes.data if res[name] is not None and res[name].size else None for name, _ in self._GATHER_OUTPUTS]
        if any(p is not None for p in ptrs):
            call(V, G, ptrs, 0, table, ids_out)
            size = self._totals_dict(t)
        res.update(table=table, ids=ids_out, totals=size)
        return res

    def SaveAllMeshesToPLYBinary(self, filename):
        """chisel_hip_save_ply_binary: SaveAllMeshesToPLY's elements, properties and vertex order as binary_little_endian 1.0"""
        rc = self.L.chisel_hip_save_ply_binary(self.h, str(filename).encode())
        if rc == 6:
            return False
        check(rc)
        return True

    _CHUNK_ARRAYS = (("sdf", np.float32, ()), ("weight", np.float32, ()), ("rgbw", np.uint8, (4,)))

    def _chunk_request(self, ids, box):
        """-> (chisel_hip_chunk_request, what it points at)"""
        req = capi.ChunkRequest()
        keep = None
        if ids is not None:
            keep = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 3))
            req.ids_xyz = keep.ctypes.data_as(C.POINTER(C.c_int))
            req.n_ids = len(keep)
        if box is not None:
            req.use_box = 1
            req.box_lo[:] = [int(v) for v in box[0]]
            req.box_hi[:] = [int(v) for v in box[1]]
        return req, keep

    def _gather_chunks_call(self, req, capacity, ptrs, on_device, ids_out, retry=False):
        """-> the number of chunks of the selection; with `retry`, minus that number - 1 when the capacity was below it (nothing written)"""
        n = C.c_int64(-1)
        rc = self.L.chisel_hip_gather_chunks(self.h, C.byref(req), capacity, *ptrs, on_device,
                                             ids_out.ctypes.data_as(C.POINTER(C.c_int)) if ids_out is not None and ids_out.size else None, C.byref(n))
        if rc == 4:
            raise KeyError(self.L.chisel_hip_last_error().decode(errors="replace"))
        if retry and rc == 1 and n.value > capacity:
            return -n.value - 1
        check(rc)
        return n.value

    def GatherChunksSize(self, ids=None, box=None):
        """chisel_hip_gather_chunks with a capacity of 0: the number of chunks of a selection (GatherChunks)"""
        req, keep = self._chunk_request(ids, box)
        return self._gather_chunks_call(req, 0, [None, None, None], 0, None)

    def GatherChunks(self, ids=None, box=None, sdf=True, weight=True, rgbw=None, out=None):
        """chisel_hip_gather_chunks: the voxels of the chunks `ids` ((n, 3), in that order, duplicates allowed; None: every resident
        chunk in GetChunkIDs' order, with box=(lo, hi) those with lo <= id <= hi on every axis) packed by one launch.  ->
        {"sdf": (n, V), "weight": (n, V), "rgbw": (n, V, 4)} numpy arrays, float32 / uint8, None for what was not asked for
        (rgbw=None: asked for iff the map holds colour), plus "ids": (n, 3) int32.  Every value is the one GetChunk returns.
        `out`: a dict of contiguous torch CUDA tensors of those shapes with at least n rows (16-byte aligned): exactly the arrays
        named in it are filled in place on the map's stream, nothing is waited for; it is returned with "ids" (numpy, host)
        added.  KeyError for a listed id that is not resident."""
        req, keep = self._chunk_request(ids, box)
        if out is not None:
            import torch
            unknown = set(out) - {name for name, _, _ in self._CHUNK_ARRAYS}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            assert out, "out: no output named"
            ptrs, cap = [], None
            for name, dtype, tail in self._CHUNK_ARRAYS:
                t = out.get(name)
                want = torch.uint8 if dtype is np.uint8 else torch.float32
                assert t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape[1:]) == (self.V,) + tail), \
                    "out[%r]: a contiguous %s CUDA tensor of shape (rows, %d%s)" % (name, want, self.V, ", 4" if tail else "")
                if t is not None:
                    cap = int(t.shape[0]) if cap is None else min(cap, int(t.shape[0]))
                ptrs.append(t.data_ptr() if t is not None and t.numel() else None)
            if cap and any(p is not None for p in ptrs):  # one call: the selection is made once (a capacity below it is refused)
                ids_out = np.zeros((cap, 3), np.int32)
                ids_out = ids_out[:self._gather_chunks_call(req, cap, ptrs, 1, ids_out)]
            else:  # (an empty tensor has no address: it stands for its array only when there is nothing to write)
                assert self._gather_chunks_call(req, 0, [None, None, None], 0, None) == 0, "out: tensors without room"
                ids_out = np.zeros((0, 3), np.int32)
            self._keep = [out]
            res = dict(out)
            res["ids"] = ids_out
            return res
        if rgbw is None:
            rgbw = self.use_color
        asked = {"sdf": sdf, "weight": weight, "rgbw": rgbw}
        # one call makes the selection once: room for the list as given, for every resident chunk otherwise (a box: its size is asked
        # first, it may hold a small part of the map); a capacity that turns out too small is refused with the count, and tried again
        cap = len(keep) if keep is not None else (self._gather_chunks_call(req, 0, [None, None, None], 0, None) if box is not None else self.NumChunks())
        while True:
            res = {name: (np.empty((cap, self.V) + tail, dtype) if asked[name] else None) for name, dtype, tail in self._CHUNK_ARRAYS}
            ids_out = np.zeros((cap, 3), np.int32)
            n = 0
            if cap:
                n = self._gather_chunks_call(req, cap, [res[name].ctypes.data if res[name] is not None else None for name, _, _ in self._CHUNK_ARRAYS], 0, ids_out, retry=True)
            else:
                n = -self._gather_chunks_call(req, 0, [None, None, None], 0, None) - 1
                n = 0 if n == -1 else n
            if n >= 0:
                break
            cap = -n - 1
        res = {name: (a[:n] if a is not None else None) for name, a in res.items()}
        res["ids"] = ids_out[:n]
        return res

    def ScatterChunks(self, ids, sdf, weight, rgbw=None, mark_updated=False):
        """chisel_hip_scatter_chunks: the packed chunks `ids` (n, 3), sdf (n, V), weight (n, V), rgbw (n, V, 4) or None (zeros on a map
        with colour) into the map -- what AddChunk per chunk leaves, by one classify, one create and one copy launch.  numpy arrays,
        or contiguous torch CUDA tensors that are complete on the map's stream (used in place, nothing is waited for after the
        copy launch).  mark_updated: the chunks are also left as an integration that changed them leaves them (GetMeshesToUpdate
        names them and their resident neighbours).  -> the number of chunks created."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 3))
        n = len(ids)
        created = C.c_int64(0)
        on_device = 0
        arrays = []
        if any(hasattr(a, "is_cuda") for a in (sdf, weight, rgbw) if a is not None):
            import torch
            on_device = 1
            for a, (name, dtype, tail) in zip((sdf, weight, rgbw), self._CHUNK_ARRAYS):
                want = torch.uint8 if dtype is np.uint8 else torch.float32
                assert a is None or (a.is_cuda and a.dtype == want and a.is_contiguous() and tuple(a.shape) == (n, self.V) + tail), \
                    "%s: a contiguous %s CUDA tensor of shape %s" % (name, want, (n, self.V) + tail)
                arrays.append(a)
            ptrs = [a.data_ptr() if a is not None and a.numel() else None for a in arrays]
        else:
            for a, (name, dtype, tail) in zip((sdf, weight, rgbw), self._CHUNK_ARRAYS):
                arrays.append(np.ascontiguousarray(a, dtype).reshape((n, self.V) + tail) if a is not None else None)
            ptrs = [a.ctypes.data if a is not None and a.size else None for a in arrays]
        check(self.L.chisel_hip_scatter_chunks(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), n, *ptrs, on_device, 1 if mark_updated else 0, C.byref(created)))
        self._keep = [arrays]
        return created.value

    # the outputs of CoarseMesh and of IndexedMesh: (name, torch's dtype, the dtype as the entry's message spells it, the capacity its rows bound)
    _COARSE_OUTPUTS = (("vertices", "float32", "float32", "vertices"), ("normals", "float32", "float32", "vertices"), ("colors", "float32", "float32", "vertices"))
    _INDEXED_OUTPUTS = (("vertices", "float32", "torch.float32", "vertices"), ("indices", "int32", "torch.int32", "triangles"),
                        ("normals", "float32", "torch.float32", "vertices"), ("colors", "float32", "torch.float32", "vertices"))

    def _coarse_request(self, stride, ids, box, stages):
        """-> (chisel_hip_coarse_request, what it points at)"""
        req = capi.CoarseRequest()
        req.chunks, keep = self._chunk_request(ids, box)
        req.stride, req.stages = int(stride), int(stages)
        return req, keep

    @staticmethod
    def _out_named(out, outputs):
        """the names of the `out` dict of CoarseMesh / IndexedMesh against the entry's table of outputs"""
        unknown = set(out) - {row[0] for row in outputs}
        assert not unknown, "out: unknown outputs %s" % sorted(unknown)
        assert "vertices" in out, "out: vertices must be named"

    @staticmethod
    def _out_tensors(out, outputs):
        """the tensors of the `out` dict against the entry's table -> (the pointers in the table's order, None for an output that is
        not named or empty; {capacity: the fewest rows of the tensors that bound it}, a capacity that no tensor bounds missing)"""
        import torch
        ptrs, caps = [], {}
        for name, dtype, spelled, cap in outputs:
            t = out.get(name)
            assert t is None or (t.is_cuda and t.dtype == getattr(torch, dtype) and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 3), \
                "out[%r]: a contiguous %s CUDA tensor of shape (rows, 3)" % (name, spelled)
            if t is not None:
                caps[cap] = min(caps.get(cap, int(t.shape[0])), int(t.shape[0]))
            ptrs.append(t.data_ptr() if t is not None and t.numel() else None)
        return ptrs, caps

    @staticmethod
    def _table_ptr(a, ctype):
        """a numpy table as the C ABI takes it; an empty array has no address"""
        return a.ctypes.data_as(C.POINTER(ctype)) if a is not None and a.size else None

    def _mesh_call(self, entry, totals, *args):
        """chisel_hip_coarse_mesh / _indexed_mesh -> the totals; KeyError for a listed id that is not resident"""
        rc = entry(self.h, *args, C.byref(totals))
        if rc == 4:
            raise KeyError(self.L.chisel_hip_last_error().decode(errors="replace"))
        check(rc)
        return self._totals_dict(totals)

    def _coarse_call(self, req, capacity, ptrs, on_device, table, ids_out):
        """-> the totals"""
        return self._mesh_call(self.L.chisel_hip_coarse_mesh, capi.CoarseTotals(), C.byref(req), capacity, *ptrs, on_device,
                               self._table_ptr(table, C.c_int64), self._table_ptr(ids_out, C.c_int))

    def _write_mesh_ply(self, filename, v, c, idx):
        """chisel_hip_write_mesh_ply: float32 vertices and colours (or None), flat int64 indices -> False when the file cannot be written"""
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None and a.size else None
        rc = self.L.chisel_hip_write_mesh_ply(str(filename).encode(), fp(v), fp(c), len(v), idx.ctypes.data_as(C.POINTER(C.c_int64)) if len(idx) else None, len(idx))
        if rc == 6:
            return False
        check(rc)
        return True

    def CoarseMeshSize(self, stride, ids=None, box=None):
        """chisel_hip_coarse_mesh with a capacity of 0: the totals of a coarse mesh (CoarseMesh) -> {"chunks", "chunks_nonempty",
        "cubes_meshed", "vertices"}"""
        req, keep = self._coarse_request(stride, ids, box, 0)
        return self._coarse_call(req, 0, [None, None, None], 0, None, None)

    def CoarseMesh(self, stride, ids=None, box=None, normals=True, colors=None, out=None, stages=None):
        """chisel_hip_coarse_mesh: the marching-cubes mesh over every `stride`-th voxel (stride divides the chunk edge) of the chunks
        `ids` ((n, 3), in that order, duplicates allowed; None: every resident chunk in GetChunkIDs' order, with box=(lo, hi) those
        with lo <= id <= hi on every axis), packed in that order.  -> {"vertices": (V, 3), "normals": (V, 3), "colors": (V, 3)}
        float32 numpy arrays, None for what was not asked for (colors=None: asked for iff the map holds colour), plus "table": (n, 2)
        int64 -- first vertex, vertices of every chunk --, "ids": (n, 3) int32 and "totals".  stages: bit 0 gradient normals (else
        face normals), bit 1 colours; None: what the outputs asked for take.
        `out`: a dict of contiguous torch CUDA float32 tensors of shape (rows, 3) with at least V rows, "vertices" among them:
        exactly the outputs named in it are filled in place on the map's stream, without a wait after the one the call needs; it is
        returned with "table", "ids" and "totals" (numpy, host) added.  KeyError for a listed id that is not resident."""
        if out is not None:
            self._out_named(out, self._COARSE_OUTPUTS)
            if stages is None:
                stages = (1 if "normals" in out else 0) | (2 if "colors" in out else 0)
            req, keep = self._coarse_request(stride, ids, box, stages)
            ptrs, caps = self._out_tensors(out, self._COARSE_OUTPUTS)
            n = len(keep) if keep is not None else self.NumChunks()
            table, ids_out = np.zeros((n, 2), np.int64), np.zeros((n, 3), np.int32)
            if caps.get("vertices"):
                totals = self._coarse_call(req, caps["vertices"], ptrs, 1, table, ids_out)
            else:  # (an empty tensor has no address: it stands for its array only when there is nothing to write)
                totals = self._coarse_call(req, 0, [None, None, None], 0, table, ids_out)
                assert totals["vertices"] == 0, "out: tensors without room"
            self._keep = [out]
            res = dict(out)
            res.update(table=table[:totals["chunks"]], ids=ids_out[:totals["chunks"]], totals=totals)
            return res
        if colors is None:
            colors = self.use_color
        if stages is None:
            stages = (1 if normals else 0) | (2 if colors else 0)
        req, keep = self._coarse_request(stride, ids, box, stages)
        size = self._coarse_call(req, 0, [None, None, None], 0, None, None)
        n, V = size["chunks"], size["vertices"]
        asked = {"vertices": True, "normals": normals, "colors": colors}
        res = {name: (np.empty((V, 3), np.float32) if asked[name] else None) for name, *_ in self._COARSE_OUTPUTS}
        table, ids_out = np.zeros((n, 2), np.int64), np.zeros((n, 3), np.int32)
        # (nothing has changed the map since the size query; without a vertex the second call is the size query again, with the tables)
        ptrs = [res[name].ctypes.data if res[name] is not None and V else None for name, *_ in self._COARSE_OUTPUTS]
        totals = self._coarse_call(req, V, ptrs, 0, table, ids_out)
        res.update(table=table, ids=ids_out, totals=totals)
        return res

    def SaveCoarseMeshPLY(self, filename, stride):
        """the coarse mesh of every resident chunk (CoarseMesh) as SaveMeshPLYASCII writes a mesh (chisel_hip_write_mesh_ply)"""
        mesh = self.CoarseMesh(stride, normals=False, colors=self.use_color)
        v = np.ascontiguousarray(mesh["vertices"], np.float32)
        c = np.ascontiguousarray(mesh["colors"], np.float32) if mesh["colors"] is not None else None
        return self._write_mesh_ply(filename, v, c, np.arange(len(v), dtype=np.int64))

    def _indexed_call(self, req, cap_v, cap_t, ptrs, on_device, table, owner_table, owner_ids):
        """-> the totals"""
        return self._mesh_call(self.L.chisel_hip_indexed_mesh, capi.IndexedTotals(), C.byref(req), cap_v, cap_t, *ptrs, on_device,
                               self._table_ptr(table, C.c_int64), self._table_ptr(owner_table, C.c_int64), self._table_ptr(owner_ids, C.c_int))

    def IndexedMeshSize(self, stride, ids=None, box=None):
        """chisel_hip_indexed_mesh with both capacities 0: the totals of an indexed mesh (IndexedMesh) -> {"chunks", "owners",
        "cubes_meshed", "vertices", "triangles"}"""
        req, keep = self._coarse_request(stride, ids, box, 0)
        return self._indexed_call(req, 0, 0, [None] * 4, 0, None, None, None)

    def IndexedMesh(self, stride, ids=None, box=None, normals=True, colors=None, out=None):
        """chisel_hip_indexed_mesh: the coarse mesh's triangles (CoarseMesh: same selection, stride and order) over ONE vertex per
        crossed lattice edge.  -> {"vertices": (V, 3) float32, "indices": (T, 3) int32, "normals": (V, 3), "colors": (V, 3)} numpy
        arrays, None for what was not asked for (colors=None: asked for iff the map holds colour; normals are gradient normals, zeros
        where the look-up fails), plus "table": (n, 2) int64 -- first triangle, triangles of every selected chunk --, "owner_table":
        (owners, 2) int64 -- first vertex, vertices of every owner: the selected chunks, then the resident + neighbours that are not
        selected, ascending --, "owner_ids": (owners, 3) int32 and "totals".  The ids of a list are distinct.
        `out`: a dict of contiguous torch CUDA tensors, "vertices" (rows, 3) float32 among them, "indices" (rows, 3) int32, "normals"
        and "colors" (rows, 3) float32 with at least V rows: exactly the outputs named in it are filled in place on the map's
        stream, without a wait after the one the call needs; it is returned with the host tables and "totals" added.  KeyError for a
        listed id that is not resident."""
        if out is not None:
            self._out_named(out, self._INDEXED_OUTPUTS)
            stages = (1 if "normals" in out else 0) | (2 if "colors" in out else 0)
            req, keep = self._coarse_request(stride, ids, box, stages)
            ptrs, caps = self._out_tensors(out, self._INDEXED_OUTPUTS)
            n = len(keep) if keep is not None else self.NumChunks()
            table, owner_table, owner_ids = np.zeros((n, 2), np.int64), np.zeros((8 * n, 2), np.int64), np.zeros((8 * n, 3), np.int32)
            cap_v, cap_t = caps.get("vertices"), caps.get("triangles", 0)
            if "indices" not in out:
                cap_t = 1 << 40  # (no index array: its capacity is not in the way)
            if cap_v:
                totals = self._indexed_call(req, cap_v, cap_t, ptrs, 1, table, owner_table, owner_ids)
            else:  # (an empty tensor has no address: it stands for its array only when there is nothing to write)
                totals = self._indexed_call(req, 0, 0, [None] * 4, 0, table, owner_table, owner_ids)
                assert totals["vertices"] == 0, "out: tensors without room"
            self._keep = [out]
            res = dict(out)
            res.update(table=table[:totals["chunks"]], owner_table=owner_table[:totals["owners"]], owner_ids=owner_ids[:totals["owners"]], totals=totals)
            return res
        if colors is None:
            colors = self.use_color
        stages = (1 if normals else 0) | (2 if colors else 0)
        req, keep = self._coarse_request(stride, ids, box, stages)
        size = self._indexed_call(req, 0, 0, [None] * 4, 0, None, None, None)
        n, owners, V, T = size["chunks"], size["owners"], size["vertices"], size["triangles"]
        asked = {"vertices": True, "indices": True, "normals": normals, "colors": colors}
        res = {name: (np.empty((T, 3), np.int32) if name == "indices" else np.empty((V, 3), np.float32)) if asked[name] else None for name, *_ in self._INDEXED_OUTPUTS}
        table, owner_table, owner_ids = np.zeros((n, 2), np.int64), np.zeros((owners, 2), np.int64), np.zeros((owners, 3), np.int32)
        # (nothing has changed the map since the size query; without a vertex the second call is the size query again, with the tables)
        ptrs = [res[name].ctypes.data if res[name] is not None and res[name].size and V else None for name, *_ in self._INDEXED_OUTPUTS]
        totals = self._indexed_call(req, V, T if V else 0, ptrs, 0, table, owner_table, owner_ids)
        res.update(table=table, owner_table=owner_table, owner_ids=owner_ids, totals=totals)
        return res

    def SaveIndexedMeshPLY(self, filename, stride, binary=True):
        """the indexed mesh of every resident chunk (IndexedMesh) as a PLY file with a real face list: binary=False as SaveMeshPLYASCII
        writes a mesh (chisel_hip_write_mesh_ply), binary=True with SaveMeshPLYBinary's elements and properties"""
        return self._write_indexed_ply(filename, self.IndexedMesh(stride, normals=False, colors=self.use_color), binary)

    def _write_indexed_ply(self, filename, mesh, binary):
        """the writer of SaveIndexedMeshPLY and SaveCleanMeshPLY: a dict with "vertices", "indices" and "colors" (or None), numpy"""
        v = np.ascontiguousarray(mesh["vertices"], np.float32)
        c = np.ascontiguousarray(mesh["colors"], np.float32) if mesh["colors"] is not None else None
        if not binary:
            return self._write_mesh_ply(filename, v, c, np.ascontiguousarray(mesh["indices"].reshape(-1), np.int64))
        any_color = c is not None and len(v) > 0
        head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
        if any_color:
            head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        head += "element face %d\nproperty list uchar int vertex_index\nend_header\n" % len(mesh["indices"])
        vert = np.zeros(len(v), np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if any_color else [])))
        vert["p"] = v
        if any_color:
            vert["c"] = (c * np.float32(255.0)).astype(np.int32).astype(np.uint8)  # (write_ply's conversion)
        face = np.zeros(len(mesh["indices"]), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
        face["n"], face["i"] = 3, mesh["indices"]
        try:
            with open(str(filename), "wb") as f:
                f.write(head.encode())
                f.write(vert.tobytes())
                f.write(face.tobytes())
        except OSError:
            return False
        return True

    @staticmethod
    def _is_tensor(a):
        return a is not None and not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")

    @staticmethod
    def _device_rows(t, name, dtype, width, rows):
        """a contiguous CUDA tensor of (>= rows, width) (width 0: one dimension) -> its address, None without a row to write"""
        import torch
        if t is None:
            return None
        shape_ok = (t.dim() == 2 and t.shape[1] == width) if width else t.dim() == 1
        assert t.is_cuda and t.dtype == getattr(torch, dtype) and t.is_contiguous() and shape_ok, \
            "%s: a contiguous torch.%s CUDA tensor of shape (rows%s)" % (name, dtype, ", %d" % width if width else "")
        assert t.shape[0] >= rows, "%s: %d rows, %d are needed" % (name, t.shape[0], rows)
        return t.data_ptr() if rows and t.numel() else None

    def _components_call(self, entry, *args):
        """chisel_hip_mesh_components / _filter_mesh -> the totals"""
        totals = capi.ComponentsTotals()
        check(entry(self.h, *args, C.byref(totals)))
        return self._totals_dict(totals)

    def MeshComponents(self, indices, n_vertices=None, out=None):
        """chisel_hip_mesh_components: the connected components of the graph whose vertices are 0 ... n_vertices - 1 and whose edges
        are the sides of the triangles `indices` -- a numpy (T, 3) int32 array (n_vertices=None: indices.max() + 1) or a contiguous
        torch CUDA int32 tensor (n_vertices is required), for instance IndexedMesh's.  A triangle with an id outside [0, n_vertices)
        joins nothing and has component -1.  Components are numbered by ascending smallest vertex id.  -> {"vertex_component": (V,)
        int32, "triangle_component": (T,) int32, "table": (C, 3) int64 -- root, vertices, triangles of every component --, "totals"};
        the labels are numpy arrays for numpy indices and CUDA tensors for a tensor.  `out`: a dict of contiguous CUDA int32 tensors
        "vertex_component" (>= V rows) and / or "triangle_component" (>= T rows): exactly those are filled in place on the map's
        stream; it is returned with "table" and "totals" (host) added.  The map itself is not touched."""
        entry = self.L.chisel_hip_mesh_components
        names = ("vertex_component", "triangle_component")
        if self._is_tensor(indices):
            import torch
            assert n_vertices is not None, "n_vertices is required for a tensor"
            V, T = int(n_vertices), int(indices.shape[0])
            src = self._device_rows(indices, "indices", "int32", 3, T)
            if out is None:
                out = {"vertex_component": torch.empty(V, dtype=torch.int32, device=indices.device),
                       "triangle_component": torch.empty(T, dtype=torch.int32, device=indices.device)}
            assert not set(out) - set(names), "out: unknown outputs %s" % sorted(set(out) - set(names))
            ptrs = [self._device_rows(out.get(name), "out[%r]" % name, "int32", 0, rows) for name, rows in zip(names, (V, T))]
            table = np.zeros((V, 3), np.int64)
            totals = self._components_call(entry, V, T, src, 1, ptrs[0], ptrs[1], V, self._table_ptr(table, C.c_int64))
            self._keep = [indices, out]
            res = dict(out)
            res.update(table=table[:totals["components"]], totals=totals)
            return res
        assert out is None, "out: device tensors go with a tensor of indices"
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
        T = len(idx)
        V = int(n_vertices) if n_vertices is not None else (max(int(idx.max()) + 1, 0) if T else 0)
        vc, tc, table = np.empty(V, np.int32), np.empty(T, np.int32), np.zeros((V, 3), np.int64)
        totals = self._components_call(entry, V, T, idx.ctypes.data if T else None, 0, vc.ctypes.data if V else None, tc.ctypes.data if T else None, V,
                                       self._table_ptr(table, C.c_int64))
        return {"vertex_component": vc, "triangle_component": tc, "table": table[:totals["components"]], "totals": totals}

    _FILTER_OUTPUTS = (("vertices", "float32", 3, "V"), ("indices", "int32", 3, "T"), ("normals", "float32", 3, "V"), ("colors", "float32", 3, "V"),
                       ("vertex_map", "int32", 0, "V"), ("triangle_map", "int32", 0, "T"))

    def FilterMesh(self, mesh, min_triangles=1, largest_only=False, out=None):
        """chisel_hip_filter_mesh: `mesh` -- the dict IndexedMesh returns, numpy or its `out` form with CUDA tensors; the number of
        vertices and triangles is its "totals" entry where it has one, else the arrays' rows -- without the connected components
        (MeshComponents) of fewer than `min_triangles` triangles; with largest_only only the component with the most triangles, the
        lowest-numbered of equals, if it has min_triangles.  Kept vertices and triangles keep their order, ids are renumbered, the
        rows of "vertices", "normals" and "colors" are copied bit for bit.  -> {"vertices", "indices", "normals", "colors" (None where
        the mesh has none), "vertex_map": (V,) int32, "triangle_map": (T,) int32 -- old -> new, -1 when dropped --, "totals"}, of the
        mesh's kind (numpy arrays, or CUDA tensors narrowed to the kept rows).  `out`: a dict of contiguous CUDA tensors named like
        the result: exactly those are filled in place on the map's stream, without a wait behind the one for the totals; it is
        returned with "totals" added.  The per-chunk tables are not carried over; the map itself is not touched."""
        entry = self.L.chisel_hip_filter_mesh
        v, idx, tot = mesh["vertices"], mesh["indices"], mesh.get("totals")
        have = {"vertices": v, "indices": idx, "normals": mesh.get("normals"), "colors": mesh.get("colors")}
        V = int(tot["vertices"]) if tot and "vertices" in tot else int(v.shape[0])
        T = int(tot["triangles"]) if tot and "triangles" in tot else int(idx.shape[0])
        head = (V, T)
        knobs = (int(min_triangles), int(largest_only))
        if self._is_tensor(v):
            import torch
            narrowed = out is None
            if narrowed:
                rows = {"V": V, "T": T}
                out = {name: torch.empty((rows[n], width) if width else (rows[n],), dtype=getattr(torch, dtype), device=v.device)
                       for name, dtype, width, n in self._FILTER_OUTPUTS if name not in have or have[name] is not None}
            unknown = set(out) - {row[0] for row in self._FILTER_OUTPUTS}
            assert not unknown, "out: unknown outputs %s" % sorted(unknown)
            src = [self._device_rows(have[name], "mesh[%r]" % name, dtype, 3, V if n == "V" else T) if (name in out or name == "indices") else None
                   for name, dtype, _, n in self._FILTER_OUTPUTS[:4]]
            cap = {"V": None, "T": None}
            for name, dtype, width, n in self._FILTER_OUTPUTS[:4]:
                if name in out:
                    cap[n] = min(cap[n], int(out[name].shape[0])) if cap[n] is not None else int(out[name].shape[0])
            cap_v = cap["V"] if cap["V"] is not None else 1  # (maps alone: any capacity but the size query's)
            cap_t = cap["T"] if cap["T"] is not None else 1
            for name, dtype, width, n in self._FILTER_OUTPUTS[:4]:  # (kind and shape; the rows are the capacity)
                self._device_rows(out.get(name), "out[%r]" % name, dtype, width, 0)
            dst = [out[name].data_ptr() if name in out and out[name].numel() else None for name, *_ in self._FILTER_OUTPUTS[:4]]
            maps = [self._device_rows(out.get(name), "out[%r]" % name, "int32", 0, V if n == "V" else T) for name, _, _, n in self._FILTER_OUTPUTS[4:]]
            totals = self._components_call(entry, *head, src[1], src[0], src[2], src[3], *knobs, cap_v, cap_t, dst[0], dst[1], dst[2], dst[3], maps[0], maps[1], 1)
            assert (cap["V"] is None or totals["kept_vertices"] <= cap_v) and (cap["T"] is None or totals["kept_triangles"] <= cap_t), "out: tensors without room"
            self._keep = [mesh, out]
            res = dict(out)
            if narrowed:
                for name, _, _, n in self._FILTER_OUTPUTS[:4]:
                    res[name] = out[name][:totals["kept_vertices" if n == "V" else "kept_triangles"]] if name in out else None
            res["totals"] = totals
            return res
        assert out is None, "out: device tensors go with a mesh of tensors"
        arr = {"vertices": np.ascontiguousarray(v, np.float32).reshape(-1, 3)[:V], "indices": np.ascontiguousarray(idx, np.int32).reshape(-1, 3)[:T]}
        for name in ("normals", "colors"):
            arr[name] = np.ascontiguousarray(have[name], np.float32).reshape(-1, 3)[:V] if have[name] is not None else None
        res = {name: (np.empty_like(arr[name]) if arr[name] is not None else None) for name in arr}
        res["vertex_map"], res["triangle_map"] = np.empty(V, np.int32), np.empty(T, np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        totals = self._components_call(entry, *head, ptr(arr["indices"]), ptr(arr["vertices"]), ptr(arr["normals"]), ptr(arr["colors"]), *knobs, max(V, 1), max(T, 1),
                                       ptr(res["vertices"]), ptr(res["indices"]), ptr(res["normals"]), ptr(res["colors"]), ptr(res["vertex_map"]),
                                       ptr(res["triangle_map"]), 0)
        for name, _, _, n in self._FILTER_OUTPUTS[:4]:
            if res[name] is not None:
                res[name] = res[name][:totals["kept_vertices" if n == "V" else "kept_triangles"]]
        res["totals"] = totals
        return res

    def SaveCleanMeshPLY(self, filename, stride, min_triangles, largest_only=False, binary=True):
        """SaveIndexedMeshPLY without the connected components of fewer than `min_triangles` triangles (FilterMesh): the indexed mesh
        of every resident chunk, filtered on the device, through the same writer"""
        mesh = self.IndexedMesh(stride, normals=False, colors=self.use_color)
        return self._write_indexed_ply(filename, self.FilterMesh(mesh, min_triangles, largest_only), binary)

    MESH_BOUNDARY, MESH_NONMANIFOLD, MESH_ISOLATED = capi.MESH_BOUNDARY, capi.MESH_NONMANIFOLD, capi.MESH_ISOLATED
    _ADJACENCY_OUTPUTS = ("tri_offsets", "tri_items", "nbr_offsets", "nbr_items", "flags")

    def _adjacency_call(self, entry, *args):
        """chisel_hip_mesh_adjacency / _mesh_vertex_normals / _smooth_mesh -> the totals"""
        totals = capi.AdjacencyTotals()
        check(entry(self.h, *args, C.byref(totals)))
        return self._totals_dict(totals)

    def MeshAdjacency(self, indices, n_vertices=None, out=None):
        """chisel_hip_mesh_adjacency: the vertex -> triangle incidence and the vertex -> vertex neighbour rows of the triangles
        `indices` over the vertices 0 ... n_vertices - 1 -- a numpy (T, 3) int32 array (n_vertices=None: indices.max() + 1) or a
        contiguous torch CUDA int32 tensor (n_vertices is required), for instance IndexedMesh's.  A triangle with an id outside
        [0, n_vertices) takes part in nothing.  -> {"tri_offsets": (V + 1,), "tri_items": (incidences,), "nbr_offsets": (V + 1,),
        "nbr_items": (neighbors,), "flags": (V,) int32 -- bit 0 MESH_BOUNDARY, bit 1 MESH_NONMANIFOLD, bit 2 MESH_ISOLATED --,
        "totals"}: row v of a pair is items[offsets[v]:offsets[v + 1]], ascending; numpy arrays for numpy indices, CUDA tensors for a
        tensor.  `out`: a dict of contiguous CUDA int32 tensors named like the result (3 T and 6 T items are always enough): exactly
        those are filled in place on the map's stream; it is returned with "totals" (host) added.  An index array with more than
        capi.MESH_MAX_INCIDENT triangles at one vertex is refused.  The map itself is not touched."""
        entry = self.L.chisel_hip_mesh_adjacency
        names = self._ADJACENCY_OUTPUTS
        if self._is_tensor(indices):
            import torch
            assert n_vertices is not None, "n_vertices is required for a tensor"
            V, T = int(n_vertices), int(indices.shape[0])
            src = self._device_rows(indices, "indices", "int32", 3, T)
            narrowed = out is None
            if narrowed:
                size = self._adjacency_call(entry, V, T, src, 1, None, 0, None, None, 0, None, None)
                rows = {"tri_offsets": V + 1, "tri_items": size["incidences"], "nbr_offsets": V + 1, "nbr_items": size["neighbors"], "flags": V}
                out = {name: torch.empty(rows[name], dtype=torch.int32, device=indices.device) for name in names}
            assert not set(out) - set(names), "out: unknown outputs %s" % sorted(set(out) - set(names))
            need = {"tri_offsets": V + 1, "tri_items": 0, "nbr_offsets": V + 1, "nbr_items": 0, "flags": V}
            ptrs = {name: self._device_rows(out.get(name), "out[%r]" % name, "int32", 0, need[name]) for name in names}
            cap = {name: int(out[name].shape[0]) if name in out else 0 for name in ("tri_items", "nbr_items")}
            for name in cap:  # (an empty tensor has no address: it stands for its array only when there is nothing to write)
                ptrs[name] = out[name].data_ptr() if cap[name] else None
            totals = self._adjacency_call(entry, V, T, src, 1, ptrs["tri_offsets"], cap["tri_items"], ptrs["tri_items"], ptrs["nbr_offsets"], cap["nbr_items"],
                                          ptrs["nbr_items"], ptrs["flags"])
            assert ("tri_items" not in out or totals["incidences"] <= cap["tri_items"]) and ("nbr_items" not in out or totals["neighbors"] <= cap["nbr_items"]), \
                "out: tensors without room"
            self._keep = [indices, out]
            res = dict(out)
            res["totals"] = totals
            return res
        assert out is None, "out: device tensors go with a tensor of indices"
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
        T = len(idx)
        V = int(n_vertices) if n_vertices is not None else (max(int(idx.max()) + 1, 0) if T else 0)
        src = idx.ctypes.data if T else None
        size = self._adjacency_call(entry, V, T, src, 0, None, 0, None, None, 0, None, None)
        res = {"tri_offsets": np.empty(V + 1, np.int32), "tri_items": np.empty(size["incidences"], np.int32), "nbr_offsets": np.empty(V + 1, np.int32),
               "nbr_items": np.empty(size["neighbors"], np.int32), "flags": np.empty(V, np.int32)}
        ptr = lambda a: a.ctypes.data if a.size else None
        res["totals"] = self._adjacency_call(entry, V, T, src, 0, ptr(res["tri_offsets"]), size["incidences"], ptr(res["tri_items"]), ptr(res["nbr_offsets"]),
                                             size["neighbors"], ptr(res["nbr_items"]), ptr(res["flags"]))
        return res

    def _mesh_arrays(self, mesh):
        """the "vertices" and "indices" of a mesh dict, and its sizes (its "totals" entry where it has one, else the arrays' rows) ->
        (V, T, vertices, indices, on_device, their addresses)"""
        v, idx, tot = mesh["vertices"], mesh["indices"], mesh.get("totals")
        V = int(tot["kept_vertices" if "kept_vertices" in tot else "vertices"]) if tot and ("vertices" in tot or "kept_vertices" in tot) else int(v.shape[0])
        T = int(tot["kept_triangles" if "kept_triangles" in tot else "triangles"]) if tot and ("triangles" in tot or "kept_triangles" in tot) else int(idx.shape[0])
        if self._is_tensor(v):
            return V, T, v, idx, 1, self._device_rows(v, "mesh['vertices']", "float32", 3, V), self._device_rows(idx, "mesh['indices']", "int32", 3, T)
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)[:V]
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)[:T]
        return V, T, v, idx, 0, v.ctypes.data if V else None, idx.ctypes.data if T else None

    def MeshVertexNormals(self, mesh, out=None):
        """chisel_hip_mesh_vertex_normals: the normals that belong to the triangles of `mesh` -- a dict with "vertices" and "indices"
        as IndexedMesh / FilterMesh / SmoothMesh return it, numpy or CUDA tensors --: per vertex the sum of its incident triangles'
        un-normalised face normals (area-weighted, pointing where the coarse mesh's face normals point), added in ascending triangle
        order and normalised; zeros for a vertex without a triangle of non-zero area.  -> (V, 3) float32, of the mesh's kind.  `out`:
        a contiguous CUDA float32 tensor of (>= V, 3), filled in place on the map's stream and returned."""
        V, T, v, idx, on_device, pv, pi = self._mesh_arrays(mesh)
        if on_device:
            import torch
            if out is None:
                out = torch.empty((V, 3), dtype=torch.float32, device=v.device)
            dst = self._device_rows(out, "out", "float32", 3, V)
            self._adjacency_call(self.L.chisel_hip_mesh_vertex_normals, V, T, pi, pv, 1, dst)
            self._keep = [mesh, out]
            return out
        assert out is None, "out: a device tensor goes with a mesh of tensors"
        normals = np.empty((V, 3), np.float32)
        self._adjacency_call(self.L.chisel_hip_mesh_vertex_normals, V, T, pi, pv, 0, normals.ctypes.data if V else None)
        return normals

    def SmoothMesh(self, mesh, iterations=10, lam=0.5, mu=-0.53, pin=capi.MESH_BOUNDARY | capi.MESH_NONMANIFOLD, normals=True, out=None):
        """chisel_hip_smooth_mesh: Taubin lambda | mu smoothing of `mesh` -- the dict IndexedMesh / FilterMesh return, numpy or CUDA
        tensors -- over the 1-ring: an iteration moves every vertex by lam times the way to its neighbours' mean, then by mu times
        (mu < 0: it does not shrink the surface; mu == 0: plain Laplacian smoothing).  Vertices whose flags (MeshAdjacency) meet `pin`
        -- by default the open rim and the non-manifold ones -- and those without a neighbour stay where they are.  -> the mesh's
        dict with "vertices" smoothed, "normals" the vertex normals of the smoothed positions (MeshVertexNormals; None with
        normals=False), "indices" and "colors" carried over unchanged, and "totals" (pinned_vertices among them).  `out`: a dict of
        contiguous CUDA float32 tensors "vertices" (>= V, 3) and optionally "normals": filled in place on the map's stream, without a
        wait behind the one for the totals; it is returned with the carried-over entries and "totals" added."""
        entry = self.L.chisel_hip_smooth_mesh
        V, T, v, idx, on_device, pv, pi = self._mesh_arrays(mesh)
        knobs = (int(iterations), float(lam), float(mu), int(pin))
        res = {"indices": mesh["indices"], "colors": mesh.get("colors")}
        if on_device:
            import torch
            if out is None:
                out = {"vertices": torch.empty((V, 3), dtype=torch.float32, device=v.device)}
                if normals:
                    out["normals"] = torch.empty((V, 3), dtype=torch.float32, device=v.device)
            assert "vertices" in out and not set(out) - {"vertices", "normals"}, "out: \"vertices\" and optionally \"normals\""
            dst = [self._device_rows(out.get(name), "out[%r]" % name, "float32", 3, V) for name in ("vertices", "normals")]
            totals = self._adjacency_call(entry, V, T, pi, pv, *knobs, 1, dst[0], dst[1])
            self._keep = [mesh, out]
            res.update(vertices=out["vertices"], normals=out.get("normals"), totals=totals)
            return res
        assert out is None, "out: device tensors go with a mesh of tensors"
        res["indices"] = idx
        if res["colors"] is not None:
            res["colors"] = np.ascontiguousarray(res["colors"], np.float32).reshape(-1, 3)[:V]
        ov = np.empty((V, 3), np.float32)
        on = np.empty((V, 3), np.float32) if normals else None
        totals = self._adjacency_call(entry, V, T, pi, pv, *knobs, 0, ov.ctypes.data if V else None, on.ctypes.data if normals and V else None)
        res.update(vertices=ov, normals=on, totals=totals)
        return res

    def SaveSmoothMeshPLY(self, filename, stride, iterations, min_triangles=1, lam=0.5, mu=-0.53, pin=capi.MESH_BOUNDARY | capi.MESH_NONMANIFOLD, binary=True):
        """SaveCleanMeshPLY with the kept mesh smoothed (SmoothMesh): the indexed mesh of every resident chunk, filtered and smoothed
        on the device, through the same writer"""
        mesh = self.FilterMesh(self.IndexedMesh(stride, normals=False, colors=self.use_color), min_triangles)
        return self._write_indexed_ply(filename, self.SmoothMesh(mesh, iterations, lam, mu, pin, normals=False), binary)

    def AlignTerms(self, depth, pose, camera, max_residual=0.0, out=None):
        """chisel_hip_align_terms: the normal equations of one Gauss-Newton step that aligns the depth image (numpy, or a torch CUDA
        tensor used in place) taken by `camera` at the guess `pose` (camera -> world) to the map.  -> (32,) float64: [0..20] the upper
        triangle of sum J J^T, [21..26] sum J rho, [27] sum rho^2, [28] used pixels, [29] valid pixels, [30], [31] 0.
        `out`: a contiguous float64 torch CUDA tensor of 32 elements, filled on the map's stream, nothing waited for; it is returned."""
        f, keep = depth_frame(depth, pose, camera)
        if out is not None:
            import torch
            assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 32, \
                "out: a contiguous float64 CUDA tensor of 32 elements"
            check(self.L.chisel_hip_align_terms(self.h, C.byref(f), float(max_residual), out.data_ptr(), 1))
            self._keep = [keep, out]
            return out
        terms = np.empty(32, np.float64)
        check(self.L.chisel_hip_align_terms(self.h, C.byref(f), float(max_residual), terms.ctypes.data, 0))
        return terms

    def AlignDepth(self, depth, pose, camera, max_iterations=10, max_residual=0.0, damping=1e-3, min_translation=1e-5,
                   min_rotation=1e-5, min_pixels=100):
        """chisel_hip_align_depth: Gauss-Newton on the pose of a depth frame against the map, from the guess `pose` -- to refine a
        keyframe's pose before IntegrateDepthScan.  -> {"pose": (3, 4) float64, "status": capi.ALIGN_*, "iterations": updates applied,
        "xi_last": (6,) the last update (v, w), "terms_first" / "terms_last": (32,) AlignTerms at the guess / as last evaluated}.
        All four statuses are outcomes, not errors."""
        f, keep = depth_frame(depth, pose, camera)
        p = capi.AlignParams(int(max_iterations), int(min_pixels), float(max_residual), 0.0, float(damping), float(min_translation),
                             float(min_rotation))
        r = capi.AlignResult()
        check(self.L.chisel_hip_align_depth(self.h, C.byref(f), C.byref(p), C.byref(r)))
        return {"pose": np.array(r.pose, np.float64).reshape(3, 4), "status": int(r.status), "iterations": int(r.iterations),
                "xi_last": np.array(r.xi_last, np.float64), "terms_first": np.array(r.terms_first, np.float64),
                "terms_last": np.array(r.terms_last, np.float64)}

    def MergeMap(self, other, src_to_dst, stats=True):
        """chisel_hip_merge_map: `other`, moved by the rigid transform src_to_dst (3 x 4 or 4 x 4), is fused into this map on the
        device; `other` is only read.  -> {"src_chunks", "dst_chunks_created", "dst_chunks_updated", "voxels_updated"}; stats=False:
        the call does not wait for its own end and returns None"""
        if not stats:
            check(self.L.chisel_hip_merge_map(self.h, other.h, _pose12(src_to_dst), None))
            return None
        st = capi.MergeStats()
        check(self.L.chisel_hip_merge_map(self.h, other.h, _pose12(src_to_dst), C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in capi.MergeStats._fields_}

    def DeintegrateDepthScan(self, integrator, depth_image, extrinsic, camera, color_rules=False, stats=True, collect=False):
        """chisel_hip_deintegrate_depth: the depth frame (numpy, or a torch CUDA tensor used in place) that was integrated at `extrinsic`
        with `integrator` is taken out of the distance voxels again; color_rules: it went in through IntegrateDepthScanColor.  ->
        {"chunks_tested", "chunks_touched", "chunks_emptied", "voxels_updated", "voxels_cleared", "voxels_skipped", "emptied_ids": (k, 3)
        int32, the chunks left without any weight}; collect=True hands those to GarbageCollect.  stats=False: the call does not wait
        for its own end and returns None"""
        self._use(integrator)
        f, keep = depth_frame(depth_image, extrinsic, camera)
        return self._deintegrate(self.L.chisel_hip_deintegrate_depth, (self.h, C.byref(f), int(bool(color_rules))), [keep], stats, collect)

    def _deintegrate(self, entry, head, keep, stats, collect):
        """the tail of DeintegrateDepthScan and DeintegrateDepthScans: `entry` is the C entry, `head` its arguments in front of
        (stats, ids, max_ids), `keep` what the frames point at"""
        if not stats:
            assert not collect, "collect=True needs the ids, which stats=False does not wait for"
            check(entry(*head, None, None, 0))
            self._keep = keep  # (the call may still be queued: the images live until the next one)
            return None
        st = capi.DeintegrateStats()
        ids = np.zeros((max(1, self.NumChunks()), 3), np.int32)  # (no chunk is created: the resident ones bound the emptied ones)
        check(entry(*head, C.byref(st), ids.ctypes.data_as(C.POINTER(C.c_int)), len(ids)))  # (it has waited for its own end: nothing to keep)
        out = {n: int(getattr(st, n)) for n, _ in capi.DeintegrateStats._fields_}
        out["emptied_ids"] = ids[:min(out["chunks_emptied"], len(ids))].copy()
        if collect and len(out["emptied_ids"]):
            self.GarbageCollect(out["emptied_ids"])
        return out

    def ReintegrateDepthScan(self, integrator, depth_image, old_extrinsic, new_extrinsic, camera, color_image=None, color_camera=None,
                             stats=True, collect=False):
        """a keyframe whose pose was corrected after it was fused: DeintegrateDepthScan at the pose it went in with, then the same
        integration at the corrected one.  Without color_image the frame went in through IntegrateDepthScan and goes back that way
        (the depth rules); with it, through IntegrateDepthScanColor (the colour rules), the colour camera (default: `camera`)
        riding on the depth camera's pose -- the distance voxels follow the correction, the colour voxels only gain the second
        look.  -> what DeintegrateDepthScan returns"""
        colour = color_image is not None
        out = self.DeintegrateDepthScan(integrator, depth_image, old_extrinsic, camera, colour, stats, collect)
        if colour:
            self.IntegrateDepthScanColor(integrator, depth_image, new_extrinsic, camera, color_image, new_extrinsic, color_camera or camera)
        else:
            self.IntegrateDepthScan(integrator, depth_image, new_extrinsic, camera)
        return out

    def DeintegrateDepthScans(self, integrator, frames, color_rules=False, stats=True, collect=False):
        """chisel_hip_deintegrate_batch: the frames -- a list of (depth, pose, camera) as IntegrateBatch takes them, numpy images or
        torch CUDA tensors used in place, of any mix of sizes and cameras -- are taken out of the distance voxels in one call; the
        map is left, bit for bit, as DeintegrateDepthScan on each of them in list order would leave it, and a voxel under several
        frames of a launch set of 16 is read and written once.  -> what DeintegrateDepthScan returns, the six counts summed over the
        frames ("chunks_emptied" and "emptied_ids": the chunks without any weight at the end, each once); collect=True hands those to
        GarbageCollect.  stats=False: the call does not wait for its own end and returns None"""
        self._use(integrator)
        n = len(frames)
        fa = (DepthFrame * max(n, 1))()
        keep = []
        for i, (d, p, cam) in enumerate(frames):
            fa[i], k = depth_frame(d, p, cam)
            keep.append(k)
        return self._deintegrate(self.L.chisel_hip_deintegrate_batch, (self.h, n, fa, int(bool(color_rules))), keep, stats, collect)

    def ReintegrateDepthScans(self, integrator, frames, new_poses, colors=None, stats=True, collect=False):
        """a stretch of trajectory whose poses were corrected after its keyframes were fused: DeintegrateDepthScans of `frames` (a
        list of (depth, pose, camera), the poses they went in with), then IntegrateBatch of the same images at `new_poses`.  With
        `colors` (a list of (color image, color camera), or of color images alone, which take the depth camera) the frames went in
        through the colour rules and go back that way, each colour camera riding on the corrected depth pose.
        All out, then all in: NOT the arithmetic of n calls of ReintegrateDepthScan, which take out and put back frame by frame --
        the two orders round differently.  -> what DeintegrateDepthScans returns"""
        assert len(new_poses) == len(frames) and (colors is None or len(colors) == len(frames))
        out = self.DeintegrateDepthScans(integrator, frames, colors is not None, stats, collect)
        again = [(d, p, cam) for (d, _, cam), p in zip(frames, new_poses)]
        riding = None
        if colors is not None:
            riding = []
            for c, p, (_, _, cam) in zip(colors, new_poses, frames):
                image, ccam = c if isinstance(c, (tuple, list)) else (c, cam)
                riding.append((image, p, ccam))
        if again:
            self.IntegrateBatch(integrator, again, riding)
        return out

    def MemoryStatistics(self):
        """ChunkManager::PrintMemoryStatistics (ChunkManager.cpp:641-678) as numbers: the voxel census of Chunk::ComputeStatistics over
        the resident chunks, the weight sum, the bounds of the chunk boxes and the two memory figures the reference prints (it
        prices a voxel at sizeof(DistVoxel) = 16 bytes)."""
        st = capi.Statistics()
        check(self.L.chisel_hip_memory_statistics(self.h, C.byref(st)))
        n, res = self.chunk_size, np.float32(self.voxel_resolution)
        out = {"numUnknown": st.n_unknown, "numKnownInside": st.n_known_inside, "numKnownOutside": st.n_known_outside,
               "totalWeight": st.total_weight, "chunks": st.n_chunks}
        if st.n_chunks:
            lo = np.array([np.float32(n[a] * st.id_min[a]) * res for a in range(3)], np.float32)                       # Chunk.cpp:43
            hi = np.array([np.float32(n[a] * st.id_max[a]) * res + np.float32(n[a]) * res for a in range(3)], np.float32)  # Chunk.cpp:65-70
            out["bounds"] = (lo, hi)
            ext = (hi - lo) * np.float32(0.5)                                                                         # AABB::GetExtents
            nv = ext * np.float32(2) / res
            out["max_memory_mb"] = float(nv[0] * nv[1] * nv[2] * np.float32(16) / np.float32(1000000.0))
        out["current_memory_mb"] = float(np.float32(st.n_chunks * n[0] * n[1] * n[2] * 16) / np.float32(1000000.0))
        return out

    # ---- measurement ----------------------------------------------------------------------------------
    def counters(self, reset=False):
        out = (C.c_uint64 * capi.NUM_COUNTERS)()
        check(self.L.chisel_hip_get_counters(self.h, out, int(reset)))
        return dict(zip(capi.COUNTER_NAMES, [int(v) for v in out]))

    def set_profiling(self, enable):
        check(self.L.chisel_hip_set_profiling(self.h, int(enable)))

    def profile(self, reset=False):
        ms = (C.c_double * capi.NUM_KERNELS)()
        n = (C.c_int64 * capi.NUM_KERNELS)()
        check(self.L.chisel_hip_get_profile(self.h, ms, n, int(reset)))
        return {k: {"ms": ms[i], "launches": int(n[i])} for i, k in enumerate(capi.KERNEL_NAMES)}

    LAUNCH_STATS = ("integrate_2_per_lane", "integrate_4_per_lane", "integrate_4_with_2_tail", "cull_4_waves", "cull_wave_per_frame",
                    "unordered_worklists", "single_stream_sets", "launch_sets", "behind_unseen_recompute", "replayed")

    def pool_info(self):
        """chisel_hip_pool_info: chunks committed now, the pool's limit, times it has grown, whether it can"""
        out = (C.c_int64 * 4)()
        check(self.L.chisel_hip_pool_info(self.h, out))
        return {"committed": int(out[0]), "limit": int(out[1]), "grown": int(out[2]), "growable": bool(out[3])}

    def hash_table(self):
        """chisel_hip_debug_hash_table: the chunk hash and the slot tables as they stand (tests; one map, not a group) -- capacity,
        committed, free_top, hash_keys[capacity] (uint64), hash_vals[capacity], slot_key[committed], free_list[:free_top]"""
        info = (C.c_int64 * 4)()
        check(self.L.chisel_hip_debug_hash_table(self.h, info, None, None, None, None))
        cap, committed = int(info[0]), int(info[1])
        keys, vals = np.empty(cap, np.uint64), np.empty(cap, np.int32)
        slot_key, free_list = np.empty(committed, np.uint64), np.empty(committed, np.int32)
        check(self.L.chisel_hip_debug_hash_table(self.h, info, keys.ctypes.data, vals.ctypes.data, slot_key.ctypes.data, free_list.ctypes.data))
        assert (int(info[0]), int(info[1])) == (cap, committed)
        return {"capacity": cap, "committed": committed, "free_top": int(info[2]), "hash_keys": keys, "hash_vals": vals,
                "slot_key": slot_key, "free_list": free_list[:int(info[2])].copy()}

    def launch_stats(self, reset=False):
        """which shapes the launch heuristics picked (chisel_hip_get_launch_stats)"""
        out = (C.c_int64 * len(self.LAUNCH_STATS))()
        check(self.L.chisel_hip_get_launch_stats(self.h, out, int(reset)))
        return dict(zip(self.LAUNCH_STATS, [int(v) for v in out]))


class DepthFilter:
    """DepthFilter of the dense-mapping thread (server_pose_graph/src/dense_mapping/depth_filter.cpp) with its state in HBM."""
    A, B, INV_DEPTH, COV, RATIO, INV_DEPTH_MASKED, DEPTH = range(7)

    def __init__(self, height, width, device_id=-1):
        self.L = capi.load_library()
        self.shape = (int(height), int(width))
        self.h = C.c_void_p()
        check(self.L.chisel_hip_depth_filter_create(int(height), int(width), int(device_id), C.byref(self.h)))
        self._keep = None
        # the device the filter lives on: what a CUDA tensor handed to Update or read must live on
        dev = C.c_int(-1)
        check(self.L.chisel_hip_depth_filter_device(self.h, C.byref(dev)))
        self.device_id = dev.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.chisel_hip_depth_filter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _map_pointer(self, img, what):
        """-> (address, on_device, keepalive) of a float64 map of the filter's shape.  Host arrays (numpy, CPU torch) of any
        number type are converted; a CUDA tensor is read in place as doubles, so it must BE float64 and on the filter's device
        -- a float32 tensor of the right shape would be read past its end."""
        if not hasattr(img, "shape"):
            raise TypeError("%s: a numpy array or a torch tensor, not %s" % (what, type(img).__name__))
        if tuple(img.shape) != self.shape:
            raise ValueError("%s: shape %s, the filter's is %s" % (what, tuple(img.shape), self.shape))
        if not isinstance(img, np.ndarray) and getattr(img, "is_cuda", False):
            import torch
            if img.dtype != torch.float64:
                raise TypeError("%s: a CUDA tensor must be float64, not %s" % (what, img.dtype))
            if img.device.index != self.device_id:
                raise ValueError("%s: on %s, the filter is on cuda:%d" % (what, img.device, self.device_id))
        return _image_pointer(img, np.float64)

    def Update(self, update_mu, update_cov, reciprocal=False):
        """DepthFilter::Update(mUpdateMu, mUpdateCov): float64 maps (numpy or torch CUDA tensors); update_cov may be a scalar.
        Host maps are consumed when this returns; device maps are kept alive here until the next Update."""
        mu_addr, dev, k1 = self._map_pointer(update_mu, "update_mu")
        if np.isscalar(update_cov):
            check(self.L.chisel_hip_depth_filter_update(self.h, mu_addr, None, float(update_cov), int(reciprocal), dev))
            self._keep = [k1]
        else:
            cov_addr, dev2, k2 = self._map_pointer(update_cov, "update_cov")
            if dev2 != dev:
                raise ValueError("update_mu and update_cov: both on the host or both CUDA tensors")
            check(self.L.chisel_hip_depth_filter_update(self.h, mu_addr, cov_addr, 0.0, int(reciprocal), dev))
            self._keep = [k1, k2]

    def read(self, which, out=None):
        """-> float64 map; `out`: a torch CUDA tensor to fill in place (stays in HBM), default a new numpy array"""
        if out is not None:
            import torch
            if not (isinstance(out, torch.Tensor) and out.is_cuda):
                raise TypeError("out: a torch CUDA tensor, not %s" % type(out).__name__)
            if out.dtype != torch.float64:
                raise TypeError("out: must be float64, not %s" % out.dtype)
            if tuple(out.shape) != self.shape or not out.is_contiguous():
                raise ValueError("out: contiguous, of shape %s; got %s" % (self.shape, tuple(out.shape)))
            if out.device.index != self.device_id:
                raise ValueError("out: on %s, the filter is on cuda:%d" % (out.device, self.device_id))
            check(self.L.chisel_hip_depth_filter_read(self.h, int(which), out.data_ptr(), 1))
            return out
        a = np.empty(self.shape, np.float64)
        check(self.L.chisel_hip_depth_filter_read(self.h, int(which), a.ctypes.data, 0))
        return a

    def GetA(self):
        return self.read(self.A)

    def GetB(self):
        return self.read(self.B)

    def GetInvDepth(self):
        return self.read(self.INV_DEPTH)

    def GetCov(self):
        return self.read(self.COV)

    def GetRatio(self):
        return self.read(self.RATIO)


def stereo_homography(K1, K2, ref_rotation, ref_translation, match_rotation, match_translation):
    """StereoMapper::Update's plane-sweep transform (sgm_stereo_mapper.cpp:179-182): R = K2 R_m^T R_r K1^-1 and
    t = K2 R_m^T (t_r - t_m) in double, narrowed to float32 as ad_calc_cost's float arguments take them (:184-189).  Poses are
    camera-to-world (R_wc, t_wc).  K1^-1 is numpy's inverse where the reference uses cv::Mat::inv (LU): the last bit may differ."""
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    Rr, Rm = np.asarray(ref_rotation, np.float64), np.asarray(match_rotation, np.float64)
    tr, tm = np.asarray(ref_translation, np.float64).reshape(3), np.asarray(match_translation, np.float64).reshape(3)
    R = K2 @ Rm.T @ Rr @ np.linalg.inv(K1)
    t = K2 @ Rm.T @ (tr - tm)
    return R.astype(np.float32), t.astype(np.float32)


def stereo_default_params():
    """-> capi.StereoParams with the reference's constants (chisel_hip_stereo_default_params)"""
    p = capi.StereoParams()
    capi.load_library().chisel_hip_stereo_default_params(C.byref(p))
    return p


def _float32_image(img, shape, what):
    """-> (address, on_device, keepalive) of a float32 (h, w) map: numpy arrays of any float type are converted, torch CUDA
    tensors are used in place and must therefore BE float32 (a float64 or half tensor would be read as float32)"""
    assert tuple(img.shape) == shape, "%s: shape %s, the mapper's is %s" % (what, tuple(img.shape), shape)
    if not isinstance(img, np.ndarray) and getattr(img, "is_cuda", False):
        import torch
        assert img.dtype == torch.float32, "%s: a CUDA tensor must be float32, not %s" % (what, img.dtype)
    return _image_pointer(img, np.float32)


def _uint8_image(img, shape, what):
    """-> (address, on_device, keepalive) of a uint8 (h, w) image, a numpy array or a torch tensor (CUDA: used in place)"""
    assert tuple(img.shape) == shape, "%s: shape %s, expected %s" % (what, tuple(img.shape), shape)
    if isinstance(img, np.ndarray):
        assert img.dtype == np.uint8, "%s: a mono8 image must be uint8, not %s" % (what, img.dtype)
    else:
        import torch
        assert img.dtype == torch.uint8, "%s: a mono8 image must be uint8, not %s" % (what, img.dtype)
    return _image_pointer(img, np.uint8)


def _doubles(a, n, what):
    a = np.asarray(a, np.float64).reshape(-1)
    assert a.size == n, "%s: %d values, expected %d" % (what, a.size, n)
    return (C.c_double * n)(*a.tolist())


def _intrinsics4(K):
    """(fx, fy, cx, cy) from a 3 x 3 camera matrix or a 4-vector"""
    K = np.asarray(K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(4))


class StereoMapper:
    """StereoMapper of the dense-mapping thread (server_pose_graph/src/dense_mapping/sgm_stereo_mapper.cpp) with its cost and SGM
    volumes in HBM (chisel_hip_stereo_*).  Two ways in: InitReference / Update / Output take the caller's already resized and
    undistorted float32 (height, width) maps; InitIntrinsic then InitReferenceImage / UpdateImage / BindSparsePoints / OutputImage
    take the camera's mono8 frames and do the resize, undistort, P2 map, gradient masks, sparse prior and final resize on the
    device.  Images are numpy arrays or torch CUDA tensors."""
    COST, SGM, DEPTH, DEPTH64, DEPTH_REAL, DEPTH_REAL64 = range(6)
    # chisel_hip_debug_stereo_prep read-outs
    PREP_REF, PREP_MATCH, PREP_P2W, PREP_MASK_X, PREP_MASK_Y, PREP_SPARSE_DEPTH, PREP_SPARSE_DIST = range(7)
    DEP_CNT = 128

    def __init__(self, width, height, params=None, device_id=-1):
        self.L = capi.load_library()
        self.shape = (int(height), int(width))
        self.h = C.c_void_p()
        check(self.L.chisel_hip_stereo_create(int(width), int(height), C.byref(params) if params is not None else None, int(device_id),
                                              C.byref(self.h)))
        self._keep = None

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.chisel_hip_stereo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def InitReference(self, ref_image, p2_weight):
        """InitReference (:55-123): the undistorted reference image and its P2 weight map; the measurement count restarts"""
        a, dev, k1 = _float32_image(ref_image, self.shape, "ref_image")
        b, dev2, k2 = _float32_image(p2_weight, self.shape, "p2_weight")
        assert dev == dev2, "ref_image and p2_weight must both be on the host or both on the device"
        check(self.L.chisel_hip_stereo_set_reference(self.h, a, b, dev))
        self._keep = [k1, k2]

    def Update(self, match_image, R, t):
        """Update (:125-199): R, t as stereo_homography returns them"""
        a, dev, k1 = _float32_image(match_image, self.shape, "match_image")
        Rf = (C.c_float * 9)(*np.asarray(R, np.float32).reshape(9).tolist())
        tf = (C.c_float * 3)(*np.asarray(t, np.float32).reshape(3).tolist())
        check(self.L.chisel_hip_stereo_update(self.h, a, Rf, tf, dev))
        self._keep = [k1]

    def Output(self, sparse_depth=None, sparse_dist=None, out=None):
        """Output (:219-385) up to the device depth map: FuseSparseInfo (when given the sparse maps), SGM, filterCost.  Returns
        the float32 depth map (numpy), or fills `out` (a torch CUDA tensor, float32 or float64) in place"""
        if sparse_depth is None:
            check(self.L.chisel_hip_stereo_output(self.h, None, None, 0))
        else:
            a, dev, k1 = _float32_image(sparse_depth, self.shape, "sparse_depth")
            b, dev2, k2 = _float32_image(sparse_dist, self.shape, "sparse_dist")
            assert dev == dev2, "sparse_depth and sparse_dist must both be on the host or both on the device"
            check(self.L.chisel_hip_stereo_output(self.h, a, b, dev))
            self._keep = [k1, k2]
        if out is not None:
            return self.read(self.DEPTH64 if str(out.dtype).endswith("float64") else self.DEPTH, out=out)
        return self.read(self.DEPTH)

    def ClearRawCost(self):
        """ClearRawCost (:202-216): cost, SGM and depth zeroed, the measurement count kept"""
        check(self.L.chisel_hip_stereo_clear(self.h))

    def read(self, which, out=None):
        """which = COST / SGM (float32 (h, w, 128)), DEPTH (float32 (h, w)), DEPTH64 (float64 (h, w)), DEPTH_REAL / DEPTH_REAL64
        (the camera-size depth of the last OutputImage, float32 / float64); `out`: a torch CUDA tensor to fill in place (stays in
        HBM), default a new numpy array"""
        if out is not None:
            check(self.L.chisel_hip_stereo_read(self.h, int(which), out.data_ptr(), 1))
            return out
        shape = self.shape + (self.DEP_CNT,) if which in (self.COST, self.SGM) else self.shape
        if which in (self.DEPTH_REAL, self.DEPTH_REAL64):
            assert getattr(self, "real_shape", None) is not None, "InitIntrinsic first"
            shape = self.real_shape
        a = np.empty(shape, np.float64 if which in (self.DEPTH64, self.DEPTH_REAL64) else np.float32)
        check(self.L.chisel_hip_stereo_read(self.h, int(which), a.ctypes.data, 0))
        return a

    # ---- the raw-image path ----
    def InitIntrinsic(self, K1, D1, K2, D2, real_size):
        """InitIntrinsic (:20-52): K as a 3 x 3 matrix or (fx, fy, cx, cy) of the camera image, D = (k1, k2, p1, p2[, k3]);
        real_size = (width, height) of the camera images the raw entries take"""
        real_w, real_h = (int(v) for v in real_size)
        pad = lambda D: list(np.asarray(D, np.float64).reshape(-1)) + [0.0] * (5 - np.asarray(D).size)
        check(self.L.chisel_hip_stereo_set_camera(self.h, real_w, real_h, _doubles(_intrinsics4(K1), 4, "K1"), _doubles(pad(D1), 5, "D1"),
                                                  _doubles(_intrinsics4(K2), 4, "K2"), _doubles(pad(D2), 5, "D2")))
        self.real_shape = (real_h, real_w)

    def _raw(self, img, what):
        assert getattr(self, "real_shape", None) is not None, "%s before InitIntrinsic" % what
        return _uint8_image(img, self.real_shape, what)

    def InitReferenceImage(self, image):
        """InitReference (:55-123) on the camera's mono8 image (uint8 (real_h, real_w)): resize, undistort, P2 map, gradient
        masks on the device; the measurement count restarts"""
        a, dev, k = self._raw(image, "InitReferenceImage")
        check(self.L.chisel_hip_stereo_set_reference_image(self.h, a, self.real_shape[1], dev))
        self._keep = [k]

    def UpdateImage(self, image, ref_pose, match_pose):
        """Update (:125-199) on a mono8 match image; poses are camera-to-world (R_wc, t_wc)"""
        a, dev, k = self._raw(image, "UpdateImage")
        Rr, tr = ref_pose
        Rm, tm = match_pose
        check(self.L.chisel_hip_stereo_update_image(self.h, a, self.real_shape[1], _doubles(Rr, 9, "ref R"), _doubles(tr, 3, "ref t"),
                                                    _doubles(Rm, 9, "match R"), _doubles(tm, 3, "match t"), dev))
        self._keep = [k]

    def BindSparsePoints(self, depths, points):
        """BindSparsePoints (sgm_stereo_mapper.h:60-66): depths (n,) and points (n, 2) x, y in camera-image pixels"""
        d = np.ascontiguousarray(np.asarray(depths, np.float64).reshape(-1))
        p = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 2))
        assert len(d) == len(p), "%d depths for %d points" % (len(d), len(p))
        check(self.L.chisel_hip_stereo_bind_sparse_points(self.h, d.ctypes.data if len(d) else None, p.ctypes.data if len(p) else None,
                                                          len(d)))

    def OutputImage(self, out=None):
        """Output (:219-422) in full: sparse prior, FuseSparseInfo, SGM, WTA and the resize to the camera size.  Returns the
        float32 (real_h, real_w) depth (numpy), or fills `out` (a torch CUDA tensor, float32 or float64) in place"""
        assert getattr(self, "real_shape", None) is not None, "OutputImage before InitIntrinsic"
        check(self.L.chisel_hip_stereo_output_image(self.h))
        if out is not None:
            assert tuple(out.shape) == self.real_shape
            return self.read(self.DEPTH_REAL64 if str(out.dtype).endswith("float64") else self.DEPTH_REAL, out=out)
        return self.read(self.DEPTH_REAL)

    def debug_prep(self, which):
        """the prepared inputs (chisel_hip_debug_stereo_prep): PREP_* -> numpy (h, w), float32 or uint8 for the masks"""
        a = np.empty(self.shape, np.uint8 if which in (self.PREP_MASK_X, self.PREP_MASK_Y) else np.float32)
        check(self.L.chisel_hip_debug_stereo_prep(self.h, int(which), a.ctypes.data))
        return a


class DepthEstimator:
    """DepthEstimator (server_pose_graph/src/dense_mapping/depth_estimator.cpp) as ServerKeyFrame drives it: the constructor and
    Initialize (:165-188, :503-599) make a StereoMapper of the work size for the keyframe's camera size (k3 = 0) and a DepthFilter
    of the camera size; FuseNewFrame (:191-197) runs FuseNewFrameSGM -- UpdateImage, OutputImage into a float64 device map, the
    filter update with 1 / depth and cov_all = (3 DEP_SAMPLE)^2 (:276-297) -- and ClearRawCost, all in HBM.  PropogateDepth,
    Validate and RegularizeDepthMap are not built: their call sites are commented out in the reference."""

    def __init__(self, ref_image, ref_pose_wc, fx, fy, cx, cy, d1, d2, d3, d4, width=640, height=480, params=None, device_id=-1):
        import torch
        self.ref_pose_wc = (np.asarray(ref_pose_wc[0], np.float64), np.asarray(ref_pose_wc[1], np.float64))
        real_h, real_w = tuple(ref_image.shape)
        self.params = params if params is not None else stereo_default_params()
        self.mapper = StereoMapper(width, height, self.params, device_id)
        K = (fx, fy, cx, cy)
        D = (d1, d2, d3, d4, 0.0)                              # :588
        self.mapper.InitIntrinsic(K, D, K, D, (real_w, real_h))
        self.mapper.InitReferenceImage(ref_image)
        self.filter = DepthFilter(real_h, real_w, device_id)   # :184
        dev = device_id if device_id >= 0 else torch.cuda.current_device()
        self._depth = torch.empty((real_h, real_w), dtype=torch.float64, device="cuda:%d" % dev)
        ds = np.float32(self.params.dep_sample)
        self.cov_all = float((np.float32(3) * ds) * (np.float32(3) * ds))   # float arithmetic, widened (:293)
        self.observations = 0

    def BindSparsePoints(self, depths, points):
        """DepthEstimator::BindSparsePoints (depth_estimator.h:109-115)"""
        self.mapper.BindSparsePoints(depths, points)

    def FuseNewFrame(self, match_image, match_pose_wc):
        """FuseNewFrame (:191-197) = FuseNewFrameSGM (:209-299) + ClearRawCost, device-resident"""
        self.mapper.UpdateImage(match_image, self.ref_pose_wc, match_pose_wc)
        self.mapper.OutputImage(out=self._depth)
        self.filter.Update(self._depth, self.cov_all, reciprocal=True)
        self.mapper.ClearRawCost()
        self.observations += 1

    def GetInvDepth(self):
        return self.filter.GetInvDepth()

    def GetRatio(self):
        return self.filter.GetRatio()

    def GetCov(self):
        return self.filter.GetCov()

    def read(self, which, out=None):
        """the filter's maps (DepthFilter.read): DepthFilter.DEPTH is the depth map ServerKeyFrame integrates"""
        return self.filter.read(which, out=out)


def align_solve(terms, damping):
    """chisel_hip_align_solve: the Gauss-Newton step xi = (v, w), (6,) float64, of the normal equations `terms` (32 doubles as
    Chisel.AlignTerms gives them) with absolute damping per used pixel; host arithmetic, no GPU needed.  Degenerate equations raise
    ChiselHipError with code 5."""
    L = capi.load_library()
    t = np.ascontiguousarray(terms, np.float64).reshape(32)
    xi = np.zeros(6, np.float64)
    dp = C.POINTER(C.c_double)
    check(L.chisel_hip_align_solve(t.ctypes.data_as(dp), float(damping), xi.ctypes.data_as(dp)))
    return xi


def condition_depth(depth64, width=640, height=480, intrinsics=None):
    """CollaborativeServer::PublishDenseInfo's depth conditioning (chisel_hip_condition_depth): float64 depth map of any size
    -> (float32 depth of the publish size with NaN outside [0.1, 20] m, rescaled (fx, fy, cx, cy) or None)"""
    L = capi.load_library()
    src = np.ascontiguousarray(depth64, np.float64)
    h0, w0 = src.shape
    dst = np.empty((height, width), np.float32)
    K = (C.c_double * 4)(*(intrinsics if intrinsics is not None else (0.0, 0.0, 0.0, 0.0)))
    check(L.chisel_hip_condition_depth(src.ctypes.data, w0, h0, 0, dst.ctypes.data, width, height, 0, K, None))
    return dst, (tuple(K) if intrinsics is not None else None)


def condition_color(image, width=640, height=480):
    """PublishDenseInfo's cv::resize of the colour image (chisel_hip_condition_color): uint8 (H, W) or (H, W, 1 / 3 / 4) ->
    uint8 of the publish size, same channel count"""
    L = capi.load_library()
    src = np.ascontiguousarray(image, np.uint8)
    cn = 1 if src.ndim == 2 else src.shape[2]
    h0, w0 = src.shape[:2]
    dst = np.empty((height, width) if src.ndim == 2 else (height, width, cn), np.uint8)
    check(L.chisel_hip_condition_color(src.ctypes.data, w0, h0, cn, 0, dst.ctypes.data, width, height, 0, None))
    return dst


def publish_cloud(depth64, color):
    """CollaborativeServer::SendPointCloud (chisel_hip_publish_cloud): float64 depth (H, W) + uint8 colour image (H, W[, C]) ->
    the PointCloud2 data array as uint32 (H, W, 4): x, y, z float bits and the packed grey rgb"""
    L = capi.load_library()
    d = np.ascontiguousarray(depth64, np.float64)
    c = np.ascontiguousarray(color, np.uint8)
    h, w = d.shape
    step = c.size // h
    out = np.empty((h, w, 4), np.uint32)
    check(L.chisel_hip_publish_cloud(d.ctypes.data, c.ctypes.data, w, h, step, 0, out.ctypes.data, 0, None))
    return out


def chunk_owner(cid, n_shards, shard_block=2):
    c = (C.c_int * 3)(*[int(v) for v in cid])
    return capi.load_library().chisel_hip_chunk_owner(c, int(n_shards), int(shard_block))


def mesh_shell_plan(entries, n_shards, rank, shard_block=2):
    """chisel_hip_mesh_shell_plan: entries (n, 4) int32 (x, y, z, flag) -> (jobs (nj, 3), items (ni, 5): owner, x, y, z, box)"""
    L = capi.load_library()
    e = np.ascontiguousarray(np.asarray(entries, np.int32).reshape(-1, 4))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None
    nj, ni = C.c_int64(0), C.c_int64(0)
    check(L.chisel_hip_mesh_shell_plan(ip(e), len(e), int(n_shards), int(rank), int(shard_block), None, 0, C.byref(nj), None, 0, C.byref(ni)))
    jobs, items = np.zeros((nj.value, 3), np.int32), np.zeros((ni.value, 5), np.int32)
    check(L.chisel_hip_mesh_shell_plan(ip(e), len(e), int(n_shards), int(rank), int(shard_block), ip(jobs), nj.value, C.byref(nj), ip(items), ni.value,
                                       C.byref(ni)))
    return jobs, items


def shell_volume(box, chunk_edge):
    return int(capi.load_library().chisel_hip_shell_volume(int(box), int(chunk_edge)))

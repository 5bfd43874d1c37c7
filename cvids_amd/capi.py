"""ctypes bindings of include/chisel_hip.h (the drop-in C ABI)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHISEL_HIP_LIB selects a diagnostic build (e.g. libchisel_hip_stamps.so); the default is the product library
_LIB = os.path.join(_HERE, os.environ.get("CHISEL_HIP_LIB", "libchisel_hip.so"))

ABI_VERSION = 3  # CHISEL_HIP_ABI_VERSION of include/chisel_hip.h this mirror was written against (tests/test_abi.py compares)
NUM_COUNTERS = 9
COUNTER_NAMES = ["sdf", "col", "col_sat", "probe", "carved", "work_chunks", "new_chunks", "updated_chunks", "frames"]
NUM_KERNELS = 6
KERNEL_NAMES = ["pyramid", "cull", "integrate", "mesh", "resolve", "cloud"]
TRUNC_CONSTANT, TRUNC_INVERSE, TRUNC_QUADRATIC = 0, 1, 2
STATUS = {0: "OK", 1: "ERR_INVALID", 2: "ERR_HIP", 3: "ERR_POOL_FULL", 4: "ERR_NOT_FOUND", 5: "ERR_UNSUPPORTED", 6: "ERR_IO"}


class ChiselHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("chisel_hip: %s (%d): %s" % (STATUS.get(code, "?"), code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("chunk_size", C.c_int * 3), ("voxel_resolution", C.c_float), ("use_color", C.c_int),
                ("device_id", C.c_int), ("max_chunks", C.c_int64), ("n_shards", C.c_int), ("shard_rank", C.c_int),
                ("shard_block", C.c_int)]


class Integrator(C.Structure):
    _fields_ = [("truncator_kind", C.c_int), ("truncator_param", C.c_float), ("weight", C.c_float),
                ("carving_enabled", C.c_int), ("carving_dist", C.c_float)]


class DepthFrame(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("on_device", C.c_int),
                ("pose", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_plane", C.c_float), ("far_plane", C.c_float)]


class ColorFrame(C.Structure):
    _fields_ = [("color", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int),
                ("on_device", C.c_int), ("pose", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float)]


class PointCloud(C.Structure):
    _fields_ = [("points", C.c_void_p), ("colors", C.c_void_p), ("n_points", C.c_int64), ("on_device", C.c_int),
                ("pose", C.c_float * 12), ("truncation", C.c_float), ("max_dist", C.c_float)]


# every symbol include/chisel_hip.h declares (tests/test_abi.py checks the header against this list)
class Statistics(C.Structure):
    """chisel_hip_statistics (include/chisel_hip.h): ChunkManager::PrintMemoryStatistics' census"""
    _fields_ = [("n_unknown", C.c_int64), ("n_known_inside", C.c_int64), ("n_known_outside", C.c_int64), ("total_weight", C.c_double),
                ("n_chunks", C.c_int64), ("id_min", C.c_int32 * 3), ("id_max", C.c_int32 * 3)]


class StereoParams(C.Structure):
    """chisel_hip_stereo_params (include/chisel_hip.h): dense_mapping_parameters.cpp:3-11 and DEP_SAMPLE"""
    _fields_ = [(n, C.c_float) for n in ("pi1", "pi2", "tau_so", "sgm_q1", "sgm_q2", "var_scale", "sparse_ratio", "dep_sample")]


class View(C.Structure):
    """chisel_hip_view (include/chisel_hip.h): the camera of chisel_hip_render_view"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pose", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("near_plane", C.c_float), ("far_plane", C.c_float), ("step", C.c_float)]


class Ray(C.Structure):
    """chisel_hip_ray (include/chisel_hip.h): one ray of chisel_hip_cast_rays, 32 bytes"""
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("t_near", C.c_float), ("t_far", C.c_float)]


RAY_MAX_SAMPLES = 65536  # CHISEL_HIP_RAY_MAX_SAMPLES


class AlignParams(C.Structure):
    """chisel_hip_align_params (include/chisel_hip.h): the loop of chisel_hip_align_depth, 40 bytes"""
    _fields_ = [("max_iterations", C.c_int), ("min_pixels", C.c_int), ("max_residual", C.c_float), ("reserved", C.c_float),
                ("damping", C.c_double), ("min_translation", C.c_double), ("min_rotation", C.c_double)]


class AlignResult(C.Structure):
    """chisel_hip_align_result (include/chisel_hip.h), 664 bytes"""
    _fields_ = [("pose", C.c_double * 12), ("xi_last", C.c_double * 6), ("terms_first", C.c_double * 32), ("terms_last", C.c_double * 32),
                ("iterations", C.c_int), ("status", C.c_int)]


class MergeStats(C.Structure):
    """chisel_hip_merge_stats (include/chisel_hip.h): what chisel_hip_merge_map did, 32 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("src_chunks", "dst_chunks_created", "dst_chunks_updated", "voxels_updated")]


class DeintegrateStats(C.Structure):
    """chisel_hip_deintegrate_stats (include/chisel_hip.h): what chisel_hip_deintegrate_depth / _batch did, 48 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("chunks_tested", "chunks_touched", "chunks_emptied", "voxels_updated", "voxels_cleared", "voxels_skipped")]


class DistanceWindow(C.Structure):
    """chisel_hip_distance_window (include/chisel_hip.h): the window of chisel_hip_distance_field, 36 bytes"""
    _fields_ = [("origin", C.c_int * 3), ("dims", C.c_int * 3), ("radius", C.c_int), ("unknown_is_obstacle", C.c_int),
                ("surface_offset", C.c_float)]


DISTANCE_MAX_RADIUS = 64  # chisel_hip_distance_field's largest radius, voxels


class FrontierWindow(C.Structure):
    """chisel_hip_frontier_window (include/chisel_hip.h): the window and the knobs of chisel_hip_frontiers, 40 bytes"""
    _fields_ = [("origin", C.c_int * 3), ("dims", C.c_int * 3), ("min_unknown_faces", C.c_int), ("connectivity", C.c_int), ("min_voxels", C.c_int),
                ("surface_offset", C.c_float)]


class FrontierTotals(C.Structure):
    """chisel_hip_frontier_totals (include/chisel_hip.h): what chisel_hip_frontiers found and kept, 64 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("unknown", "free", "occupied", "frontier", "clusters", "largest_voxels", "kept_clusters", "kept_voxels")]


assert C.sizeof(FrontierWindow) == 40 and C.sizeof(FrontierTotals) == 64
FRONTIER_MAX_VOXELS = 1 << 26  # chisel_hip_frontiers' largest window, voxels
FRONTIER_TABLE_COLUMNS = ("root", "voxels", "sum_x", "sum_y", "sum_z", "min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "unknown_faces")


class TravelWindow(C.Structure):
    """chisel_hip_travel_window (include/chisel_hip.h): the window and the request of chisel_hip_travel_field, 56 bytes"""
    _fields_ = [("origin", C.c_int * 3), ("dims", C.c_int * 3), ("connectivity", C.c_int), ("step_cost", C.c_int * 3), ("max_cost", C.c_int),
                ("clearance", C.c_int), ("unknown_is_obstacle", C.c_int), ("surface_offset", C.c_float)]


TRAVEL_TOTALS = ("unknown", "free", "occupied", "traversable", "seeds_used", "seeds_ignored", "reached", "largest_cost", "targets_reached",
                 "targets_ignored", "rounds", "tile_visits")  # the last two: diagnostics of the implementation


class TravelTotals(C.Structure):
    """chisel_hip_travel_totals (include/chisel_hip.h): what chisel_hip_travel_field found, 96 bytes"""
    _fields_ = [(n, C.c_int64) for n in TRAVEL_TOTALS]


assert C.sizeof(TravelWindow) == 56 and C.sizeof(TravelTotals) == 96
TRAVEL_TABLE_COLUMNS = ("rows", "reached", "least_cost", "least_index")
TRAVEL_ROUNDS_PER_WAIT = 16  # travel_checks.h: round launches between two looks at the flagged tiles
TRAVEL_MAX_SEEDS = 1 << 20
TRAVEL_MAX_COST = 1 << 30


class MeshRequest(C.Structure):
    """chisel_hip_mesh_request (include/chisel_hip.h): the selection and the marker colours of chisel_hip_gather_meshes, 56 bytes"""
    _fields_ = [("ids_xyz", C.POINTER(C.c_int)), ("n_ids", C.c_int64), ("marker_colors", C.c_int), ("light0", C.c_float * 3),
                ("light1", C.c_float * 3), ("diffuse", C.c_float), ("ambient", C.c_float)]


class MeshTotals(C.Structure):
    """chisel_hip_mesh_totals (include/chisel_hip.h): what a selection of chisel_hip_gather_meshes holds, 48 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("meshes", "meshes_nonempty", "vertices", "grids", "arenas_read", "tiles")]


GATHER_TILE_FLOATS = 4096  # CHISEL_HIP_GATHER_TILE_FLOATS


class ChunkRequest(C.Structure):
    """chisel_hip_chunk_request (include/chisel_hip.h): the selection of chisel_hip_gather_chunks, 48 bytes"""
    _fields_ = [("ids_xyz", C.POINTER(C.c_int)), ("n_ids", C.c_int64), ("use_box", C.c_int), ("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3)]


assert C.sizeof(ChunkRequest) == 48
CHUNK_TILE_BYTES = 16384  # bytes of one packed array one workgroup of the chunk copy kernels moves (kernels_chunks.h: CHUNK_TILE_QUADS * 16)


class CoarseRequest(C.Structure):
    """chisel_hip_coarse_request (include/chisel_hip.h): the selection, the stride and the stages of chisel_hip_coarse_mesh, 56 bytes"""
    _fields_ = [("chunks", ChunkRequest), ("stride", C.c_int), ("stages", C.c_int)]


class CoarseTotals(C.Structure):
    """chisel_hip_coarse_totals (include/chisel_hip.h): what a coarse mesh of a selection holds, 32 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("chunks", "chunks_nonempty", "cubes_meshed", "vertices")]


assert C.sizeof(CoarseRequest) == 56 and C.sizeof(CoarseTotals) == 32


class IndexedTotals(C.Structure):
    """chisel_hip_indexed_totals (include/chisel_hip.h): what an indexed mesh of a selection holds, 40 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("chunks", "owners", "cubes_meshed", "vertices", "triangles")]


assert C.sizeof(IndexedTotals) == 40


class ComponentsTotals(C.Structure):
    """chisel_hip_components_totals (include/chisel_hip.h): what chisel_hip_mesh_components / _filter_mesh found and kept, 64 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("vertices", "triangles", "invalid_triangles", "components", "largest_triangles", "kept_components",
                                         "kept_vertices", "kept_triangles")]


assert C.sizeof(ComponentsTotals) == 64


class AdjacencyTotals(C.Structure):
    """chisel_hip_adjacency_totals (include/chisel_hip.h): what chisel_hip_mesh_adjacency / _mesh_vertex_normals / _smooth_mesh found, 96 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("vertices", "triangles", "invalid_triangles", "incidences", "neighbors", "max_incident", "max_neighbors",
                                         "boundary_vertices", "nonmanifold_vertices", "isolated_vertices", "pinned_vertices", "reserved")]


assert C.sizeof(AdjacencyTotals) == 96
MESH_MAX_INCIDENT = 32  # CHISEL_HIP_MESH_MAX_INCIDENT
MESH_BOUNDARY, MESH_NONMANIFOLD, MESH_ISOLATED = 1, 2, 4  # CHISEL_HIP_MESH_*

ALIGN_CONVERGED, ALIGN_ITERATION_LIMIT, ALIGN_TOO_FEW_PIXELS, ALIGN_DEGENERATE = 0, 1, 2, 3  # CHISEL_HIP_ALIGN_*
ALIGN_STATUS = {0: "CONVERGED", 1: "ITERATION_LIMIT", 2: "TOO_FEW_PIXELS", 3: "DEGENERATE"}


EXPORTS = [
    "chisel_hip_abi_version", "chisel_hip_last_error", "chisel_hip_device_count", "chisel_hip_host_alloc", "chisel_hip_host_free", "chisel_hip_create",
    "chisel_hip_destroy", "chisel_hip_reset", "chisel_hip_set_integrator", "chisel_hip_set_stream",
    "chisel_hip_synchronize", "chisel_hip_wait_event", "chisel_hip_record_event", "chisel_hip_order_stream_after_map", "chisel_hip_order_map_after_stream", "chisel_hip_integrate_depth", "chisel_hip_integrate_depth_color",
    "chisel_hip_integrate_batch", "chisel_hip_integrate_pointcloud", "chisel_hip_garbage_collect", "chisel_hip_update_meshes", "chisel_hip_num_chunks",
    "chisel_hip_list_chunks", "chisel_hip_has_chunk", "chisel_hip_download_chunk", "chisel_hip_upload_chunk",
    "chisel_hip_meshes_to_update", "chisel_hip_meshes_to_update_since", "chisel_hip_meshes_to_update_prefetch", "chisel_hip_shell_plan_device", "chisel_hip_shell_segment_bytes", "chisel_hip_export_shells_packed", "chisel_hip_import_shells_packed", "chisel_hip_update_meshes_planned", "chisel_hip_shell_plan_queue", "chisel_hip_import_shells_fixed", "chisel_hip_shell_commit", "chisel_hip_num_meshes", "chisel_hip_list_meshes", "chisel_hip_mesh_size",
    "chisel_hip_download_mesh", "chisel_hip_get_sdf", "chisel_hip_get_sdf_and_gradient", "chisel_hip_save_ply",
    "chisel_hip_save_map", "chisel_hip_load_map",
    "chisel_hip_drop_ghost_chunks", "chisel_hip_update_meshes_of", "chisel_hip_condition_depth", "chisel_hip_condition_color", "chisel_hip_publish_cloud",
    "chisel_hip_depth_filter_create", "chisel_hip_depth_filter_destroy", "chisel_hip_depth_filter_update", "chisel_hip_depth_filter_read",
    "chisel_hip_depth_filter_device",
    "chisel_hip_stereo_default_params", "chisel_hip_stereo_create", "chisel_hip_stereo_destroy", "chisel_hip_stereo_set_reference",
    "chisel_hip_stereo_update", "chisel_hip_stereo_output", "chisel_hip_stereo_clear", "chisel_hip_stereo_read",
    "chisel_hip_stereo_set_camera", "chisel_hip_stereo_set_reference_image", "chisel_hip_stereo_update_image",
    "chisel_hip_stereo_bind_sparse_points", "chisel_hip_stereo_output_image", "chisel_hip_stereo_homography",
    "chisel_hip_get_counters", "chisel_hip_memory_statistics", "chisel_hip_topology_epoch", "chisel_hip_candidates", "chisel_hip_cloud_candidates", "chisel_hip_mesh_cube", "chisel_hip_write_mesh_ply", "chisel_hip_shade_vertices", "chisel_hip_generate_mesh", "chisel_hip_recompute_mesh", "chisel_hip_integrate_chunk", "chisel_hip_dirty_ids_device", "chisel_hip_mesh_shell_plan",
    "chisel_hip_shell_volume", "chisel_hip_set_profiling", "chisel_hip_get_profile", "chisel_hip_get_launch_stats", "chisel_hip_pool_info", "chisel_hip_mc_tables", "chisel_hip_mesh_cube_values", "chisel_hip_interpolate_vertex", "chisel_hip_raycast", "chisel_hip_chunk_owner", "chisel_hip_frustum", "chisel_hip_frustum_from_vectors", "chisel_hip_create_group", "chisel_hip_render_view",
    "chisel_hip_query_points", "chisel_hip_cast_rays", "chisel_hip_align_terms", "chisel_hip_align_solve", "chisel_hip_align_depth",
    "chisel_hip_merge_map", "chisel_hip_deintegrate_depth", "chisel_hip_deintegrate_batch", "chisel_hip_distance_field",
    "chisel_hip_gather_meshes", "chisel_hip_gather_meshes_size", "chisel_hip_save_ply_binary",
    "chisel_hip_gather_chunks", "chisel_hip_scatter_chunks", "chisel_hip_coarse_mesh", "chisel_hip_indexed_mesh",
    "chisel_hip_mesh_components", "chisel_hip_filter_mesh",
    "chisel_hip_mesh_adjacency", "chisel_hip_mesh_vertex_normals", "chisel_hip_smooth_mesh",
    "chisel_hip_frontiers", "chisel_hip_travel_field", "chisel_hip_travel_path",
]
# the device self-tests and debug read-outs include/chisel_hip_selftest.h declares
SELFTEST_EXPORTS = [
    "chisel_hip_kat_truncation", "chisel_hip_kat_dist", "chisel_hip_kat_color", "chisel_hip_kat_color_fresh", "chisel_hip_kat_color_any",
    "chisel_hip_kat_reciprocal", "chisel_hip_kat_floor", "chisel_hip_kat_raycast", "chisel_hip_debug_cloud_stats",
    "chisel_hip_debug_cull_space", "chisel_hip_debug_frustum_range", "chisel_hip_debug_stereo_prep", "chisel_hip_debug_hash_table",
]


def library_path():
    return _LIB


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of cvids_amd/csrc (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    if not force and os.path.exists(_LIB):
        newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir))
        newest = max(newest, os.path.getmtime(os.path.join(_HERE, "..", "include", "chisel_hip.h")))
        if os.path.getmtime(_LIB) >= newest:
            return _LIB
    subprocess.check_call(["make", "-C", src_dir])
    return _LIB


_lib = None


def load_library():
    """Load libchisel_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise ChiselHipError(2, "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback)" % _LIB)
    # torch bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP runtimes in one process do not
    # work ("No HIP GPUs are available" in whichever comes second), so when torch is installed let it load its
    # runtime first; libchisel_hip.so then binds to that copy.  A C++ host without torch uses /opt/rocm's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB)
    if L.chisel_hip_abi_version() != ABI_VERSION:  # array lengths and signatures below are this version's: no call into another
        raise ChiselHipError(2, "%s has ABI version %d, these bindings are for %d: rebuild (`make -C cvids_amd/csrc`)" % (_LIB, L.chisel_hip_abi_version(), ABI_VERSION))
    vp, i32p, f32p, u8p, i64p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    L.chisel_hip_last_error.restype = C.c_char_p
    L.chisel_hip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.chisel_hip_create_group.argtypes = [C.POINTER(Config), i32p, C.c_int, C.POINTER(vp)]
    L.chisel_hip_destroy.argtypes = [vp]
    L.chisel_hip_reset.argtypes = [vp]
    L.chisel_hip_set_integrator.argtypes = [vp, C.POINTER(Integrator)]
    L.chisel_hip_set_stream.argtypes = [vp, vp]
    L.chisel_hip_synchronize.argtypes = [vp]
    L.chisel_hip_integrate_depth.argtypes = [vp, C.POINTER(DepthFrame)]
    L.chisel_hip_integrate_depth_color.argtypes = [vp, C.POINTER(DepthFrame), C.POINTER(ColorFrame)]
    L.chisel_hip_integrate_batch.argtypes = [vp, C.c_int, C.POINTER(DepthFrame), C.POINTER(ColorFrame)]
    L.chisel_hip_integrate_pointcloud.argtypes = [vp, C.POINTER(PointCloud)]
    L.chisel_hip_garbage_collect.argtypes = [vp, i32p, C.c_int]
    L.chisel_hip_update_meshes.argtypes = [vp, C.c_int]
    L.chisel_hip_num_chunks.argtypes = [vp, i64p]
    L.chisel_hip_list_chunks.argtypes = [vp, i32p, C.c_int64, i64p]
    L.chisel_hip_has_chunk.argtypes = [vp, i32p, i32p]
    L.chisel_hip_download_chunk.argtypes = [vp, i32p, f32p, f32p, u8p]
    L.chisel_hip_upload_chunk.argtypes = [vp, i32p, f32p, f32p, u8p]
    L.chisel_hip_meshes_to_update.argtypes = [vp, i32p, C.c_int64, i64p]
    L.chisel_hip_meshes_to_update_since.argtypes = [vp, C.POINTER(C.c_uint64), i32p, C.c_int64, i64p, i32p]
    L.chisel_hip_meshes_to_update_prefetch.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.chisel_hip_host_alloc.argtypes = [C.c_size_t]
    L.chisel_hip_host_alloc.restype = C.c_void_p
    L.chisel_hip_host_free.argtypes = [vp]
    L.chisel_hip_host_free.restype = None
    L.chisel_hip_num_meshes.argtypes = [vp, i64p]
    L.chisel_hip_list_meshes.argtypes = [vp, i32p, C.c_int64, i64p]
    L.chisel_hip_mesh_size.argtypes = [vp, i32p, i64p, i64p]
    L.chisel_hip_download_mesh.argtypes = [vp, i32p, f32p, f32p, f32p, f32p]
    L.chisel_hip_get_sdf.argtypes = [vp, f32p, C.POINTER(C.c_double), i32p]
    L.chisel_hip_get_sdf_and_gradient.argtypes = [vp, f32p, C.POINTER(C.c_double), f32p, i32p]
    L.chisel_hip_save_ply.argtypes = [vp, C.c_char_p]
    L.chisel_hip_drop_ghost_chunks.argtypes = [vp]
    L.chisel_hip_condition_depth.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), vp]
    L.chisel_hip_condition_color.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]
    L.chisel_hip_publish_cloud.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]
    L.chisel_hip_update_meshes_of.argtypes = [vp, i32p, C.c_int]
    L.chisel_hip_depth_filter_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.chisel_hip_depth_filter_destroy.argtypes = [vp]
    L.chisel_hip_depth_filter_update.argtypes = [vp, vp, vp, C.c_double, C.c_int, C.c_int]
    L.chisel_hip_depth_filter_read.argtypes = [vp, C.c_int, vp, C.c_int]
    L.chisel_hip_depth_filter_device.argtypes = [vp, C.POINTER(C.c_int)]
    L.chisel_hip_stereo_default_params.argtypes = [C.POINTER(StereoParams)]
    L.chisel_hip_stereo_default_params.restype = None
    L.chisel_hip_stereo_create.argtypes = [C.c_int, C.c_int, C.POINTER(StereoParams), C.c_int, C.POINTER(vp)]
    L.chisel_hip_stereo_destroy.argtypes = [vp]
    L.chisel_hip_stereo_set_reference.argtypes = [vp, vp, vp, C.c_int]
    L.chisel_hip_stereo_update.argtypes = [vp, vp, f32p, f32p, C.c_int]
    L.chisel_hip_stereo_output.argtypes = [vp, vp, vp, C.c_int]
    L.chisel_hip_stereo_clear.argtypes = [vp]
    L.chisel_hip_stereo_read.argtypes = [vp, C.c_int, vp, C.c_int]
    f64p = C.POINTER(C.c_double)
    L.chisel_hip_stereo_set_camera.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, f64p, f64p]
    L.chisel_hip_stereo_set_reference_image.argtypes = [vp, vp, C.c_int, C.c_int]
    L.chisel_hip_stereo_update_image.argtypes = [vp, vp, C.c_int, f64p, f64p, f64p, f64p, C.c_int]
    L.chisel_hip_stereo_bind_sparse_points.argtypes = [vp, vp, vp, C.c_int]
    L.chisel_hip_stereo_output_image.argtypes = [vp]
    L.chisel_hip_stereo_homography.argtypes = [f64p, f64p, f64p, f64p, f64p, f64p, f32p, f32p]
    L.chisel_hip_debug_stereo_prep.argtypes = [vp, C.c_int, vp]
    L.chisel_hip_save_map.argtypes = [vp, C.c_char_p]
    L.chisel_hip_load_map.argtypes = [vp, C.c_char_p]
    L.chisel_hip_get_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.chisel_hip_set_profiling.argtypes = [vp, C.c_int]
    if hasattr(L, "chisel_hip_candidates"):
        L.chisel_hip_topology_epoch.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.chisel_hip_candidates.argtypes = [f32p, f32p, i32p, C.c_float, i32p, C.c_int64, i64p]
        L.chisel_hip_cloud_candidates.argtypes = [vp, C.POINTER(PointCloud), i32p, C.c_int64, i64p]
        L.chisel_hip_mesh_cube.argtypes = [vp, i32p, i32p, f32p, f32p, f32p, i32p, i32p]
        L.chisel_hip_write_mesh_ply.argtypes = [C.c_char_p, f32p, f32p, C.c_int64, i64p, C.c_int64]
        L.chisel_hip_shade_vertices.argtypes = [vp, f32p, C.c_int64, f32p, f32p, C.c_int]
        L.chisel_hip_integrate_chunk.argtypes = [vp, i32p, C.POINTER(DepthFrame), C.POINTER(ColorFrame), i32p]
        L.chisel_hip_recompute_mesh.argtypes = [vp, i32p]
        L.chisel_hip_dirty_ids_device.argtypes = [vp, vp, C.c_int]
        L.chisel_hip_shell_plan_device.argtypes = [vp, vp, C.c_int, C.c_int, i64p]
        L.chisel_hip_shell_segment_bytes.argtypes = [vp, C.c_int64, C.c_int64]
        L.chisel_hip_shell_segment_bytes.restype = C.c_int64
        L.chisel_hip_export_shells_packed.argtypes = [vp, vp, C.c_int64]
        L.chisel_hip_import_shells_packed.argtypes = [vp, vp, C.c_int64]
        L.chisel_hip_update_meshes_planned.argtypes = [vp]
        L.chisel_hip_shell_plan_queue.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, vp, vp, C.c_int]
        L.chisel_hip_import_shells_fixed.argtypes = [vp, vp, C.c_int64, vp, C.c_int, C.c_int]
        L.chisel_hip_shell_commit.argtypes = [vp, C.c_int]
        L.chisel_hip_mesh_shell_plan.argtypes = [i32p, C.c_int64, C.c_int, C.c_int, C.c_int, i32p, C.c_int64, i64p, i32p, C.c_int64, i64p]
        L.chisel_hip_shell_volume.argtypes = [C.c_int, C.c_int]
        L.chisel_hip_shell_volume.restype = C.c_int64
        L.chisel_hip_generate_mesh.argtypes = [vp, i32p, C.c_int, C.c_int64, C.c_int64, f32p, f32p, f32p, f32p, i64p, i64p]
    if hasattr(L, "chisel_hip_memory_statistics"):
        L.chisel_hip_memory_statistics.argtypes = [vp, C.POINTER(Statistics)]
    L.chisel_hip_render_view.argtypes = [vp, C.POINTER(View), vp, vp, vp, C.c_int]
    L.chisel_hip_get_profile.argtypes = [vp, C.POINTER(C.c_double), i64p, C.c_int]
    L.chisel_hip_get_launch_stats.argtypes = [vp, i64p, C.c_int]
    L.chisel_hip_pool_info.argtypes = [vp, i64p]
    L.chisel_hip_chunk_owner.argtypes = [i32p, C.c_int, C.c_int]
    L.chisel_hip_kat_truncation.argtypes = [C.c_int, C.c_float, f32p, C.c_int, f32p, f32p]
    L.chisel_hip_kat_dist.argtypes = [f32p, C.c_int, f32p]
    L.chisel_hip_kat_color.argtypes = [u8p, C.c_int, u8p]
    # entry points added after ABI version 1 was first built (an older library simply lacks them: A/B runs of tools/)
    for name, types in (("chisel_hip_wait_event", [vp, vp]), ("chisel_hip_record_event", [vp, vp]),
                        ("chisel_hip_order_stream_after_map", [vp, vp]), ("chisel_hip_order_map_after_stream", [vp, vp]),
                        ("chisel_hip_query_points", [vp, vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int]),
                        ("chisel_hip_cast_rays", [vp, vp, C.c_int64, C.c_float, vp, vp, vp, vp, C.c_int]),
                        ("chisel_hip_align_terms", [vp, C.POINTER(DepthFrame), C.c_float, vp, C.c_int]),
                        ("chisel_hip_align_solve", [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]),
                        ("chisel_hip_align_depth", [vp, C.POINTER(DepthFrame), C.POINTER(AlignParams), C.POINTER(AlignResult)]),
                        ("chisel_hip_merge_map", [vp, vp, f32p, C.POINTER(MergeStats)]),
                        ("chisel_hip_deintegrate_depth", [vp, C.POINTER(DepthFrame), C.c_int, C.POINTER(DeintegrateStats), i32p, C.c_int]),
                        ("chisel_hip_deintegrate_batch", [vp, C.c_int, C.POINTER(DepthFrame), C.c_int, C.POINTER(DeintegrateStats), i32p, C.c_int]),
                        ("chisel_hip_distance_field", [vp, C.POINTER(DistanceWindow), vp, vp, vp, C.c_int]),
                        ("chisel_hip_frontiers", [vp, C.POINTER(FrontierWindow), vp, vp, C.c_int64, vp, C.c_int64, i64p, C.c_int, C.POINTER(FrontierTotals)]),
                        ("chisel_hip_travel_field", [vp, C.POINTER(TravelWindow), i32p, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, i64p, C.c_int,
                                                     C.POINTER(TravelTotals)]),
                        ("chisel_hip_travel_path", [vp, i32p, i32p, C.c_int64, i32p, i64p]),
                        ("chisel_hip_gather_meshes", [vp, C.POINTER(MeshRequest), C.c_int64, C.c_int64, vp, vp, vp, vp, vp, C.c_int, i64p, i32p,
                                                      C.POINTER(MeshTotals)]),
                        ("chisel_hip_gather_meshes_size", [vp, C.POINTER(MeshRequest), C.POINTER(MeshTotals)]),
                        ("chisel_hip_save_ply_binary", [vp, C.c_char_p]),
                        ("chisel_hip_gather_chunks", [vp, C.POINTER(ChunkRequest), C.c_int64, vp, vp, vp, C.c_int, i32p, i64p]),
                        ("chisel_hip_scatter_chunks", [vp, i32p, C.c_int64, vp, vp, vp, C.c_int, C.c_int, i64p]),
                        ("chisel_hip_coarse_mesh", [vp, C.POINTER(CoarseRequest), C.c_int64, vp, vp, vp, C.c_int, i64p, i32p, C.POINTER(CoarseTotals)]),
                        ("chisel_hip_indexed_mesh", [vp, C.POINTER(CoarseRequest), C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int, i64p, i64p, i32p,
                                                     C.POINTER(IndexedTotals)]),
                        ("chisel_hip_mesh_components", [vp, C.c_int64, C.c_int64, vp, C.c_int, vp, vp, C.c_int64, i64p, C.POINTER(ComponentsTotals)]),
                        ("chisel_hip_filter_mesh", [vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int64, C.c_int64, vp, vp, vp, vp,
                                                    vp, vp, C.c_int, C.POINTER(ComponentsTotals)]),
                        ("chisel_hip_mesh_adjacency", [vp, C.c_int64, C.c_int64, vp, C.c_int, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.POINTER(AdjacencyTotals)]),
                        ("chisel_hip_mesh_vertex_normals", [vp, C.c_int64, C.c_int64, vp, vp, C.c_int, vp, C.POINTER(AdjacencyTotals)]),
                        ("chisel_hip_smooth_mesh", [vp, C.c_int64, C.c_int64, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, vp, vp,
                                                    C.POINTER(AdjacencyTotals)]),
                        ("chisel_hip_kat_color_fresh", [C.POINTER(C.c_uint)]),
                        ("chisel_hip_kat_color_any", [C.POINTER(C.c_uint)]),
                        ("chisel_hip_debug_cloud_stats", [vp, i64p]),
                        ("chisel_hip_debug_hash_table", [vp, i64p, vp, vp, vp, vp]),
                        ("chisel_hip_kat_raycast", [f32p, C.c_int, i32p, i32p, i32p, C.c_int, i32p]),
                        ("chisel_hip_kat_reciprocal", [C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]),
                        ("chisel_hip_kat_floor", [C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)])):
        try:
            getattr(L, name).argtypes = types
        except AttributeError:
            pass
    L.chisel_hip_frustum.argtypes = [f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, f32p, f32p, f32p]
    L.chisel_hip_debug_frustum_range.argtypes = [f32p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                                 C.c_int, C.c_float, i32p, i32p, f32p, f32p]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise ChiselHipError(rc, load_library().chisel_hip_last_error().decode(errors="replace"))

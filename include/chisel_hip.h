/*
 * chisel_hip.h -- C ABI of libchisel_hip.so, the MI355X (gfx950) dense-TSDF backend that replaces the
 * CPU hot path of the OpenChisel library vendored in z619850002/CVIDS.
 *
 * Plain C: opaque handle, plain pointers and sizes, no Eigen / torch / STL types.  Every entry point
 * names the reference interface it replaces (paths relative to OpenChisel/open_chisel/ in the
 * reference tree).  The C++ facade in cvids_amd/open_chisel/ re-creates the reference's class
 * surface (chisel::Chisel, ProjectionIntegrator, ChunkManager, Chunk, Mesh) on top of this ABI;
 * INTEGRATION.md shows the binding a CVIDS maintainer adds.
 *
 * Conventions
 *   - all functions return a chisel_hip_status (0 = OK) unless documented otherwise;
 *     chisel_hip_last_error() gives the message of the calling thread's last failure.
 *   - poses are camera->world rigid transforms, row-major 3x4 [R|t] (the `Transform` /
 *     Eigen::Affine3f the reference passes; optical frame: z forward, x right, y down).
 *   - chunk ids are int[3] (chisel::ChunkID = Eigen::Vector3i); voxel i of a chunk is
 *     (z*N + y)*N + x (Chunk.h:81-84).
 *   - integrate calls are asynchronous on the map's HIP stream(s); every query / download
 *     synchronises first, so the observable behaviour is the reference's synchronous one.
 *   - image pointers may be host or device memory (`on_device`); device images must be complete
 *     when the call is made (or ordered with chisel_hip_set_stream / chisel_hip_wait_event) and stay
 *     valid until the map has consumed them (chisel_hip_synchronize / chisel_hip_record_event).
 *     Host images in pageable memory are copied during the call.  Host images in page-locked memory
 *     (hipHostMalloc / hipHostRegister) are read by the device when the batch runs -- depth straight
 *     over the bus by the first kernel, colour through an asynchronous copy -- so they too must stay
 *     untouched until the map has consumed them.
 *   - a map is driven from one thread at a time, as the reference is (chisel_ros: one ros::spin thread).
 */
#ifndef CHISEL_HIP_H_
#define CHISEL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an export is removed or re-typed, a struct of this header changes its layout, or one of the array-length macros below
 * (CHISEL_HIP_NUM_*) grows: a client built against another value must not call into the library (chisel_hip_abi_version() tells; the
 * facade's chisel::Chisel constructor and cvids_amd/capi.py refuse a mismatch).
 *   1  rounds 1-4
 *   2  round 5-6: chisel_hip_mesh_shell_plan_all removed, CHISEL_HIP_NUM_LAUNCH_STATS 8 -> 10, the device-plan and incremental
 *      meshesToUpdate entries added; later additions within 2 (nothing removed or re-typed): chisel_hip_pool_info,
 *      chisel_hip_frustum_from_vectors, chisel_hip_order_stream_after_map / _map_after_stream, the wait-free sharded recompute
 *      (chisel_hip_shell_plan_queue, _import_shells_fixed, _shell_commit), the stereo matcher (chisel_hip_stereo_*)
 *   3  chisel_hip_export_chunks, _import_ghost_chunks, _export_shells, _import_ghost_shells removed; later additions within 3 (nothing
 *      removed or re-typed): chisel_hip_render_view, chisel_hip_query_points, chisel_hip_cast_rays, chisel_hip_align_terms,
 *      chisel_hip_align_solve, chisel_hip_align_depth, chisel_hip_merge_map, chisel_hip_deintegrate_depth, chisel_hip_deintegrate_batch,
 *      chisel_hip_distance_field, chisel_hip_gather_meshes,
 *      chisel_hip_gather_meshes_size, chisel_hip_save_ply_binary, chisel_hip_gather_chunks, chisel_hip_scatter_chunks, chisel_hip_coarse_mesh,
 *      chisel_hip_indexed_mesh, chisel_hip_mesh_components, chisel_hip_filter_mesh, chisel_hip_mesh_adjacency,
 *      chisel_hip_mesh_vertex_normals, chisel_hip_smooth_mesh, chisel_hip_frontiers, chisel_hip_travel_field,
 *      chisel_hip_travel_path (no slot in the hipEvent profiler: CHISEL_HIP_NUM_KERNELS stays) */
#define CHISEL_HIP_ABI_VERSION 3

typedef struct chisel_hip_map chisel_hip_map; /* opaque: one TSDF map (or one shard of it) on one GPU */

typedef enum {
    CHISEL_HIP_OK = 0,
    CHISEL_HIP_ERR_INVALID = 1,     /* bad argument (null, non-cubic chunk, bad channel count ...)        */
    CHISEL_HIP_ERR_HIP = 2,         /* a HIP runtime call failed / no gfx950 device                        */
    CHISEL_HIP_ERR_POOL_FULL = 3,   /* chunk pool or hash exhausted (a fixed pool, or a growing one at its limit) */
    CHISEL_HIP_ERR_NOT_FOUND = 4,   /* chunk / mesh absent (the reference throws std::out_of_range)        */
    CHISEL_HIP_ERR_UNSUPPORTED = 5, /* feature outside the supported envelope                             */
    CHISEL_HIP_ERR_IO = 6           /* file could not be written                                          */
} chisel_hip_status;

/* truncation/{ConstantTruncator.h:48-51, InverseTruncator.h:42-53, QuadraticTruncator.h:42-67} */
typedef enum {
    CHISEL_HIP_TRUNC_CONSTANT = 0,  /* param = truncation distance [m]  */
    CHISEL_HIP_TRUNC_INVERSE = 1,   /* param = scalingFactor (the one ChiselNode.cpp:98 instantiates) */
    CHISEL_HIP_TRUNC_QUADRATIC = 2  /* param = scalingFactor */
} chisel_hip_truncator_kind;

/* Chisel::Chisel(const Eigen::Vector3i& chunkSize, float voxelResolution, bool useColor) Chisel.h:41,
 * ChunkManager::ChunkManager(...) ChunkManager.cpp:44-48 */
typedef struct {
    int chunk_size[3];       /* voxels per chunk edge; must be cubic: 8, 16 or 32                      */
    float voxel_resolution;  /* metres                                                                  */
    int use_color;           /* allocate RGBW voxels (ColorVoxel.h:95-98)                               */
    int device_id;           /* HIP device ordinal, -1 = current device                                 */
    int64_t max_chunks;      /* chunk pool: > 0 = exactly that many chunks (more: CHISEL_HIP_ERR_POOL_FULL); 0 = about 6 GiB of
                              * voxel payload to begin with, GROWING with the scene as the reference's unordered_map of heap chunks
                              * does (ChunkManager.h:40-55; up to 16 times that or three quarters of the device's memory); < 0 =
                              * -max_chunks chunks to begin with, growing likewise.  See chisel_hip_pool_info.  */
    int n_shards;            /* spatial sharding of the chunk hash over GPUs: number of shards (>=1)    */
    int shard_rank;          /* this map's shard, 0 <= shard_rank < n_shards                            */
    int shard_block;         /* ownership super-block edge in chunks, 0 = default (2)                   */
} chisel_hip_config;

/* ProjectionIntegrator(truncator, weighter, carvingDist, enableCarving, centroids) ProjectionIntegrator.h:43-44;
 * ChiselServer::SetupProjectionIntegrator chisel_ros/src/ChiselServer.cpp:480-487 */
typedef struct {
    int truncator_kind;      /* chisel_hip_truncator_kind                                               */
    float truncator_param;
    float weight;            /* ConstantWeighter(weight) weighting/ConstantWeighter.h:35-46            */
    int carving_enabled;     /* ProjectionIntegrator::SetCarvingEnabled                                 */
    float carving_dist;      /* ProjectionIntegrator::SetCarvingDist                                    */
} chisel_hip_integrator;

/* DepthImage<float> (camera/DepthImage.h:33-103) + PinholeCamera (camera/PinholeCamera.h:35-69) + Transform */
typedef struct {
    const float *depth;      /* width*height row-major fp32 metres, NaN = invalid                       */
    int width, height;
    int on_device;           /* 0: host pointer (copied in), 1: device pointer (used in place)          */
    float pose[12];
    float fx, fy, cx, cy;    /* Intrinsics.h:40-47                                                      */
    float near_plane, far_plane;
} chisel_hip_depth_frame;

/* ColorImage<uint8_t> (camera/ColorImage.h:38-134): 1 = mono, 2, 3 = BGR, 4 = BGRA */
typedef struct {
    const uint8_t *color;
    int width, height, channels;
    int on_device;
    float pose[12];
    float fx, fy, cx, cy;
} chisel_hip_color_frame;

/* PointCloud (pointcloud/PointCloud.h:33-82) + the arguments of Chisel::IntegratePointCloud (Chisel.h:57) */
typedef struct {
    const float *points;     /* n_points x (x, y, z) in the sensor frame (PointCloud::GetPoints)              */
    const float *colors;     /* n_points x (r, g, b) in [0, 1] (PointCloud::GetColors), or NULL = no colours  */
    int64_t n_points;
    int on_device;           /* both arrays in device memory (complete, or ordered by stream / event)         */
    float pose[12];          /* extrinsic: sensor -> world, row-major 3x4                                      */
    float truncation;        /* segment half-length of the chunk enumeration (ChiselServer.cpp:523: 0.1)      */
    float max_dist;          /* points farther from the sensor list no chunk (ChiselServer.cpp:523: far plane) */
} chisel_hip_pointcloud;

/* per-map accumulated voxel counters; index into the array of chisel_hip_get_counters */
enum {
    CHISEL_HIP_CNT_SDF = 0,       /* DistVoxel::Integrate executions                                    */
    CHISEL_HIP_CNT_COL = 1,       /* ColorVoxel::Integrate executions                                   */
    CHISEL_HIP_CNT_COL_SAT = 2,   /* in band, on the colour image, colour weight already >= 8           */
    CHISEL_HIP_CNT_PROBE = 3,     /* voxels of resident chunks that took the carve test                 */
    CHISEL_HIP_CNT_CARVED = 4,    /* Carve() / weight decay executions                                  */
    CHISEL_HIP_CNT_WORK_CHUNKS = 5, /* chunks the integration kernel visited                            */
    CHISEL_HIP_CNT_NEW_CHUNKS = 6,  /* chunks allocated                                                 */
    CHISEL_HIP_CNT_UPDATED_CHUNKS = 7, /* chunks whose integration reported "updated"                   */
    CHISEL_HIP_CNT_FRAMES = 8,
    CHISEL_HIP_NUM_COUNTERS = 9
};

/* kernels timed by the built-in hipEvent profiler (chisel_hip_set_profiling) */
enum {
    CHISEL_HIP_KERNEL_PYRAMID = 0,   /* depth min/max pyramid                                           */
    CHISEL_HIP_KERNEL_CULL = 1,      /* candidate enumeration + conservative culling + compaction        */
    CHISEL_HIP_KERNEL_INTEGRATE = 2, /* projective SDF/weight/colour integration (+ allocation)          */
    CHISEL_HIP_KERNEL_MESH = 3,      /* marching cubes (count + emit)                                   */
    CHISEL_HIP_KERNEL_RESOLVE = 4,   /* hash lookup of the candidates -> work-list                       */
    CHISEL_HIP_KERNEL_CLOUD = 5,     /* point-cloud fusion mode (all of its kernels)                     */
    CHISEL_HIP_NUM_KERNELS = 6
};

/* ---- life cycle ------------------------------------------------------------------------------------- */
int chisel_hip_abi_version(void);
const char *chisel_hip_last_error(void);
/* number of visible gfx950 devices (0 when there is none) */
int chisel_hip_device_count(void);
/* Image buffers of the caller (DepthImage.h:42-52 / ColorImage.h:44-58: `new DataType[...]`, allocated once by chisel_ros and refilled
 * every frame, ChiselServer.cpp:268-273,287-292): page-locked host memory, which the integrate calls read without the runtime's staged
 * copy of pageable memory (depth straight over the bus, colour as one asynchronous copy).  The facade's DepthImage / ColorImage allocate
 * through these; plain malloc / free when no HIP device is present (the buffer is then ordinary memory -- nothing computes on the CPU). */
void *chisel_hip_host_alloc(size_t bytes);
void chisel_hip_host_free(void *ptr);
/* Chisel::Chisel Chisel.h:41 */
int chisel_hip_create(const chisel_hip_config *config, chisel_hip_map **out);
int chisel_hip_destroy(chisel_hip_map *map);
/* Chisel::Reset Chisel.cpp:44-48 (+ ChunkManager::Reset ChunkManager.cpp:176-180) */
int chisel_hip_reset(chisel_hip_map *map);
/* ProjectionIntegrator setters ProjectionIntegrator.h:185-217 */
int chisel_hip_set_integrator(chisel_hip_map *map, const chisel_hip_integrator *integrator);
/* run the map's kernels on a caller-owned hipStream_t (NULL = the map's own stream) */
int chisel_hip_set_stream(chisel_hip_map *map, void *hip_stream);
int chisel_hip_synchronize(chisel_hip_map *map);
/* Ordering against work the caller queued on OTHER streams, without blocking the host (no reference counterpart: the
 * reference's images are host buffers).  wait_event: the device frames of the next integrate call are complete once
 * `hip_event` (a hipEvent_t the caller recorded behind their producer, e.g. an RCCL all-gather) has completed.
 * record_event: records `hip_event` behind everything queued on the map so far -- once it has completed the frames of
 * all earlier integrate calls have been read and their buffers may be overwritten. */
int chisel_hip_wait_event(chisel_hip_map *map, void *hip_event);
int chisel_hip_record_event(chisel_hip_map *map, void *hip_event);
/* The same two orderings for a caller that has a STREAM rather than events (hipStream_t as void*), one call each, with events the map keeps:
 * order_stream_after_map: whatever `stream` is given next starts after what the map has queued so far; order_map_after_stream: the map's
 * next call starts after what `stream` has been given so far.  Nothing is waited for. */
int chisel_hip_order_stream_after_map(chisel_hip_map *map, void *stream);
int chisel_hip_order_map_after_stream(chisel_hip_map *map, void *stream);

/* ---- the hot path ------------------------------------------------------------------------------------ */
/* Chisel::IntegrateDepthScan<float> Chisel.h:59-112 -> ProjectionIntegrator::Integrate ProjectionIntegrator.h:51-99
 * (candidate enumeration ChunkManager.cpp:182-212, allocation :171-174, GarbageCollect Chisel.cpp:61-67) */
int chisel_hip_integrate_depth(chisel_hip_map *map, const chisel_hip_depth_frame *frame);
/* Chisel::IntegrateDepthScanColor<float,uint8_t> Chisel.h:114-213 -> IntegrateColor ProjectionIntegrator.h:101-183 */
int chisel_hip_integrate_depth_color(chisel_hip_map *map, const chisel_hip_depth_frame *frame,
                                     const chisel_hip_color_frame *color);
/* Chisel::IntegratePointCloud Chisel.cpp:107-157 -> ChunkManager::GetChunkIDsIntersecting(cloud) ChunkManager.cpp:214-257,
 * ProjectionIntegrator::Integrate(cloud) ProjectionIntegrator.cpp:38-173, Raycast geometry/Raycast.cpp:35-128.  Every voxel
 * receives the updates of the rays that meet it in cloud order, as the reference's loop applies them.  Counters afterwards:
 * SDF, COL, PROBE (= ray cells inside listed chunks), CARVED, WORK_CHUNKS (= listed chunks), NEW_CHUNKS, UPDATED_CHUNKS.
 * Rays whose cell walk the reference would never finish (an axis steps past its end cell) stop at that point; rays with a
 * coordinate that is not finite meet no voxel.  CHISEL_HIP_ERR_UNSUPPORTED (at the next call that waits): more than 65536
 * chunks or 16 (chunk, point) pairs per point in one cloud, chunk ids beyond +-2^20. */
int chisel_hip_integrate_pointcloud(chisel_hip_map *map, const chisel_hip_pointcloud *cloud);
/* n frames in order (frame k+1 sees frame k's result, as n successive calls would); colors may be NULL.  Consecutive
 * frames of one image size share launch sets of up to 16 frames: the voxels of a chunk stay in registers across them. */
int chisel_hip_integrate_batch(chisel_hip_map *map, int n, const chisel_hip_depth_frame *frames,
                               const chisel_hip_color_frame *colors);
/* CHUNK IDS.  The map addresses the ids -2^20 + 2 ... 2^20 - 2 on every axis (an id and its 26 neighbours fit the 21 bits per axis the
 * chunk hash packs them into).  Every entry that takes a chunk id from its caller -- chisel_hip_garbage_collect, _has_chunk,
 * _download_chunk, _upload_chunk, _integrate_chunk, _update_meshes_of, _recompute_mesh, _mesh_size, _download_mesh, _generate_mesh,
 * _mesh_cube, _gather_chunks, _scatter_chunks, and chisel_hip_load_map for the ids of its file (chisel_hip_chunk_owner is a function of the id alone and takes any) --
 * refuses an id outside that range with CHISEL_HIP_ERR_INVALID before anything is launched: the map is as it was (after a refused
 * chisel_hip_load_map: reset, holding the file's chunks in front of the refused one). */
/* Chisel::GarbageCollect(const ChunkIDList&) Chisel.cpp:61-67 / ChunkManager::RemoveChunk(ChunkID) ChunkManager.h:99-108 */
int chisel_hip_garbage_collect(chisel_hip_map *map, const int *chunk_ids_xyz, int n);
/* Chisel::UpdateMeshes Chisel.cpp:50-59 (recompute on every 10th call unless force) ->
 * ChunkManager::RecomputeMeshes ChunkManager.cpp:130-169 */
int chisel_hip_update_meshes(chisel_hip_map *map, int force);

/* ---- queries (each synchronises) --------------------------------------------------------------------- */
/* ChunkManager::GetChunks().size() ChunkManager.h:67-70 */
int chisel_hip_num_chunks(chisel_hip_map *map, int64_t *out);
/* ids of all resident chunks, 3 ints each, ascending (x, then y, then z; the reference: the order of an unordered_map); writes
 * min(count, max_ids) ids, *count = total */
int chisel_hip_list_chunks(chisel_hip_map *map, int *ids_xyz, int64_t max_ids, int64_t *count);
/* ChunkManager::HasChunk ChunkManager.h:79-82 */
int chisel_hip_has_chunk(chisel_hip_map *map, const int id_xyz[3], int *out);
/* Chunk::GetVoxels / GetColorVoxels Chunk.h:66,117-120: N^3 sdf, N^3 weight, 4*N^3 rgbw (may be NULL) */
int chisel_hip_download_chunk(chisel_hip_map *map, const int id_xyz[3], float *sdf, float *weight, uint8_t *rgbw);
/* inverse of download (ChunkManager::AddChunk ChunkManager.h:89-92 with caller-filled voxels).  A chunk the pool has no slot for is
 * refused with CHISEL_HIP_ERR_POOL_FULL and the map stays as it was: later calls do not report the pool as exhausted */
int chisel_hip_upload_chunk(chisel_hip_map *map, const int id_xyz[3], const float *sdf, const float *weight,
                            const uint8_t *rgbw);
/* Chisel::GetMeshesToUpdate Chisel.h:220-223: ids flagged since the last recompute (27-neighbourhoods) */
int chisel_hip_meshes_to_update(chisel_hip_map *map, int *ids_xyz, int64_t max_ids, int64_t *count);
/* The same set for a caller that keeps its own copy between calls (the facade's Chisel::GetMeshesToUpdate, read after every frame:
 * ChiselServer.cpp:346): the ids that joined Chisel::meshesToUpdate (Chisel.h:175-189, :228) since the state `cursor` stands for -- two
 * words, zero before the first call, updated by the call.  *cleared != 0: the set was emptied in between (Chisel::UpdateMeshes' recompute,
 * Chisel.cpp:57, or Reset): the caller empties its copy first.  When more than max_ids ids are due nothing is consumed: *count says how
 * many, call again with room for them.  Cost: proportional to what changed since the cursor, not to the map. */
int chisel_hip_meshes_to_update_since(chisel_hip_map *map, uint64_t cursor[2], int *ids_xyz, int64_t max_ids, int64_t *count, int *cleared);
/* queues that listing behind the integration just handed over, without waiting: the caller's chisel_hip_synchronize then covers it and the
 * _since call that follows (same cursor, nothing integrated in between) neither launches nor waits */
int chisel_hip_meshes_to_update_prefetch(chisel_hip_map *map, const uint64_t cursor[2]);
/* ChunkManager::GetAllMeshes ChunkManager.h:163-166 */
int chisel_hip_num_meshes(chisel_hip_map *map, int64_t *out);
int chisel_hip_list_meshes(chisel_hip_map *map, int *ids_xyz, int64_t max_ids, int64_t *count);
/* Mesh (mesh/Mesh.h:54-58) sizes of one chunk's mesh: vertices (= normals = colors = indices), grids */
int chisel_hip_mesh_size(chisel_hip_map *map, const int id_xyz[3], int64_t *n_vertices, int64_t *n_grids);
/* 3 floats per vertex / grid; any pointer may be NULL; indices are 0..n_vertices-1 (MarchingCubes.h:92-94) */
int chisel_hip_download_mesh(chisel_hip_map *map, const int id_xyz[3], float *vertices, float *normals,
                             float *colors, float *grids);
/* ChunkManager::GetSDF ChunkManager.cpp:476-499 ; *found = 0 when the reference returns false */
int chisel_hip_get_sdf(chisel_hip_map *map, const float pos[3], double *dist, int *found);
/* ChunkManager::GetSDFAndGradient ChunkManager.cpp:449-474 */
int chisel_hip_get_sdf_and_gradient(chisel_hip_map *map, const float pos[3], double *dist, float grad[3], int *found);
/* Chisel::SaveAllMeshesToPLY Chisel.cpp:69-105 + SaveMeshPLYASCII io/PLY.cpp:29-88 */
int chisel_hip_save_ply(chisel_hip_map *map, const char *path);
/* SaveMeshPLYASCII(fileName, mesh) (src/io/PLY.cpp:29-88) for ONE mesh the caller holds: the same text format; colors (3 floats in
 * [0, 1] per vertex) may be NULL; indices: three per face, as Mesh::indices.  Host I/O only. */
int chisel_hip_write_mesh_ply(const char *path, const float *vertices, const float *colors, int64_t n_vertices, const int64_t *indices,
                              int64_t n_indices);

/* ---- the map's chunk meshes gathered into one buffer (DESIGN.md 3.12 "Mesh gather") ----------------------------------
 * Not in the reference as an entry: what ChiselServer::FillMarkerTopicWithMeshes (chisel_ros/src/ChiselServer.cpp:613-716) does
 * by walking GetAllMeshes() -- every chunk mesh's vertices and grids appended to one marker, every vertex coloured from the mesh
 * colours or from two Lambert terms of its normal -- as one call from HBM into the caller's contiguous arrays. */
#define CHISEL_HIP_GATHER_TILE_FLOATS 4096   /* floats of the concatenated outputs one workgroup copies (tests aim at tile edges) */
typedef struct {
    const int *ids_xyz; int64_t n_ids;  /* NULL / 0: every mesh, in chisel_hip_list_meshes' order (x, then y, then z); otherwise these
                                           chunks' meshes in the caller's order, duplicates allowed */
    int marker_colors;                  /* 0: rgba is not asked for */
    float light0[3], light1[3];         /* used as given, not normalised by the library */
    float diffuse, ambient;
} chisel_hip_mesh_request;              /* 56 bytes */
typedef struct { int64_t meshes, meshes_nonempty, vertices, grids, arenas_read, tiles; } chisel_hip_mesh_totals;
/* Mesh i of the selection occupies vertices [first_i, first_i + n_v,i) of `vertices`, `normals`, `colors` (3 floats each; colors only
 * on a map that holds colour) and `rgba` (4 floats), and grid entries [gfirst_i, gfirst_i + n_g,i) of `grids` (3 floats); the firsts
 * are the exclusive prefix sums of the selection in order, and every float is the bit pattern chisel_hip_download_mesh returns for
 * that chunk.  A mesh that exists but is empty contributes a table row of zeros.  rgba (a = 1): on a map with colour the mesh colour
 * of the vertex; otherwise, in fp32 with every operation rounded on its own, d_k = (n.x l_k.x + n.y l_k.y) + n.z l_k.z,
 * s_k = fmaxf(d_k, 0) diffuse (0 for a NaN normal), c = (s_0 + s_1) + ambient, r = g = b = fminf(c, 1).
 * Any of the five output arrays may be NULL, not all.  With on_device they are device pointers, filled on the map's stream by one
 * launch, and nothing is waited for after it; otherwise host arrays, complete on return, each copied out once, exactly its live
 * data.  capacity_vertices / capacity_grids: the entries the per-vertex arrays / the grids array have room for (an array that is not
 * asked for needs none).  mesh_table (4 int64 per mesh: first vertex, vertices, first
 * grid, grids), mesh_ids_xyz (3 per mesh) and totals are host memory, complete on return, and may be NULL.  The map is only read.
 * Waits: once, for the job records of a mesh recompute that is still in flight (as chisel_hip_list_meshes does); the segment table
 * goes up from pinned memory that outlives the call, its device copy is scratch kept in the map, grown on demand, freed with it.
 * Refused with nothing written: CHISEL_HIP_ERR_INVALID for a null map or request, n_ids < 0, ids without a count or a count without
 * ids, an id outside the addressable range, no output, colors on a map without colour, a light, diffuse or ambient that is not
 * finite with marker_colors set, rgba without marker_colors, a capacity below the totals (totals is filled all the same, so that
 * the caller can retry); CHISEL_HIP_ERR_NOT_FOUND for an id without a mesh (the message names its index);
 * CHISEL_HIP_ERR_UNSUPPORTED for a group (its meshes sit on several devices; one shard of several is served: its meshes are its
 * own) and for a selection of more than 2^31 - 1 floats in one array. */
int chisel_hip_gather_meshes(chisel_hip_map *map, const chisel_hip_mesh_request *request, int64_t capacity_vertices, int64_t capacity_grids,
                             float *vertices, float *normals, float *colors, float *rgba, float *grids, int on_device,
                             int64_t *mesh_table, int *mesh_ids_xyz, chisel_hip_mesh_totals *totals);
/* the same bookkeeping without a launch: the totals of the selection (tiles: of all arrays the map and the request could give) */
int chisel_hip_gather_meshes_size(chisel_hip_map *map, const chisel_hip_mesh_request *request, chisel_hip_mesh_totals *totals);
/* chisel_hip_save_ply's elements, properties and vertex order as "format binary_little_endian 1.0", fed by one host-side gather (no
 * host copy of any arena is made).  A group is CHISEL_HIP_ERR_UNSUPPORTED. */
int chisel_hip_save_ply_binary(chisel_hip_map *map, const char *path);

/* ---- many chunks out of and into the map in one launch each (DESIGN.md 3.13 "Chunk gather and scatter") ---------------
 * Not in the reference as entries: what a loop of Chunk::GetVoxels / ChunkManager::AddChunk over many chunks moves
 * (chisel_hip_download_chunk / chisel_hip_upload_chunk here), as one packed set.  A packed set of n chunks is sdf[n][V],
 * weight[n][V], rgbw[n][V][4] with V = N^3: chunk i of the selection at index i, voxel order the map's ((z N + y) N + x), every value
 * the bit pattern the per-chunk entry moves (NaN payloads, -0.0 and denormals included).  With on_device the three arrays are
 * device pointers, 16-byte aligned; otherwise host arrays.  Ids are always host memory. */
typedef struct {
    const int *ids_xyz; int64_t n_ids;  /* NULL / 0: every resident chunk, ascending (x, then y, then z) as chisel_hip_list_chunks;
                                           otherwise these chunks in the caller's order, duplicates allowed */
    int use_box; int box_lo[3], box_hi[3]; /* with ids NULL and use_box: only the resident chunks with lo <= id <= hi on every axis */
} chisel_hip_chunk_request;             /* 48 bytes */
/* Only reads the map.  Any of sdf, weight, rgbw may be NULL.  capacity_chunks: the chunks each given array (and chunk_ids_xyz) has
 * room for; capacity_chunks == 0 is the size query, which fills *n_chunks and nothing else.  With all three arrays NULL at a non-zero
 * capacity, chunk_ids_xyz alone is filled (the selection's ids; nothing is launched).  With on_device the arrays are filled by one
 * launch on the map's stream, behind whatever is queued, and nothing is waited for after it; host arrays are staged through one
 * owned device buffer, copied out once each, and are complete on return.  One wait, for the selection: the listing of the resident
 * chunks (all, box) or the slot look-up of a list.  chunk_ids_xyz (3 per chunk, may be NULL) and *n_chunks are complete on return.
 * Refused with nothing written: CHISEL_HIP_ERR_INVALID for a null map or request, n_ids < 0, ids without a count or a count without
 * ids, use_box together with ids, a box with lo > hi on an axis, an id outside the addressable range (the message names its index), no
 * output at a non-zero capacity, rgbw on a map without colour, a device pointer that is not 16-byte aligned, a capacity below the
 * selection (*n_chunks is filled all the same, so that the caller can retry); CHISEL_HIP_ERR_NOT_FOUND for a listed id that is not
 * resident (the message names its index); CHISEL_HIP_ERR_UNSUPPORTED for a group (one shard of several is served with its own chunks)
 * and for a selection whose bytes or launch grid do not fit (2^31 - 1 chunks, 2^31 - 1 tiles of 16 KiB per array). */
int chisel_hip_gather_chunks(chisel_hip_map *map, const chisel_hip_chunk_request *request, int64_t capacity_chunks,
                             float *sdf, float *weight, uint8_t *rgbw, int on_device,
                             int *chunk_ids_xyz, int64_t *n_chunks);
/* Changes the map: for an accepted call what n calls of chisel_hip_upload_chunk in order leave -- resident ids, every voxel,
 * chisel_hip_meshes_to_update, the meshes of a later recompute, what later integrations leave.  An absent id is created, a resident
 * chunk is overwritten whole; rgbw == NULL on a map with colour writes zeros; the slot's sign summary says "any sign" (the mesher
 * looks at the chunk).  mark_updated != 0: every chunk of the call is also left as an integration that changed it leaves it -- it
 * and its resident neighbours are named by chisel_hip_meshes_to_update and meshed by the next recompute (a live map that receives
 * chunks needs this; a restore into a fresh map does not).  On the map's stream: ids up, a classify launch (slot per id, the absent
 * ones counted), THE ONE WAIT of the call (the absent count and the free slots, through pinned memory), room in a growable pool, a
 * create launch, the copy launch.  With on_device nothing is waited for after the copy launch; host arrays are staged and are
 * consumed on return.  *n_created (may be NULL): the chunks the call created.  n == 0 is a successful no-op.
 * Refused with the map as it was: CHISEL_HIP_ERR_INVALID for a null map, ids, sdf or weight, n < 0, an id out of range, an id that
 * repeats an earlier one (the message names the second index), an id another shard owns (chisel_hip_chunk_owner; the message names
 * its index), rgbw on a map without colour, a device pointer that is not 16-byte aligned; CHISEL_HIP_ERR_POOL_FULL when a fixed pool
 * (or a growable one at its limit) cannot take the absent ids -- all or nothing, decided before the create launch, and not latched
 * as "map incomplete"; CHISEL_HIP_ERR_UNSUPPORTED for a group. */
int chisel_hip_scatter_chunks(chisel_hip_map *map, const int *ids_xyz, int64_t n,
                              const float *sdf, const float *weight, const uint8_t *rgbw, int on_device,
                              int mark_updated, int64_t *n_created);

/* ---- a coarse marching-cubes mesh at every s-th voxel, packed (DESIGN.md 3.14 "Coarse mesh") ----------------------------
 * Not in the reference: its mesh exists at the voxel grid alone.  With N the chunk edge, res the voxel resolution, s the stride
 * (1 <= s <= N, N % s == 0) and M = N / s, a selected resident chunk c has the coarse cubes (i, j, k) in [0, M)^3.  Cube (i, j, k)
 * has the base voxel b = s (i, j, k); its corner d is the voxel b + s cubeIndexOffsets[d] (ChunkManager.cpp:67-69), a component equal
 * to N meaning voxel 0 of the chunk one further along that axis (ExtractBorderVoxelMesh's rule, :296-379; + neighbours only, up to
 * seven).  A cube yields nothing when a corner's chunk is absent or a corner's weight is <= 0.5 (:273, :311, :351); every other cube
 * is a MESHED cube.  Its coordinates are ((float)b res + half_res) + (float)(N c) res per axis (:50-66, Chunk.cpp:43), corner d lies
 * at coords + (float)offset_d step with step = (float)s res rounded once to fp32 -- at s = 1 cubeCoordOffsets exactly --, and its
 * triangles are MarchingCubes::MeshCube's on those eight coordinates and distances: vertices in its push order (t + 2, t + 1, t),
 * each triangle's face normal three times (as chisel_hip_mesh_cube_values).  Order: chunks in the selection's order, cubes of a
 * chunk by ascending (k M + j) M + i, vertices of a cube in MeshCube's order -- a pure function of map and request.  At s = 1 a
 * chunk's triangles are those of chisel_hip_generate_mesh, in another order.  No grid entries.
 * stages (as chisel_hip_generate_mesh): bit 0 replaces a face normal by ComputeNormalsFromGradients' where the look-up succeeds, bit
 * 1 gives InterpolateColor's colour -- exactly what chisel_hip_shade_vertices makes of the call's vertices and face normals;
 * colours without bit 1 are zeros. */
typedef struct {
    chisel_hip_chunk_request chunks; /* the selection: all resident / a box / a list, as chisel_hip_gather_chunks */
    int stride;                      /* s */
    int stages;                      /* bit 0 gradient normals, bit 1 colours */
} chisel_hip_coarse_request;         /* 56 bytes */
typedef struct { int64_t chunks, chunks_nonempty, cubes_meshed, vertices; } chisel_hip_coarse_totals;
/* Only reads the map; everything runs on the map's stream, behind whatever is queued.  vertices, normals, colors: 3 floats per
 * vertex, each with room for capacity_vertices vertices; normals and colors may be NULL.  chunk_table (2 per chunk of the
 * selection: first vertex, vertices; a chunk without a triangle has (first, 0)), chunk_ids_xyz (3 per chunk) and totals are host
 * memory, may be NULL, and are complete on return.  capacity_vertices == 0 is the size query: the count pass runs, totals is
 * filled, chunk_table and chunk_ids_xyz when given, and nothing else is written.  Otherwise the host waits once, for the totals,
 * read through pinned memory (a list's slot look-up is queued in front of the count; "all" and a box wait a second time before it,
 * for the listing of the resident chunks that the host sorts); with on_device the emit and shade launches follow and nothing is
 * waited for after them; host arrays are staged through one owned device buffer, copied out once each with exactly their live
 * data, and are complete on return.  The scratch (per-chunk counts and firsts, the slot list) is kept in the map, grown on demand
 * and freed with it.
 * Refused with nothing written: CHISEL_HIP_ERR_INVALID for a null map or request, a stride < 1, > N or that does not divide N,
 * stages outside 0 .. 3, stage bit 1 or colors on a map without colour, whatever chisel_hip_gather_chunks refuses of a selection,
 * a negative capacity, the size query without totals, no output at a non-zero capacity, normals or colors without vertices, a
 * capacity below the total (totals is filled all the same, so that the caller can retry); CHISEL_HIP_ERR_NOT_FOUND for a listed id
 * that is not resident (the message names its index); CHISEL_HIP_ERR_UNSUPPORTED for a group or one shard of several (a cube on a
 * + face needs its neighbour's owner) and for more than 2^31 - 1 floats in one array. */
int chisel_hip_coarse_mesh(chisel_hip_map *map, const chisel_hip_coarse_request *request, int64_t capacity_vertices,
                           float *vertices, float *normals, float *colors, int on_device,
                           int64_t *chunk_table, int *chunk_ids_xyz, chisel_hip_coarse_totals *totals);

/* ---- an indexed marching-cubes mesh: one vertex per crossed lattice edge (DESIGN.md 3.15 "Indexed mesh") ----------------
 * Not in the reference: MarchingCubes::MeshCube (MarchingCubes.h:73-106) pushes three private vertices per triangle, and a shared
 * edge's vertex is recomputed per cube.  Selection, stride s, M = N / s, lattice, MESHED cube and configuration are exactly
 * chisel_hip_coarse_mesh's.  A lattice point l = (li, lj, lk) in [0, M)^3 of a resident chunk o -- the OWNER -- owns three EDGES,
 * one per axis a, from l to l + e_a; the upper end may be lattice point 0 of the + neighbour.  An edge is USED when it is crossed
 * ((sdf_lo < 0) != (sdf_hi < 0), CalculateVertexConfiguration's comparison, MarchingCubes.h:108-118) and at least one MESHED cube
 * of a selected chunk has it among its twelve (edgeIndexPairs, MarchingCubes.cpp:289-303); exactly the used edges get a vertex.
 * Its position is InterpolateVertex(P, Q, sdf_lo, sdf_hi) (MarchingCubes.h:135-146, the |difference| < 1e-6 branch included),
 * always from the lower end to the upper: P the centre of voxel s l of the owner, ((float)(s l) res + half_res) + (float)(N o) res
 * per axis (ChunkManager.cpp:50-66, Chunk.cpp:43), Q = P with step = (float)s res added on axis a only -- a function of the edge
 * alone, never of the selection or of the cube that asks.
 * Owners: the selected chunks in the selection's order, then the EXTRAS -- the resident + neighbours (up to seven per selected
 * chunk) that are not selected, each once, ascending by x, then y, then z ("all resident" has none).  Vertex ids: owners in that
 * order, inside an owner ascending (a, lk, lj, li).  Triangles: selected chunks in order, cubes by ascending (k M + j) M + i,
 * MeshCube's triangles in table order, the three ids in its push order (t + 2, t + 1, t) -- row for row the coarse mesh's.
 * normals (stage bit 0) are zeros overwritten by ComputeNormalsFromGradients (ChunkManager.cpp:609-626) where its look-up succeeds,
 * colors (stage bit 1) InterpolateColor's: bit for bit what chisel_hip_shade_vertices makes of the vertices with zero normals;
 * colours without bit 1 are zeros.  Face normals have no per-vertex meaning and are not offered
 * (the normals of the triangles around a vertex: chisel_hip_mesh_vertex_normals). */
typedef struct { int64_t chunks, owners, cubes_meshed, vertices, triangles; } chisel_hip_indexed_totals;
/* Only reads the map; everything runs on the map's stream, behind whatever is queued.  vertices, normals, colors: 3 floats per
 * vertex with room for capacity_vertices; indices: 3 int32 per triangle with room for capacity_triangles; normals, colors and
 * indices may be NULL.  chunk_table (2 per selected chunk: first triangle, triangles), owner_table (2 per owner: first vertex,
 * vertices), owner_ids_xyz (3 per owner; at most 8 per selected chunk) and totals are host memory, may be NULL, and are complete
 * on return.  Both capacities 0 is the size query: totals and the tables are filled and nothing else is written.  The host waits
 * once, for the totals (pinned memory), plus the wait "all" and a box cost the coarse mesh; with on_device nothing is waited for
 * after the launches.  The scratch (row masks and prefixes per owner, counts, the slot -> owner table) is kept in the map, grown
 * on demand and freed with it.
 * Refused with nothing written: everything chisel_hip_coarse_mesh refuses; CHISEL_HIP_ERR_INVALID for an id that repeats an
 * earlier one of the list (an owner is unique; the message names its index), normals without stage bit 0, indices without
 * vertices, either capacity below its total (totals is filled all the same); CHISEL_HIP_ERR_NOT_FOUND for a listed id that is not
 * resident; CHISEL_HIP_ERR_UNSUPPORTED for a group or one shard of several and for more than 2^31 - 1 vertices or index entries. */
int chisel_hip_indexed_mesh(chisel_hip_map *map, const chisel_hip_coarse_request *request, int64_t capacity_vertices,
                            int64_t capacity_triangles, float *vertices, int32_t *indices, float *normals, float *colors,
                            int on_device, int64_t *chunk_table, int64_t *owner_table, int *owner_ids_xyz,
                            chisel_hip_indexed_totals *totals);

/* ---- connected components of an indexed mesh, and the mesh without its small ones (DESIGN.md 3.16 "Mesh components") ----
 * Not in the reference, whose meshes share no vertex.  Input: n_vertices = V, n_triangles = T, indices: 3 int32 per triangle (what
 * chisel_hip_indexed_mesh writes, or any index array).  A triangle is VALID when all three ids lie in [0, V); an invalid one joins
 * nothing, has component -1, is never kept and is counted in totals.invalid_triangles -- the kernels test the three ids before they
 * use any as an address: an array of garbage gives a wrong answer, never a fault.  The COMPONENTS are those of the graph on the V
 * vertices whose edges are the sides of the valid triangles; a triangle with repeated ids is valid and joins what it names; a vertex
 * in no valid triangle is a component of its own with 0 triangles.  A component's ROOT is its smallest vertex id; components are
 * numbered 0 ... C - 1 by ascending root.  vertex_component[v]: the number of v's component; triangle_component[t]: that of its
 * first id, or -1; component_table: 3 int64 per component -- root, vertices, valid triangles.  FILTER: component c is KEPT when
 * triangles(c) >= min_triangles (>= 1); with largest_only it must in addition be the component with the most triangles, the lowest
 * number winning a tie.  Kept vertices keep their order and are renumbered 0 ... V' - 1, kept triangles keep theirs and their ids
 * are renumbered; the rows of vertices, normals and colors are copied bit for bit; vertex_map[V] and triangle_map[T] say old -> new,
 * -1 when dropped.  Everything is a pure function of (V, T, indices, min_triangles, largest_only): no float is computed. */
typedef struct { int64_t vertices, triangles, invalid_triangles, components, largest_triangles, kept_components, kept_vertices, kept_triangles; } chisel_hip_components_totals;
/* The map is neither read nor written: it lends its device, its stream and its scratch (a group is refused with
 * CHISEL_HIP_ERR_UNSUPPORTED; hand in a map of one shard).  Everything is queued on the map's stream behind what is queued, a
 * chisel_hip_indexed_mesh(on_device) whose outputs are this call's inputs included.  on_device says where ALL array arguments live,
 * inputs and outputs alike; component_table and totals are always host memory.  Host arrays are staged through owned device buffers,
 * copied out once with exactly their live rows, and complete on return.  The host waits once, for the totals (pinned memory); with
 * on_device nothing is waited for behind the launches that write the arrays -- except for component_table, whose rows (their number
 * is a total) are written to pinned memory behind that wait and waited for.  vertex_component (V), triangle_component (T) and
 * component_table (room for capacity_components rows; capacity 0: not asked for) may be NULL; with none of them asked for the call
 * is the size query: totals is filled and nothing else is written.  A table capacity below the number of components is refused
 * with totals filled.  totals: vertices, triangles, invalid_triangles, components, largest_triangles (the most valid triangles of
 * one component); kept_* are 0 (no filter is applied).  V = 0 and T = 0 succeed with zero totals and nothing launched.  The scratch
 * (6 ints per vertex, 1 per triangle, tile sums) is kept in the map, grown on demand and freed with it.
 * Refused with nothing written: CHISEL_HIP_ERR_INVALID for a null map, negative sizes or capacity, null indices with T > 0, a
 * capacity without a table, the size query without totals; CHISEL_HIP_ERR_UNSUPPORTED for V or 3 T above 2^31 - 1. */
int chisel_hip_mesh_components(chisel_hip_map *map, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, int on_device,
                               int32_t *vertex_component, int32_t *triangle_component,
                               int64_t capacity_components, int64_t *component_table,
                               chisel_hip_components_totals *totals);
/* The frame of chisel_hip_mesh_components.  vertices, normals, colors: 3 floats per vertex, read only where the matching output is
 * written; out_vertices, out_normals, out_colors have room for capacity_vertices rows, out_indices for capacity_triangles; the
 * outputs must not overlap the inputs.  vertex_map (V) and triangle_map (T) are optional and sized by the input.  Both capacities
 * 0 is the size query: totals (all eight) is filled and nothing else is written.  A capacity below its total, of an array that is
 * asked for, is refused with totals filled, so that the caller can retry.  With on_device nothing is waited for behind the
 * compaction launches.
 * Refused with nothing written: what chisel_hip_mesh_components refuses about sizes and indices; min_triangles < 1; largest_only
 * outside 0 / 1; negative capacities; the size query without totals; an output (vertices, normals, colors) without the matching
 * input; normals or colors in without the matching output where out_vertices is asked for; out_indices, out_normals or out_colors
 * without out_vertices. */
int chisel_hip_filter_mesh(chisel_hip_map *map, int64_t n_vertices, int64_t n_triangles, const int32_t *indices,
                           const float *vertices, const float *normals, const float *colors,
                           int64_t min_triangles, int largest_only,
                           int64_t capacity_vertices, int64_t capacity_triangles,
                           float *out_vertices, int32_t *out_indices, float *out_normals, float *out_colors,
                           int32_t *vertex_map, int32_t *triangle_map, int on_device,
                           chisel_hip_components_totals *totals);

/* ---- adjacency, vertex normals and smoothing of an indexed mesh (DESIGN.md 3.17 "Mesh adjacency") ----
 * Not in the reference.  Input as for chisel_hip_mesh_components: n_vertices = V, n_triangles = T, indices: 3 int32 per triangle.  A
 * triangle is VALID when all three ids lie in [0, V); the ids are tested before any is used as an address (garbage gives a wrong
 * answer, never a fault); invalid triangles take part in nothing and are counted.
 * INCIDENCE: row v is the ascending list of the valid triangles that name v, each once even when it names v twice; deg(v) is its
 * length.  NEIGHBOURS: row v is the ascending list of the distinct ids u != v named by the triangles of v's incidence row; c(v, u)
 * is the number of triangles of row v that name u.  FLAGS of v: bit 0 BOUNDARY: some u with c(v, u) == 1; bit 1 NONMANIFOLD: some u
 * with c(v, u) > 2; bit 2 ISOLATED: deg(v) == 0.  Rows are stored CSR-wise: row v is items[offsets[v]] ... items[offsets[v + 1] - 1].
 * VALENCE LIMIT: an index array with a deg above CHISEL_HIP_MESH_MAX_INCIDENT (marching cubes cannot exceed 20) is refused by all
 * three entries with CHISEL_HIP_ERR_UNSUPPORTED, totals filled up to max_incident (the neighbour and flag totals then leave the rows
 * above the limit out); this bounds every per-vertex loop.
 * VERTEX NORMALS, every step fp32 and rounded on its own: acc = (+0, +0, +0); for each t of v's incidence row in ascending order, with
 * its ids (i0, i1, i2) as stored, px = P[i1] - P[i0], py = P[i2] - P[i0], n = (px.y py.z - px.z py.y, px.z py.x - px.x py.z,
 * px.x py.y - px.y py.x) (the coarse mesh's un-normalised face normal), acc = acc + n; len = sqrt((acc.x acc.x + acc.y acc.y) +
 * acc.z acc.z); the normal is acc / len when len > 0, else (+0, +0, +0).
 * SMOOTHING (Taubin): a vertex is PINNED when flags & pin_flags is non-zero or it has no neighbour.  One PASS with factor f copies a
 * pinned vertex bit for bit and gives any other, per component and in ascending neighbour order, m = ((P[u0] + P[u1]) + P[u2]) + ...,
 * m = m / (float)count, d = m - P[v], Q[v] = P[v] + f d (the product rounded, then the sum).  An iteration is a pass with lambda, then
 * one with mu when mu != 0 (mu == 0: plain Laplacian smoothing); a pass reads only the positions the pass before it wrote; the
 * adjacency is the input's; iterations == 0 copies the vertices.  Integers and floats alike are a pure function of the arguments:
 * no float is added atomically, every sum has one order. */
#define CHISEL_HIP_MESH_MAX_INCIDENT 32
enum { CHISEL_HIP_MESH_BOUNDARY = 1, CHISEL_HIP_MESH_NONMANIFOLD = 2, CHISEL_HIP_MESH_ISOLATED = 4 };
typedef struct {
    int64_t vertices, triangles, invalid_triangles, incidences, neighbors, max_incident, max_neighbors;
    int64_t boundary_vertices, nonmanifold_vertices, isolated_vertices, pinned_vertices /* chisel_hip_smooth_mesh; else 0 */, reserved;
} chisel_hip_adjacency_totals;
/* The frame of chisel_hip_mesh_components: the map lends its device, its stream and its scratch (a group is refused with
 * CHISEL_HIP_ERR_UNSUPPORTED), everything is queued on the map's stream behind what is queued, on_device says where ALL array arguments
 * live, totals is host memory, host arrays are staged through owned device buffers and are complete on return.  The host waits once,
 * for the totals: the whole structure is built in the map's scratch in front of that wait, so also the compact neighbour arrays cost
 * no second one; with on_device nothing is waited for behind the launches that write the arrays.  All outputs are optional:
 * tri_offsets and nbr_offsets (V + 1), tri_items (room for capacity_incidence ids), nbr_items (room for capacity_neighbors),
 * vertex_flags (V); with none of them it is the size query: totals is filled and nothing else is written.  A capacity below its total,
 * of an array that is asked for, is refused with totals filled.  3 T bounds the incidences and 6 T the neighbours, so a call with
 * those capacities never needs a retry.  V = 0 or T = 0 succeeds: every vertex is isolated.  The scratch (6 ints per vertex, 9 per
 * triangle, tile sums) is kept in the map, grown on demand and freed with it.
 * Refused with nothing written: what chisel_hip_mesh_components refuses about sizes and indices; CHISEL_HIP_ERR_UNSUPPORTED for 6 T
 * above 2^31 - 1 and for the valence limit; negative capacities; the size query without totals. */
int chisel_hip_mesh_adjacency(chisel_hip_map *map, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, int on_device,
                              int32_t *tri_offsets, int64_t capacity_incidence, int32_t *tri_items,
                              int32_t *nbr_offsets, int64_t capacity_neighbors, int32_t *nbr_items,
                              int32_t *vertex_flags, chisel_hip_adjacency_totals *totals);
/* normals[V]: 3 floats per vertex by the rule above, from vertices[V] (3 floats each).  Without normals it is the size query.  One
 * host wait, for the totals and the valence verdict.  Refused in addition: null vertices where normals are asked for (V > 0). */
int chisel_hip_mesh_vertex_normals(chisel_hip_map *map, int64_t n_vertices, int64_t n_triangles, const int32_t *indices,
                                   const float *vertices, int on_device, float *normals, chisel_hip_adjacency_totals *totals);
/* out_vertices[V]: the positions after `iterations` iterations; out_normals[V] (optional): the vertex normals of those positions.
 * pin_flags: a mask over the FLAGS bits; totals.pinned_vertices counts the pinned.  Without out_vertices it is the size query.  One
 * host wait.  out_vertices must not overlap vertices.  A second position buffer (3 V floats) is kept in the map.
 * Refused in addition: negative iterations, a lambda or mu that is not finite, pin_flags outside 0 .. 7, out_normals without
 * out_vertices, null vertices where out_vertices is asked for (V > 0), out_vertices overlapping vertices. */
int chisel_hip_smooth_mesh(chisel_hip_map *map, int64_t n_vertices, int64_t n_triangles, const int32_t *indices, const float *vertices,
                           int iterations, float lambda, float mu, int pin_flags, int on_device,
                           float *out_vertices, float *out_normals, chisel_hip_adjacency_totals *totals);

/* ---- meshing a sharded map (SURVEY.md 8e "meshing across shards") -------------------------------------------------
 * A chunk's mesh reads its 26 neighbours (cube corners: ChunkManager.cpp:316-357; gradient normals and colours of border
 * vertices: :449-499, :588-607), most of which belong to other shards.  The owners send the parts of those chunks that
 * are read, the mesher installs them as "ghost" chunks -- resident, never integrated (cull_kernel only takes chunks this
 * shard owns) -- recomputes the meshes of its own chunks and drops the ghosts again.  cvids_amd/sharded.py orchestrates
 * the exchange (ShardedChisel.UpdateMeshes) with the device plan and its wait-free form further down
 * (chisel_hip_shell_plan_device, chisel_hip_shell_plan_queue).
 * What the meshes are equal to: the reference's on this shard's VIEW -- its own chunks and the received boxes, default voxels
 * elsewhere in a ghost -- element for element.  Against the reference on the whole map, vertex positions and grid entries are
 * always equal; normals and colours are equal except at vertices whose normal or colour the reference reads outside the job's 26
 * neighbours: the v1 + 0.5 v2 vertex of InterpolateVertex's degenerate branch (MarchingCubes.h:135-146), 1.5 times as far from the
 * origin as its cube, and InterpolateColor's eight look-ups at voxel indices taken for metres (ChunkManager.cpp:506-520), which near
 * the origin land in chunks of other shards.  Measured on hand-built fields: no row of 285 870 at 3 cm away from
 * such look-ups, up to 2 747 colour rows of 285 870 where they land inside the map, up to 1 301 normal and 2 168 colour rows of
 * 76 800 with degenerate vertices near the origin; none far from the origin.  Whole far chunks are not moved.
 *   drop_ghost_chunks    remove the ghosts of the latest chisel_hip_import_shells_packed / _import_shells_fixed (named by
 *                        the items of the received segments, which must stay untouched until then)
 *   update_meshes_of     RecomputeMeshes (ChunkManager.cpp:130-169) for exactly these chunk ids -- the shard's share of
 *                        the union of all shards' meshesToUpdate -- then meshesToUpdate.clear() (Chisel.cpp:57) */
int chisel_hip_drop_ghost_chunks(chisel_hip_map *map);
int chisel_hip_update_meshes_of(chisel_hip_map *map, const int *ids_xyz, int n);

/* ---- the step before the path ------------------------------------------------------------------------
 * CollaborativeServer::PublishDenseInfo's image conditioning (server_pose_graph/src/collaborative_server_system.cpp:
 * 199-276): cv::resize of the depth map (CV_64F) and the colour image (CV_8UC1 / CV_8UC3) to the publish size (640 x 480
 * there, :213-214), and for depth the narrowing to float (:255), NaN for readings < 0.1 or > 20 (:262-265) and the rescaled
 * intrinsics fx, fy, cx, cy (:216-219).  cv::resize with its default INTER_LINEAR is restated from OpenCV's published
 * algorithm (imgproc/resize.cpp without IPP): scale = 1. / (dst / (double)src); tap position (d + 0.5) * scale - 0.5 narrowed
 * to float; along x out-of-image taps clamp with weight 0 and the last column's horizontal pass is S[sx] * ONE; along y the rows
 * are clipped and the weights kept; 64-bit floats use float weights and double sums; 8-bit images use short weights
 * (round-to-even of weight * 2048), an int horizontal pass and uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2)
 * vertically; halving both axes exactly is INTER_AREA (mean of the 2 x 2 block: double sum * 0.25f, 8-bit (sum + 2) >> 2); an
 * image that already has the publish size is copied.  src: w0 x h0 (x channels, interleaved), dst: w x h, each on the host or
 * (flag) in HBM; the results feed chisel_hip_integrate_* directly.  Parity unpinned: OpenCV is not available here to generate
 * vectors; hand-computed cases of the rules above are in tests/test_publish_dense.py. */
int chisel_hip_condition_depth(const double *src, int w0, int h0, int src_on_device, float *dst, int w, int h, int dst_on_device,
                               double intrinsics_fx_fy_cx_cy[4], void *hip_stream);
int chisel_hip_condition_color(const uint8_t *src, int w0, int h0, int channels, int src_on_device, uint8_t *dst, int w, int h,
                               int dst_on_device, void *hip_stream);
/* CollaborativeServer::SendPointCloud (collaborative_server_system.cpp:318-381), the third thing PublishDenseInfo sends (:249): the
 * data array of its organised sensor_msgs::PointCloud2 -- w * h points of 16 bytes {float x = column, float y = row, float z =
 * (float)depth, int32 rgb = grey byte replicated}, all four words NaN unless 0.1 < z < 10.  depth: w x h doubles (the resized
 * map); color: the resized colour image, color_step bytes per row; the grey byte is the one at byte offset `column` of the row,
 * as mColorImage.at<uint8_t>(u, v) reads it whatever the channel count.  Both inputs on the host or both (flag) in HBM. */
int chisel_hip_publish_cloud(const double *depth, const uint8_t *color, int w, int h, int color_step, int src_on_device, void *points,
                             int dst_on_device, void *hip_stream);

/* ---- the step before that: the inverse-depth filter ----------------------------------------------
 * DepthFilter (server_pose_graph/src/dense_mapping/depth_filter.cpp): per-pixel Gaussian x uniform mixture filter of the
 * inverse depth a stereo matcher delivers; its state (a, b, mu, cov: four CV_64F maps) lives in HBM here.
 *   create   DepthFilter::DepthFilter(height, width)            depth_filter.cpp:130-142
 *   update   DepthFilter::Update(mUpdateMu, mUpdateCov)         depth_filter.cpp:177-259 (NormPdf :10-16)
 *            cov == NULL: cov_all for every pixel (depth_estimator.cpp:293); reciprocal != 0: the update is 1.0 / mu[i]
 *            (depth_estimator.cpp:286 fused in).  Arrays of width * height doubles, on the host or (flag) in HBM.
 *            Host arrays (pageable or pinned) have been consumed when update returns: the caller may overwrite or free them
 *            at once, and several updates may follow each other with no read between them.  Device arrays are read by a
 *            kernel on the null stream after update returns: they stay alive and unchanged until a later call on that
 *            stream (a read, say) has returned; mu and cov are both on the host or both in HBM.
 *   read     which = 0 GetA, 1 GetB, 2 GetInvDepth, 3 GetCov, 4 GetRatio (depth_filter.h:66-86), 5 the inverse-depth map
 *            DepthEstimator keeps (1e-5 where the ratio is below 0.5, depth_estimator.cpp:387-398), 6 the depth map 1.0 / that
 *            (server_keyframe.cpp:1117) -- the input of chisel_hip_condition_depth, so depth can stay in HBM from the
 *            matcher to the TSDF.
 *   device   the device the filter lives on (device_id of create, or the device that was current then): where arrays handed
 *            over with the on_device flags must be.
 * All arithmetic in double in the reference's order; exp() is the device library's (parity unpinned, tolerances in
 * tests/filter_cases.py).  PropogateDepth is not built: its only call site is commented out (server_pose_graph.cpp:891). */
typedef struct chisel_hip_depth_filter chisel_hip_depth_filter;
int chisel_hip_depth_filter_create(int height, int width, int device_id, chisel_hip_depth_filter **out);
int chisel_hip_depth_filter_destroy(chisel_hip_depth_filter *filter);
int chisel_hip_depth_filter_update(chisel_hip_depth_filter *filter, const double *mu, const double *cov, double cov_all, int reciprocal,
                                   int on_device);
int chisel_hip_depth_filter_read(chisel_hip_depth_filter *filter, int which, double *dst, int dst_on_device);
int chisel_hip_depth_filter_device(const chisel_hip_depth_filter *filter, int *device);

/* ---- the step before that: the stereo matcher (StereoMapper, the reference's only GPU code) --------------------------------
 * StereoMapper (server_pose_graph/src/dense_mapping/sgm_stereo_mapper.cpp, kernels calc_cost.cu): plane-sweep absolute-difference
 * cost over STEREO_DEP_CNT = 128 inverse depths i * dep_sample, four-path SGM, winner-takes-all with parabola sub-sample.  The cost
 * and SGM volumes ([height][width][128] floats, depth fastest: 314 MB at 640 x 480) and the depth map live in HBM.  Two ways in:
 * the float entries (set_reference / update / output) take images the caller has already resized and undistorted, with its own P2
 * weight map and sparse maps; the raw-image entries (set_camera and after, below) take the camera's mono8 frames and do the
 * reference's OpenCV work on the device too.  Same numbers as the reference bit for bit, except match-image samples: bilinear with
 * exact fp32 weights where the CUDA texture quantises them.  Images: width * height floats, on the host or (flag)
 * in HBM.
 *   default_params  dense_mapping_parameters.cpp:3-11 (pi1 16, pi2 64, tau_so 8, sgm_q1 1, sgm_q2 1, var_scale 1, nSparseRatio 15)
 *                   and DEP_SAMPLE = 1.0f / (0.11f * 460.95f) (dense_mapping_parameters.h:24,36-37)
 *   create          StereoMapper::StereoMapper (sgm_stereo_mapper.cpp:11-18); width, height >= 2 at run time (the reference
 *                   fixes 640 x 480); p == NULL: the defaults
 *   set_reference   InitReference (:55-123): the undistorted reference image and its P2 weight map; measurement count = 0
 *   update          Update (:125-199) -> ad_calc_cost (calc_cost.cu:20-233): count + 1, then the running mean of the AD cost.
 *                   R = K2 R_m^T R_r K1^-1, t = K2 R_m^T (t_r - t_m) as floats, row-major (:179-182)
 *   output          Output (:219-385): FuseSparseInfo (calc_cost.cu:684-736) with the sparse depth and distance maps
 *                   (both NULL: no prior; the reference's all -1 map changes nothing), the SGM volume zeroed, sgm2 right,
 *                   left, down, up (:365-546), filterCostKernel (:235-282) -> depth map (1000 where no minimum is accepted)
 *   clear           ClearRawCost (:202-216): cost, SGM and depth zeroed; the measurement count is NOT reset (the reference's)
 *   read            which = 0 cost volume f32, 1 SGM volume f32, 2 depth map f32, 3 depth map widened to f64
 *                   (depth_estimator.cpp:283): the input of chisel_hip_depth_filter_update(..., reciprocal = 1, on_device = 1);
 *                   4 / 5 the camera-size depth of the last output_image as f32 / f64 (5: the filter's input when the filter has
 *                   the camera size, as DepthEstimator's has, depth_estimator.cpp:276-297); both need set_camera
 * Every call runs on the null stream: update / output return before the kernels finish and the next call (also a depth-filter
 * call) is ordered after them; read waits. */
typedef struct {
    float pi1, pi2, tau_so, sgm_q1, sgm_q2, var_scale, sparse_ratio, dep_sample;
} chisel_hip_stereo_params;
typedef struct chisel_hip_stereo chisel_hip_stereo;
void chisel_hip_stereo_default_params(chisel_hip_stereo_params *p);
int chisel_hip_stereo_create(int width, int height, const chisel_hip_stereo_params *p, int device_id, chisel_hip_stereo **out);
int chisel_hip_stereo_destroy(chisel_hip_stereo *s);
int chisel_hip_stereo_set_reference(chisel_hip_stereo *s, const float *ref, const float *p2_weight, int on_device);
int chisel_hip_stereo_update(chisel_hip_stereo *s, const float *match, const float R[9], const float t[3], int on_device);
int chisel_hip_stereo_output(chisel_hip_stereo *s, const float *sparse_depth, const float *sparse_dist, int on_device);
int chisel_hip_stereo_clear(chisel_hip_stereo *s);
int chisel_hip_stereo_read(chisel_hip_stereo *s, int which, void *dst, int dst_on_device);
/* The raw-image path: StereoMapper's OpenCV steps, restated from OpenCV 4's published algorithms and run on the device.  Parity
 * with the real OpenCV is unpinned (OpenCV is not a dependency; the restatement in tests/stereo_prep_restated.py fixes each rule).
 *   set_camera             InitIntrinsic (sgm_stereo_mapper.cpp:20-52): K = (fx, fy, cx, cy) of the real_w x real_h camera, fx, cx
 *                          divided by real_w / (double)width, fy, cy by real_h / (double)height; D = (k1, k2, p1, p2, k3) (the
 *                          reference passes k3 = 0, depth_estimator.cpp:588).  Builds both cameras' cv::undistort maps once, on
 *                          the host in double (they depend only on K, D and the size; the reference rebuilds them per call) and
 *                          keeps them in HBM.  Needs width, height >= 9 (the border of the 9-tap Sobel).
 *   set_reference_image    InitReference (:55-123) on a real_w x real_h mono8 image (ServerKeyFrame::m_mImage), row step `step`
 *                          bytes, on the host or (flag) in HBM: cv::resize to width x height (8-bit INTER_LINEAR, the rules of
 *                          chisel_hip_condition_color), cv::undistort (remap with the fixed-point bilinear table, BORDER_CONSTANT),
 *                          the f32 reference image; the P2 weight map (float)(((1.5 m) m) m / (1 + g (g g)) * 1.0 + 0.8), g =
 *                          |Sobel(5,5,9)|, m = mean g; the thresholded Sobel(3,0,7) / Sobel(0,3,7) maps as masks g >= mean +
 *                          stddev && g > 0 (all Output reads of them); Sobel kernels of getSobelKernels, BORDER_REFLECT_101, exact
 *                          in int32; mean and stddev from exact int64 sums.  Measurement count = 0.
 *   update_image           Update (:125-199): the match image resized and undistorted with camera 2, R and t from the two
 *                          camera-to-world poses (chisel_hip_stereo_homography with the scaled K), then the cost pass of update
 *   bind_sparse_points     BindSparsePoints (sgm_stereo_mapper.h:60-66): n points, depth[n] and xy[2 n] (x, y in real-image
 *                          pixels, as server_keyframe.cpp:936-960 builds them), host arrays, copied; n = 0 clears
 *   output_image           Output in full (:219-422): the sparse depth / distance maps rasterised on the device with every quirk of
 *                          the window loop (:229-357: swapped x / y scales, int truncation, bounds from the masks read at the flat
 *                          index (nY + vs) * width + nX + us -- a read outside the map counts as 0, where the reference is
 *                          undefined --, the outward propagation, the border skip, a write when dist < ratio that stores ratio^2;
 *                          overlapping windows give the sequential loop's result), FuseSparseInfo, SGM, WTA, then the f32
 *                          INTER_LINEAR cv::resize of the depth to real_w x real_h (float weights and products; 1000 is
 *                          interpolated like any other value) for read-outs 4 and 5
 *   homography             host arithmetic, no device: R = K2 Rm^T Rr K1^-1 and t = K2 Rm^T (tr - tm) (:179-182) in double, every
 *                          3 x 3 product an entry at a time a0 b0 + a1 b1 + a2 b2 left to right, K1^-1 the closed form cv::invert
 *                          (DECOMP_LU) takes for 3 x 3 (det3 along the first row, d = 1. / det, adjugate entries times d); narrowed
 *                          to float.  K = (fx, fy, cx, cy), R row-major, poses camera-to-world.
 * A raw entry before set_camera, a work size below 9 x 9, a step below real_w or n < 0 is CHISEL_HIP_ERR_INVALID, nothing launched. */
int chisel_hip_stereo_set_camera(chisel_hip_stereo *s, int real_w, int real_h, const double K1[4], const double D1[5], const double K2[4],
                                 const double D2[5]);
int chisel_hip_stereo_set_reference_image(chisel_hip_stereo *s, const uint8_t *img, int step, int on_device);
int chisel_hip_stereo_update_image(chisel_hip_stereo *s, const uint8_t *img, int step, const double ref_R_wc[9], const double ref_t_wc[3],
                                   const double match_R_wc[9], const double match_t_wc[3], int on_device);
int chisel_hip_stereo_bind_sparse_points(chisel_hip_stereo *s, const double *depth, const double *xy, int n);
int chisel_hip_stereo_output_image(chisel_hip_stereo *s);
int chisel_hip_stereo_homography(const double K1[4], const double K2[4], const double Rr[9], const double tr[3], const double Rm[9],
                                 const double tm[3], float R[9], float t[3]);

/* Binary dump / restore of the whole map (the correct counterpart of chisel_ros FillChunkMessage,
 * Serialization.h:31-84, whose bit packing loses data; also checkpoint / resume).  File: 32-byte header
 * {"CHSLHIP1", int32 chunk edge, float resolution, int32 has_colour, 4 spare bytes, int64 n_chunks}, then per chunk, in
 * ascending id order: int32 id[3], float sdf[V], float weight[V], (uint8 rgbw[4 V] if has_colour).  load replaces the
 * map's contents (Reset first); chunk size, resolution and colour must match the map's. */
int chisel_hip_save_map(chisel_hip_map *map, const char *path);
int chisel_hip_load_map(chisel_hip_map *map, const char *path);

/* ---- one map over several GPUs of the node, inside one process -------------------------------------------------------- */
/* The reference has one chisel::Chisel object per map (Chisel.h:38-230) and one calling thread; a C++ caller that links this
 * library (chisel_ros) cannot start one process per GPU.  chisel_hip_create_group returns a handle that every entry point of
 * this header accepts like any other map: behind it one shard map per entry of device_ids[] (n_shards = n_devices, shard i on
 * device_ids[i]; chunk ownership = chisel_hip_chunk_owner; a device may be named several times).  The library hands every
 * shard every frame (device frames are copied peer-to-peer to the shards on other devices), all shards integrate concurrently,
 * chisel_hip_update_meshes exchanges the neighbour chunks between the shards, queries go to the owner, listings / PLY / map
 * dumps are merged in ascending id order and equal a single map's.  cfg->device_id, n_shards and shard_rank are ignored.
 * Not available on a group: chisel_hip_set_stream, chisel_hip_record_event (one stream / event cannot span GPUs: use
 * chisel_hip_synchronize), and the shard-to-shard calls (export / import / drop ghost chunks, update_meshes_of). */
int chisel_hip_create_group(const chisel_hip_config *cfg, const int *device_ids, int n_devices, chisel_hip_map **out);

/* ---- view frustum (host arithmetic, no GPU needed) -------------------------------------------------------------- */
/* PinholeCamera::SetupFrustum (src/camera/PinholeCamera.cpp:55-59) -> Frustum::SetFromParams / SetFromVectors
 * (src/geometry/Frustum.cpp:143-219), with the reference's quirks (fy is used for both focal lengths, cx is ignored) and fp32
 * operation order: the frustum the integration enumerates its candidate chunks from, for the caller's use
 * (chisel_ros draws it: ChiselServer.cpp:97-134).
 *   corners[8][3]   farTopLeft, farTopRight, farBotLeft, farBotRight, nearBotRight, nearTopLeft, nearTopRight, nearBotLeft
 *                   (Frustum::GetCorners, Frustum.cpp:181-188)
 *   lines[24][3]    the 12 edges as point pairs in the order of Frustum::GetLines (Frustum.cpp:190-217)
 *   planes[6][4]    far, near, top, bottom, left, right: normalised normal xyz + offset as Plane(p1, p2, p3) leaves them
 *                   (src/geometry/Plane.cpp:44-52: the offset is NOT divided by the normal's length)
 * Any of the three outputs may be NULL. */
int chisel_hip_frustum(const float pose_c2w[12], float fy, float cy, int width, int height, float near_plane, float far_plane,
                       float *corners, float *lines, float *planes);
/* Frustum::SetFromVectors (src/geometry/Frustum.cpp:155-219) itself, for a caller that has its own view vectors (what
 * Frustum::SetFromOpenGLViewProjection, :124-141, ends in): same outputs, same fp32 operation order. */
int chisel_hip_frustum_from_vectors(const float forward[3], const float pos[3], const float right[3], const float up[3], float near_plane,
                                    float far_plane, float fov, float aspect, float *corners, float *lines, float *planes);

/* ---- meshing a sharded map with shells -----------------------------------------------------------------
 * What a chunk's mesh reads of a neighbour chunk is a shell one or two voxels thick (cube corners, gradients around the vertices, the
 * nearest voxel's colour: SURVEY.md 8e's "faces"), not the whole chunk.  A "box code" names the part of a ghost chunk that travels:
 * two bits per axis (x: bits 0-1, y: 2-3, z: 4-5), 0 = every coordinate, 1 = {0, 1}, 2 = {N - 1}, 3 = {0, 1, N - 1}; chisel_hip_shell_volume gives its
 * number of voxels; the payload of an item (x, y, z, box) is its box in z, y, x order.
 *   chisel_hip_dirty_ids_device  the chunks updated since the last recompute as a DEVICE int array: out[0] = n, then n entries
 *                                (x, y, z, flag) -- flag 0: the chunk was updated (its 27-neighbourhood is meshesToUpdate, Chisel.h:175-189),
 *                                flag 1: an entry of meshesToUpdate kept on the host; nothing is waited for (record_event orders the
 *                                collective that gathers the ranks' arrays)
 *   chisel_hip_mesh_shell_plan   the host planner of rounds 3-4, kept as the independent check of the device plan below (tests/
 *                                test_sharded_cpu.py); no entry point consumes its items.  Host arithmetic, identical on every rank:
 *                                from the gathered entries the ids `rank` meshes (jobs) and the ghosts it needs as items
 *                                (owner, x, y, z, box) -- one or more boxes per ghost, ascending by owner, id, box */
int chisel_hip_dirty_ids_device(chisel_hip_map *map, int *out_dev, int capacity);
int chisel_hip_mesh_shell_plan(const int *entries, int64_t n_entries, int n_shards, int rank, int shard_block, int *jobs, int64_t max_jobs,
                               int64_t *n_jobs, int *items, int64_t max_items, int64_t *n_items);
/* The sharded recompute without host planning (round 5; cvids_amd/sharded.py: ShardedChisel.UpdateMeshes): from the
 * all-gathered list of updated chunks (per rank 1 + 4 * cap ints: count, then (x, y, z, flag) entries -- chisel_hip_dirty_ids_device)
 * every shard derives ON THE DEVICE its own jobs, the shells it sends to every peer and how much it receives from each.
 * chisel_hip_shell_plan_device: out[0] = jobs of this shard, out[1] = ghost chunks its earlier recomputes created (a running total), out[2] = largest per-rank count of the list (> cap: gather again with more
 * room), out[3] = items sent, then (items, voxels) per peer sent, then per peer received -- the one host wait of a sharded recompute.
 * chisel_hip_export_shells_packed writes one byte segment per peer, back to back in rank order (chisel_hip_shell_segment_bytes each:
 * heads, items that say where their voxels are, sdf | weight | rgbw), the caller's all-to-all moves them, chisel_hip_import_shells_packed
 * turns what arrived into ghost chunks (the buffer stays untouched until chisel_hip_drop_ghost_chunks), chisel_hip_update_meshes_planned
 * recomputes the plan's jobs.  No reference counterpart: the reference has one process and one map (Chisel.h:150-195). */
int chisel_hip_shell_plan_device(chisel_hip_map *map, const int *gathered_dev, int world, int capacity, int64_t *out);
int64_t chisel_hip_shell_segment_bytes(chisel_hip_map *map, int64_t items, int64_t voxels);
int chisel_hip_export_shells_packed(chisel_hip_map *map, void *out_dev, int64_t bytes);
int chisel_hip_import_shells_packed(chisel_hip_map *map, const void *in_dev, int64_t bytes);
int chisel_hip_update_meshes_planned(chisel_hip_map *map);
/* The same recompute with NO host wait (round 6; ShardedChisel.UpdateMeshes(wait_free=True)).  The host reads nothing of the plan: every
 * (sender, receiver) segment has `seg_stride` bytes to itself (a multiple of 16, agreed between the ranks beforehand -- from what the previous
 * recompute needed), the exchange is an all-to-all of equal splits, and the steps behind it read the heads of the received segments.
 *   chisel_hip_shell_plan_queue    queues the plan and, behind it, the export of `world` segments of seg_stride bytes into out_dev, whose first
 *                                  workgroup also writes this rank's STATUS into status_dev (CHISEL_HIP_SHELL_STATUS_INTS ints on the device):
 *                                  [0] bits that call the recompute off (1: a rank's dirty list exceeds `capacity`, 2: the plan's
 *                                  tables overflowed, 4: a segment exceeds seg_stride), [1] largest per-rank dirty count, [2] bytes of this
 *                                  rank's largest segment, [3] its jobs, [4] items it receives, [5] items it sends, [6] voxels it receives,
 *                                  [7] ghost chunks its earlier recomputes created.  The caller all-reduces the vector with MAX (in place)
 *                                  in front of the exchange.  send_items_hint: [5] of the previous recompute (a grid size; 0 = unknown)
 *   chisel_hip_import_shells_fixed ghosts from the received segments; then chisel_hip_update_meshes_planned and chisel_hip_drop_ghost_chunks
 *                                  as before -- all of it queued, and all of it a no-op ON THE DEVICE if word 0 of the all-reduced status
 *                                  is not zero (no ghost, no mesh, no dirty flag cleared: on every rank alike)
 *   chisel_hip_shell_commit        once the host has read the all-reduced status (any time before it next changes the map): settles the mesh
 *                                  step; aborted != 0: the recompute did not happen -- make it again with chisel_hip_shell_plan_device */
#define CHISEL_HIP_SHELL_STATUS_INTS 8
int chisel_hip_shell_plan_queue(chisel_hip_map *map, const int *gathered_dev, int world, int capacity, int64_t seg_stride, int *status_dev, void *out_dev,
                                int send_items_hint);
int chisel_hip_import_shells_fixed(chisel_hip_map *map, const void *in_dev, int64_t seg_stride, const int *status_dev, int jobs_hint, int items_hint);
int chisel_hip_shell_commit(chisel_hip_map *map, int aborted);
int64_t chisel_hip_shell_volume(int box, int chunk_edge);

/* ---- measurement ------------------------------------------------------------------------------------ */
/* accumulated since creation / last reset_counters; out has CHISEL_HIP_NUM_COUNTERS entries */
int chisel_hip_get_counters(chisel_hip_map *map, uint64_t *out, int reset_counters);
/* ChunkManager::PrintMemoryStatistics (src/ChunkManager.cpp:641-678; the reference calls it after every depth-only frame,
 * Chisel.h:111): the census of Chunk::ComputeStatistics (src/Chunk.cpp:89-116) over every resident chunk -- voxels with weight > 0 and
 * sdf < 0 / >= 0, voxels with weight <= 0 -- as one reduction kernel, the sum of the weights (a double here; the reference adds floats
 * in hash-map order), and the smallest / largest resident chunk id per axis, from which the caller forms the bounds
 * (min = chunk_size * id_min * resolution, max = chunk_size * (id_max + 1) * resolution, Chunk.cpp:65-70).  n_chunks == 0: the ids are
 * undefined. */
typedef struct chisel_hip_statistics {
    int64_t n_unknown, n_known_inside, n_known_outside;
    double total_weight;
    int64_t n_chunks;
    int32_t id_min[3], id_max[3];
} chisel_hip_statistics;
int chisel_hip_memory_statistics(chisel_hip_map *map, chisel_hip_statistics *out);
/* A counter that moves whenever chunks appear or disappear by anything other than integration (garbage collection, reset, upload, map
 * load, ghost import / drop): together with chisel_hip_num_chunks -- integration only ever adds chunks -- it tells a caller that keeps
 * mirrors of the chunk map (ChunkManager::GetChunks, ChunkManager.h:65-73) whether they are still current. */
int chisel_hip_topology_epoch(chisel_hip_map *map, uint64_t *out);
/* ChunkManager::GetChunkIDsIntersecting(const Frustum &, ChunkIDList *) (src/ChunkManager.cpp:182-212) for a frustum given as
 * chisel_hip_frustum returns it (corners[8][3], planes[6][4] in the order far, near, top, bottom, left, right): the ids in the
 * reference's order (x outer, z inner).  ids may be NULL (count only); at most max_ids are written. */
int chisel_hip_candidates(const float corners[24], const float planes[24], const int chunk_size[3], float voxel_resolution, int *ids,
                          int64_t max_ids, int64_t *count);
/* ChunkManager::GetChunkIDsIntersecting(const PointCloud &, const Transform &, float truncation, float maxDist, ChunkIDList *)
 * (src/ChunkManager.cpp:214-257): the chunks the segments point -+ truncation along the viewing rays pass through (Raycast over the
 * chunk grid, points further than max_dist skipped) -- the listing step of chisel_hip_integrate_pointcloud on its own, same kernel.
 * The reference returns them in the order of an unordered_map; here ascending (x, then y, then z).  A shard lists the chunks it owns.
 * ids may be NULL (count only); at most max_ids are written. */
int chisel_hip_cloud_candidates(chisel_hip_map *map, const chisel_hip_pointcloud *cloud, int *ids_xyz, int64_t max_ids, int64_t *count);
/* ChunkManager::ComputeNormalsFromGradients (src/ChunkManager.cpp:609-626; stages bit 0: a normal is overwritten where the gradient
 * lookup of its vertex succeeds, kept otherwise) and ChunkManager::ColorizeMesh / InterpolateColor (:628-639, :501-573; stages bit 1)
 * for a caller's own vertex list (host arrays of 3 n floats). */
int chisel_hip_shade_vertices(chisel_hip_map *map, const float *vertices, int64_t n, float *normals, float *colors, int stages);
/* A camera for chisel_hip_render_view: pose and intrinsics as in chisel_hip_depth_frame, and the spacing of the samples along the
 * optical axis. */
typedef struct {
    int width, height;
    float pose[12];          /* camera -> world, row-major 3 x 4                                         */
    float fx, fy, cx, cy;
    float near_plane, far_plane;
    float step;              /* z-distance between two samples of a ray [m]; <= 0: the map's voxel resolution */
} chisel_hip_view;          /* 84 bytes */
/* Not in the reference: what the map holds as a camera at `view` sees it.  Pixel (col, row) looks along the ray through (col + 0.5,
 * row + 0.5) and takes K = floor((far - near) / step) + 1 samples ChunkManager::GetSDF (nearest voxel) at the z-depths near + k step;
 * its depth is where the distance changes from positive to <= 0 between two consecutive observed samples, interpolated linearly, as
 * z-depth along the optical axis (what DepthImage holds: the image can go straight into chisel_hip_integrate_depth of another map).
 * normals / colors (each 3 floats per pixel, or NULL): ChunkManager::ComputeNormalsFromGradients' normal and InterpolateColor's colour
 * at the hit point, as chisel_hip_shade_vertices gives them.  A pixel without a hit -- nothing observed along the ray, or the ray comes
 * up behind a surface -- is NaN in all three; so is the normal where the gradient lookup fails.  DESIGN.md "Rendering a view" has the
 * definition to the bit.  The map is only read.  on_device: the outputs are device pointers, filled on the map's stream without a wait;
 * otherwise host arrays, complete on return.  CHISEL_HIP_ERR_INVALID: colors on a map without colour voxels, K < 1 or K > 65536, a
 * non-positive size; CHISEL_HIP_ERR_UNSUPPORTED: a group or one shard of several (a ray needs every owner's voxels). */
int chisel_hip_render_view(chisel_hip_map *map, const chisel_hip_view *view, float *depth, float *normals, float *colors, int on_device);
/* Not in the reference: the map read at n positions of the caller's in one launch (one thread per position; DESIGN.md "Querying points
 * and rays" has the definition to the bit).  Any output may be NULL; what is not asked for is not computed.  Per position p:
 *   found     bit 0: ChunkManager::GetSDF(p) returns true (src/ChunkManager.cpp:476-499); bit 1: GetSDFAndGradient(p) does (:449-474) --
 *             evaluated only when `gradient` is asked for, 0 otherwise
 *   sdf       the stored distance of the voxel GetSDF reads (the float whose double chisel_hip_get_sdf returns); NaN where bit 0 is clear
 *   weight    the weight of that voxel wherever its chunk is resident and the linear voxel id in range (Chunk.h:81-84), weights
 *             <= 1e-12 included; NaN elsewhere
 *   gradient  3 floats: what chisel_hip_get_sdf_and_gradient returns; NaN x 3 where bit 1 is clear
 *   colors    3 floats: ChunkManager::InterpolateColor(p) (:501-573), what chisel_hip_shade_vertices (stage 2) writes, its (0, 0, 0)
 *             answers included
 * A position with a non-finite component is answered without a look at the map: found 0, NaN in every other output.  on_device:
 * positions and outputs are device pointers, the kernel goes on the map's stream (behind the event of a chisel_hip_wait_event or
 * chisel_hip_order_map_after_stream before it, which says that the positions are ready) and nothing is waited for; otherwise host
 * arrays, complete on return.  The map is only read.  CHISEL_HIP_ERR_UNSUPPORTED: a group or one shard of several.  Then
 * CHISEL_HIP_ERR_INVALID for n < 0; then n == 0 is CHISEL_HIP_OK, launches nothing and looks at no other argument; then
 * CHISEL_HIP_ERR_INVALID for null positions, no output at all, or colors on a map without colour voxels. */
int chisel_hip_query_points(chisel_hip_map *map, const float *positions /* 3 n */, int64_t n, uint8_t *found, float *sdf, float *weight,
                            float *gradient /* 3 n */, float *colors /* 3 n */, int on_device);
/* A ray for chisel_hip_cast_rays: the samples are origin + t direction, t from t_near to t_far.  The direction is used as given (t is
 * in units of its length: unit directions give Euclidean range).  Device arrays of rays are 16-byte aligned. */
typedef struct {
    float origin[3];
    float direction[3];
    float t_near, t_far;
} chisel_hip_ray;           /* 32 bytes */
#define CHISEL_HIP_RAY_MAX_SAMPLES 65536 /* per ray (chisel_hip_render_view's limit) */
/* Not in the reference: chisel_hip_render_view's march along n rays of the caller's, one ray per lane in the caller's order.  Ray r
 * takes K = floor((t_far - t_near) / step) + 1 samples (at most CHISEL_HIP_RAY_MAX_SAMPLES; none where the quotient is negative or NaN,
 * or the ray has a non-finite origin, direction or t_near) ChunkManager::GetSDF (nearest voxel) at t_k = t_near + k step; step <= 0:
 * the map's voxel resolution.  It ends at the first observed sample with a distance <= 0.
 *   status   1 (hit): the sample before the end is observed with a distance > 0; 2: the ray ended otherwise (it came up behind a
 *            surface); 0: it took all its samples without ending, or took none
 *   t_hit    status 1: where the distance changes sign between the two samples, interpolated linearly; NaN otherwise.  Required.
 *   normals / colors (3 floats per ray): as chisel_hip_render_view shades a hit, at origin + t_hit direction; NaN without a hit
 * status, normals and colors may be NULL.  A ray's outputs depend on that ray and the map alone, not on its neighbours or its place
 * in the array.  The rays of a chisel_hip_view (direction = R (xc, yc, 1), t_near = near, t_far = far) give chisel_hip_render_view's
 * image bit for bit.  on_device, the map, n == 0 and the error codes: as chisel_hip_query_points; also CHISEL_HIP_ERR_INVALID for a
 * NaN step or a null t_hit.  DESIGN.md "Querying points and rays" has the definition to the bit. */
int chisel_hip_cast_rays(chisel_hip_map *map, const chisel_hip_ray *rays, int64_t n, float step, float *t_hit, uint8_t *status,
                         float *normals /* 3 n */, float *colors /* 3 n */, int on_device);
/* A window of voxels for chisel_hip_distance_field.  A global voxel index per axis is chunk_id * N + voxel_coordinate (floor division
 * for negative indices); origin is the index of the window's first voxel, dims = (nx, ny, nz) its extent, radius R the reach of the
 * transform in voxels (1 ... 64). */
typedef struct {
    int origin[3];
    int dims[3];
    int radius;
    int unknown_is_obstacle;   /* nonzero: unknown voxels are obstacles too */
    float surface_offset;      /* metres: a voxel is occupied when it is observed with sdf < surface_offset */
} chisel_hip_distance_window;   /* 36 bytes */
/* Not in the reference: how far the nearest obstacle is from every voxel of a window, and whether the voxel was ever observed -- what
 * a planner asks of a box around the robot.  A truncated, exact Euclidean distance transform in squared voxel units (integers: the
 * answer does not depend on the algorithm).  Element (x, y, z) of every output sits at (z ny + y) nx + x.
 *   state (uint8)     0 unknown: the voxel's chunk is not resident (or its id is outside the addressable range), or its weight reads
 *                     as unobserved by ChunkManager::GetSDF's rule (src/ChunkManager.cpp:489); 2 occupied: observed and
 *                     sdf < surface_offset (one fp32 compare); 1 free: observed otherwise
 *   dist2 (int32)     min |v - o|^2 over the obstacle voxels o of the MAP (not of the window: the seeds are read over the window
 *                     widened by R on every side) with |v - o|^2 <= R^2; -1 where there is none.  Obstacles: the occupied voxels,
 *                     with unknown_is_obstacle the unknown ones too
 *   distance (float)  (float)(sqrt((double)dist2) * (double)voxel_resolution), +inf where dist2 is -1; read from a table the host computes
 * Any of the three may be NULL, not all.  on_device, the stream, groups and shards: as chisel_hip_query_points.  The map is only read;
 * the scratch is kept in the map, grown on demand and freed with it.  CHISEL_HIP_ERR_INVALID (nothing is touched): null window, no
 * output, a dimension < 1, R < 1 or R > 64, a NaN surface_offset, a coordinate of the widened window beyond +-2^30;
 * CHISEL_HIP_ERR_UNSUPPORTED: a widened window of more than 2^30 voxels.  DESIGN.md 3.11 "Distance field" has the definition. */
int chisel_hip_distance_field(chisel_hip_map *map, const chisel_hip_distance_window *window, uint8_t *state, int32_t *dist2, float *distance,
                              int on_device);
/* ---- frontier voxels of a window, clustered and tabulated (DESIGN.md 3.18 "Frontiers") ----
 * Not in the reference: where the observed space ends -- what an exploration planner, a next-best-view step or a task allocator asks
 * first.  The window is chisel_hip_distance_window's: origin (global voxel index per axis, chunk_id * N + voxel coordinate) and
 * dims = (nx, ny, nz); element (x, y, z) of a per-voxel output sits at (z ny + y) nx + x, the voxel's LINEAR INDEX.  The STATE of a
 * voxel (0 unknown, 1 free, 2 occupied) is chisel_hip_distance_field's, bit for bit: the same residency rule, look-up guard and weight
 * rule, one fp32 compare sdf < surface_offset.  A voxel of the window is a FRONTIER voxel when it is free and at least
 * min_unknown_faces (1 ... 6) of its six face neighbours are unknown; the neighbours are voxels of the MAP (read over the window
 * widened by one voxel on every side), and unknown_faces(v) is that count.  The CLUSTERS are the connected components of the frontier
 * voxels of the window under connectivity 6, 18 or 26 (offsets with 1, <= 2, <= 3 non-zero coordinates, each -1 ... 1); voxels outside
 * the window join nothing.  A cluster's ROOT is its smallest linear index; clusters are numbered by ascending root; a cluster is KEPT
 * when it has at least min_voxels (>= 1) voxels, and the kept clusters are renumbered 0 ... K - 1 in the same order. */
typedef struct {
    int origin[3];
    int dims[3];
    int min_unknown_faces;     /* 1 ... 6 */
    int connectivity;          /* 6, 18 or 26 */
    int min_voxels;            /* >= 1: clusters with fewer voxels are dropped */
    float surface_offset;      /* metres: a voxel is occupied when it is observed with sdf < surface_offset */
} chisel_hip_frontier_window;   /* 40 bytes */
typedef struct { int64_t unknown, free, occupied, frontier, clusters, largest_voxels, kept_clusters, kept_voxels; } chisel_hip_frontier_totals;
/* Outputs, each optional:
 *   state (uint8 per voxel)   the distance field's, bit for bit
 *   label (int32 per voxel)   the kept cluster's number; -1 for a voxel that is not a frontier voxel; -2 for a frontier voxel of a
 *                             cluster that was dropped
 *   voxels (4 int32 a row, room for capacity_voxels rows)   (x, y, z, cluster) of every kept frontier voxel, window-relative, in
 *                             ascending linear index
 *   cluster_table (12 int64 a row, room for capacity_clusters rows, HOST memory whatever on_device says)   per kept cluster: root,
 *                             voxels, sum x, sum y, sum z (window-relative), min x, y, z, max x, y, z, sum of unknown_faces.  The
 *                             centre in metres is the caller's arithmetic: ((origin + sum / voxels) + 0.5) * resolution
 *   totals (required, host)   unknown, free and occupied voxels of the window, frontier voxels, clusters, the largest cluster's
 *                             voxels, kept clusters, kept voxels
 * on_device says where state, label and voxels live.  Everything is queued on the map's stream behind what is queued; the host waits
 * once, for the totals (pinned memory); with on_device nothing is waited for behind the launches that write the arrays -- except for
 * cluster_table, whose rows are written to pinned memory behind that wait and waited for.  Host arrays are staged, copied out once
 * with exactly their live rows, and complete on return.  With no array asked for (a list or a table with capacity 0 is not asked
 * for) the call is the size query: totals is filled and nothing else is written.  A capacity below its total (kept_voxels,
 * kept_clusters) is refused with CHISEL_HIP_ERR_INVALID, totals filled and nothing else written, so that the caller can retry.  The
 * map is only read; the scratch (two bits per voxel of the widened window, four bits, 12 bytes and an eighth of a byte per voxel of
 * the window; 96 bytes per kept cluster when the table is asked for) is kept in the map, grown on demand and freed with it.  No float
 * is computed after the one compare: the answer is a pure function of the map and the window.
 * Refused with nothing written, in this order: CHISEL_HIP_ERR_UNSUPPORTED for a group, CHISEL_HIP_ERR_INVALID for a null map,
 * CHISEL_HIP_ERR_UNSUPPORTED for one shard of several; then CHISEL_HIP_ERR_INVALID for a null window, null totals, a dimension < 1,
 * min_unknown_faces outside 1 ... 6, a connectivity other than 6 / 18 / 26, min_voxels < 1, a NaN surface_offset, a negative
 * capacity, a capacity without its array, a coordinate of the widened window beyond +-2^30; then CHISEL_HIP_ERR_UNSUPPORTED for a
 * window of more than 2^26 voxels. */
int chisel_hip_frontiers(chisel_hip_map *map, const chisel_hip_frontier_window *window, uint8_t *state, int32_t *label,
                         int64_t capacity_voxels, int32_t *voxels, int64_t capacity_clusters, int64_t *cluster_table, int on_device,
                         chisel_hip_frontier_totals *totals);
/* ---- travel cost over free space from seed voxels (DESIGN.md 3.19 "Travel field") ----
 * Not in the reference: can the robot get there, and how far is the way -- a planner's third question after the distance to the nearest
 * obstacle and the frontiers.  The window is chisel_hip_distance_window's: origin and dims = (nx, ny, nz); every per-voxel array is
 * [z][y][x], element (x, y, z) at the LINEAR INDEX (z ny + y) nx + x.  The STATE of a voxel (0 unknown, 1 free, 2 occupied) is
 * chisel_hip_distance_field's, bit for bit: one fp32 compare sdf < surface_offset.  A voxel of the window is TRAVERSABLE when it is free
 * and, with clearance r >= 1, no obstacle voxel o of the MAP has |v - o|^2 <= r^2: exactly chisel_hip_distance_field at radius r
 * reading dist2 == -1, with the same unknown_is_obstacle rule, read beyond the window's rim.  With clearance 0 only the voxel's own
 * state counts and no distance transform is run.  Voxels outside the window are not traversable.  The MOVES are the offsets of
 * connectivity 6, 18 or 26 as the frontiers define them; a move with k non-zero coordinates costs step_cost[k - 1] (face, edge,
 * corner; each 1 ... 65535, all three checked at every connectivity) and needs only its two end voxels traversable: nothing is checked
 * about cut corners, the clearance is the caller's tool for that.  The SEEDS are n_seeds (1 ... 2^20) rows of window-relative
 * (x, y, z) int32, HOST memory always; a seed on a voxel that is not traversable is ignored and counted, duplicates are harmless.
 * COST(v) is the least sum of move costs over paths of traversable voxels from any used seed to v provided the sum is <= max_cost
 * (0 ... 2^30), else -1; a seed has cost 0; no candidate exceeds 2^30 + 65535.  STEP(v) is 13 at a seed (cost 0), 255 at an unreached
 * voxel, otherwise the smallest code (dz + 1) 9 + (dy + 1) 3 + (dx + 1) among the moves o of the connectivity with
 * cost(v + o) + cost_of(o) == cost(v): computed from the converged costs alone; following steps strictly lowers the cost and ends at a
 * seed.  TARGETS (optional) are n_targets rows of int32 (x, y, z, group) -- exactly the `voxels` list chisel_hip_frontiers writes --
 * with n_groups >= 1; a row with a coordinate outside the window or a group outside 0 ... n_groups - 1 is ignored and counted. */
typedef struct {
    int origin[3];
    int dims[3];
    int connectivity;          /* 6, 18 or 26 */
    int step_cost[3];          /* face, edge, corner: 1 ... 65535 each */
    int max_cost;              /* 0 ... 2^30 */
    int clearance;             /* 0 ... 64 voxels */
    int unknown_is_obstacle;   /* for the clearance: unknown voxels are obstacles too */
    float surface_offset;      /* metres: a voxel is occupied when it is observed with sdf < surface_offset */
} chisel_hip_travel_window;     /* 56 bytes */
typedef struct {
    int64_t unknown, free, occupied, traversable;   /* voxels of the window */
    int64_t seeds_used, seeds_ignored;
    int64_t reached, largest_cost;                  /* voxels with a cost; the largest of them, -1 without one */
    int64_t targets_reached, targets_ignored;
    int64_t rounds, tile_visits;                    /* diagnostics of the implementation: round launches that found a flagged tile,
                                                       tiles relaxed over all rounds.  Not part of the definition */
} chisel_hip_travel_totals;     /* 96 bytes */
/* Outputs, each optional:
 *   cost (int32 per voxel), step (uint8 per voxel), state (uint8 per voxel)
 *   group_table (4 int64 a row, n_groups rows, HOST memory whatever on_device says)   rows of the group, reached rows, the least
 *                             cost over the reached rows (-1 without one), the smallest linear index among the rows with that cost
 *                             (-1 without one)
 *   totals (required, host)
 * on_device says where cost, step, state and targets live.  Everything is queued on the map's stream behind what is queued.  The host
 * waits once per TRAVEL_ROUNDS_PER_WAIT relaxation rounds and once for the totals, so every output is complete on return.  With no
 * array and no table asked for the call is the size and reachability query: only totals is filled.  The map is only read; the scratch
 * (two bits per voxel of the window widened by one, a bit and 4 bytes per voxel -- 8 with a clearance, beside the distance field's own
 * scratch --, 8 bytes per tile of 16 x 16 x 8 voxels, 12 bytes per seed, 32 per group) is kept in the map, grown on demand and freed
 * with it.  Integers throughout: the same call gives the same bytes.
 * Refused with nothing written, in this order: CHISEL_HIP_ERR_UNSUPPORTED for a group, CHISEL_HIP_ERR_INVALID for a null map,
 * CHISEL_HIP_ERR_UNSUPPORTED for one shard of several; then CHISEL_HIP_ERR_INVALID for a null window, null seeds, null totals, n_seeds
 * outside 1 ... 2^20, a dimension < 1, a seed outside the window, a connectivity other than 6 / 18 / 26, a step_cost outside
 * 1 ... 65535, max_cost outside 0 ... 2^30, clearance outside 0 ... 64, a NaN surface_offset, a negative count, more than 2^26 targets
 * or groups, a target count without targets, targets without n_groups >= 1, a group table without targets, a coordinate of the window
 * widened by max(clearance, 1) beyond +-2^30; then CHISEL_HIP_ERR_UNSUPPORTED for a window of more than 2^26 voxels, or with a
 * clearance one that widened by it holds more than 2^30. */
int chisel_hip_travel_field(chisel_hip_map *map, const chisel_hip_travel_window *window, const int32_t *seeds, int64_t n_seeds,
                            const int32_t *targets, int64_t n_targets, int64_t n_groups, int32_t *cost, uint8_t *step, uint8_t *state,
                            int64_t *group_table, int on_device, chisel_hip_travel_totals *totals);
/* Needs no device (as chisel_hip_align_solve): walks the steps of a chisel_hip_travel_field result in HOST memory from the voxel `from`
 * (window-relative x, y, z) to its seed and writes (x, y, z) rows, both ends included; *length is the number of rows.
 * CHISEL_HIP_ERR_INVALID for a null argument, a negative capacity, a dimension < 1 or more than 2^26 voxels, a start outside the
 * window, an unreached start (255), a code that is no move, a step that leaves the window, a walk longer than the window has voxels,
 * a capacity below the length -- then *length is filled all the same (and the first `capacity` rows written), so that the caller can
 * retry. */
int chisel_hip_travel_path(const uint8_t *step, const int dims[3], const int from[3], int64_t capacity, int32_t *path, int64_t *length);
/* Not in the reference: the normal equations of one Gauss-Newton step that aligns a depth frame to the map (point-to-surface against the
 * TSDF; DESIGN.md "Aligning a frame to the map" has the definition to the bit).  frame->pose is the guess, camera -> world.  Pixel i
 * with depth z is VALID when z is finite and near <= z <= far; its point p = o + z d lies on chisel_hip_render_view's ray of that pixel;
 * ChunkManager::GetSDFAndGradient(p) (src/ChunkManager.cpp:449-474, called unchanged) gives the distance d0 at the centre c of p's
 * voxel and the normalised gradient g; the residual is rho = d0 + g . (p - c); the pixel is USED when it is valid, the lookup succeeds
 * and, with max_residual > 0, |rho| <= max_residual.  With J = (g, p x g) in double -- the left perturbation p' = p + v + w x p,
 * xi = (v, w) -- terms[32] holds over the used pixels:
 *   [0..20] the upper triangle of sum J J^T, row-major;  [21..26] sum J rho;  [27] sum rho^2;  [28] the number of used pixels;
 *   [29] the number of valid pixels;  [30], [31] 0
 * Every sum is taken in one fixed order (a pairwise tree over groups of 256 pixels in row-major order), without atomics: the 32 doubles
 * are the same bits on every run.  frame->on_device as in chisel_hip_integrate_depth; terms_on_device: terms is a device pointer,
 * written on the map's stream without a wait (behind the event of a chisel_hip_wait_event or chisel_hip_order_map_after_stream before
 * it, which says that a device image is ready); otherwise a host array, complete on return.  The map is only read.
 * CHISEL_HIP_ERR_UNSUPPORTED: a group or one shard of several (a point needs every owner's voxels).  Then CHISEL_HIP_ERR_INVALID for a
 * null argument or image, or a non-positive size. */
int chisel_hip_align_terms(chisel_hip_map *map, const chisel_hip_depth_frame *frame, float max_residual, double *terms /* 32 */, int terms_on_device);
/* The step of those normal equations, on the host in double (no device is needed): A = the symmetric matrix of terms[0..20] with
 * damping * terms[28] added to its diagonal (absolute Tikhonov damping per used pixel), Cholesky A = L L^T in which a pivot s is accepted
 * iff s > 1e-12 max_j A_jj, then A xi = -terms[21..26] by forward and back substitution.  xi = (v, w).  CHISEL_HIP_ERR_UNSUPPORTED when
 * a pivot is refused (the equations are degenerate; xi is left alone), CHISEL_HIP_ERR_INVALID for a null argument. */
int chisel_hip_align_solve(const double terms[32], double damping, double xi[6]);
typedef struct {
    int max_iterations;      /* >= 1                                                                     */
    int min_pixels;          /* fewer used pixels than this: CHISEL_HIP_ALIGN_TOO_FEW_PIXELS             */
    float max_residual;      /* [m]; <= 0: every valid pixel whose lookup succeeds is used               */
    float reserved;
    double damping;          /* chisel_hip_align_solve's                                                  */
    double min_translation;  /* [m] and ...                                                               */
    double min_rotation;     /* ... [rad]: an update smaller than both ends the loop                      */
} chisel_hip_align_params;  /* 40 bytes */
typedef struct {
    double pose[12];         /* the refined pose, camera -> world, row-major 3 x 4                        */
    double xi_last[6];       /* the last update applied (zeros when there was none)                       */
    double terms_first[32];  /* chisel_hip_align_terms at the guess ...                                   */
    double terms_last[32];   /* ... and as last evaluated (at the pose before the last update)            */
    int iterations;          /* updates applied                                                           */
    int status;              /* CHISEL_HIP_ALIGN_*                                                        */
} chisel_hip_align_result;  /* 664 bytes */
#define CHISEL_HIP_ALIGN_CONVERGED 0       /* the last update was smaller than min_translation and min_rotation */
#define CHISEL_HIP_ALIGN_ITERATION_LIMIT 1 /* max_iterations updates applied                                     */
#define CHISEL_HIP_ALIGN_TOO_FEW_PIXELS 2  /* terms[28] < min_pixels: the pose is as before that iteration       */
#define CHISEL_HIP_ALIGN_DEGENERATE 3      /* chisel_hip_align_solve refused a pivot: likewise                    */
/* Gauss-Newton on the pose of a depth frame against the map: up to max_iterations times chisel_hip_align_terms at the current pose
 * (kept in double, handed to the kernels rounded to float), chisel_hip_align_solve, and the update R <- R_d R, t <- R_d t + v with
 * R_d = I + (sin th / th) K + ((1 - cos th) / th^2) K^2, K the cross-product matrix of w, th = |w| (R_d = I + K where th <= 1e-12).
 * A host image is copied to the device once.  All four statuses are outcomes and return CHISEL_HIP_OK; the map is only read; complete on
 * return.  Error codes as chisel_hip_align_terms; also CHISEL_HIP_ERR_INVALID for null params or result or max_iterations < 1. */
int chisel_hip_align_depth(chisel_hip_map *map, const chisel_hip_depth_frame *frame, const chisel_hip_align_params *params,
                           chisel_hip_align_result *result);
/* Not in the reference: the map `src`, moved by the rigid transform src_to_dst (row-major 3 x 4, as every pose here), fused into `dst` --
 * what a pose-graph server needs when an inter-agent loop closure moves a whole agent's trajectory and the frames that built its map
 * are gone (ServerKeyFrame::FreeSpace); also a map dump brought into a live map at an offset, and the shards of a map collected into
 * one.  DESIGN.md "Merging maps" has the definition to the bit; in short, with M the inverse of src_to_dst taken as rigid (R^T, -R^T t,
 * formed in double, rounded to fp32): every voxel of `dst` whose centre c (ChunkManager.cpp:50-66) has an observed source voxel
 * ChunkManager::GetSDF(M c) (nearest voxel, weight > 1e-12) takes DistVoxel::Integrate(source distance, source weight) and, when both
 * maps hold colour and the source voxel's colour weight is > 0, ColorVoxel::Integrate(source colour, source colour weight).  Afterwards
 * `dst` holds a chunk iff it held it before or one of its voxels was updated (the rule of Chisel::IntegrateDepthScan, Chisel.h:59-213),
 * and every updated chunk is left as an integration leaves it: in meshesToUpdate with its 27-neighbourhood, counted in
 * CHISEL_HIP_CNT_SDF / _COL / _NEW_CHUNKS / _UPDATED_CHUNKS.  `src` is only read.
 * The work runs on dst's stream, behind everything queued on src's stream so far; what src is given next starts behind it: no
 * synchronisation by the caller before or after.  The host waits once, for the number of chunks `dst` may have to create.  stats may be
 * NULL; otherwise the call also waits for its own end and reports src_chunks = resident chunks of `src`, dst_chunks_created = chunks
 * `dst` did not hold before, dst_chunks_updated = chunks with at least one updated voxel (old or new), voxels_updated.
 * Refused with neither map touched: CHISEL_HIP_ERR_INVALID for a null argument, dst == src, maps on different devices, of different
 * chunk size or voxel resolution, an entry of src_to_dst that is not finite, a rotation part with max |R^T R - I| > 1e-4;
 * CHISEL_HIP_ERR_UNSUPPORTED for a group or one shard of several; CHISEL_HIP_ERR_POOL_FULL when a fixed pool (max_chunks > 0) cannot take
 * the chunks the merge may create -- decided before the first one is created (a growing pool grows). */
typedef struct {
    int64_t src_chunks, dst_chunks_created, dst_chunks_updated, voxels_updated;
} chisel_hip_merge_stats;   /* 32 bytes */
int chisel_hip_merge_map(chisel_hip_map *dst, chisel_hip_map *src, const float src_to_dst[12], chisel_hip_merge_stats *stats);
/* Not in the reference: one depth frame taken back out of the map -- what a pose-graph server needs when a loop closure moves a keyframe
 * whose depth map is already fused: take it out at the pose it went in with, integrate it again at the corrected one.  DESIGN.md "Taking
 * a frame out again" has the definition to the bit; in short: a voxel is selected when the frame's integration under the map's current
 * integrator settings (chisel_hip_set_integrator; the caller sees to it that they are the ones the frame went in with) sent it down the
 * in-band branch -- ProjectionIntegrator::Integrate (color_rules == 0: depth <= 50, update weight wu = 1) or IntegrateColor
 * (color_rules != 0: NaN depth skipped, depth <= 100, wu = weight / (5 truncation)) -- which depends on the frame and the geometry only.
 * With sd = depth - camera z, a selected voxel (s, w):
 *   !(w > 0)                          is left alone                                  (voxels_skipped)
 *   w2 = w - wu, !(w2 > w * 2^-16)    becomes DistVoxel::Reset(), (99999, 0)         (voxels_cleared: the frame was the voxel's only one, or
 *                                     what is left is a residue of rounding, negative -- the voxel was carved since -- or NaN)
 *   otherwise                         becomes ((w s - wu sd) / w2, w2)               (voxels_updated)
 * each product, sum and quotient rounded separately in fp32.  NOT undone: the carve branch (Carve() and the weight decay destroy what they
 * act on) and colour voxels, which this call never writes -- so integrating the same frame again restores the distance field up to
 * rounding, and only where nothing was carved in between.
 * No chunk is created or removed.  A chunk with an updated or cleared voxel (chunks_touched) is left as an integration leaves an updated
 * chunk, in meshesToUpdate with its 27-neighbourhood; of those, the chunks in which no voxel has a weight > 0 afterwards are counted in
 * chunks_emptied and the ids of the first max_ids of them, in any order, written to emptied_ids_xyz (3 ints each; NULL and 0 are allowed):
 * hand them to chisel_hip_garbage_collect to be rid of them.  chunks_tested: the resident chunks, each tested against the frame's image
 * pyramid.  The CHISEL_HIP_CNT_* counters are not touched: they count forward executions.
 * frame->on_device as in chisel_hip_integrate_depth.  The work is queued on the map's stream; with stats == NULL (and a device image) the
 * call waits for nothing, otherwise once, at its end.
 * Refused with nothing touched: CHISEL_HIP_ERR_INVALID for a null map, frame or depth image, a non-positive size or more than 2^31 - 1
 * pixels, a pose entry or an intrinsic that is not finite, max_ids < 0, emptied_ids_xyz without stats; CHISEL_HIP_ERR_UNSUPPORTED for a
 * group or one shard of several (ghost chunks would need a rule of their own). */
typedef struct {
    int64_t chunks_tested, chunks_touched, chunks_emptied, voxels_updated, voxels_cleared, voxels_skipped;
} chisel_hip_deintegrate_stats;   /* 48 bytes */
int chisel_hip_deintegrate_depth(chisel_hip_map *map, const chisel_hip_depth_frame *frame, int color_rules, chisel_hip_deintegrate_stats *stats,
                                 int *emptied_ids_xyz, int max_ids);
/* Many frames taken out in one call -- a loop closure moves a stretch of a trajectory, and most of its keyframes look at the same voxels.
 * The map is left, bit for bit, in the state that n calls of chisel_hip_deintegrate_depth on frames[0], ..., frames[n-1], in that order,
 * would leave it: the distance voxels (the frames apply to a voxel in call order; the rule depends on the voxel's state), meshesToUpdate
 * and the sign summaries; the CHISEL_HIP_CNT_* counters are not touched.  DESIGN.md "Many frames in one call" has the definition.  The
 * frames go in launch sets of up to 16, and a voxel under several frames of a set is read and written once.
 * stats: the sums of what the n single calls would report -- chunks_tested = n x the resident chunks, chunks_touched = the (chunk, frame)
 * pairs in which that frame updated or cleared a voxel, chunks_emptied = the chunks some frame of the call touched and in which no voxel
 * has a weight > 0 at the end (each counted once; the ids of the first max_ids of them, in any order, in emptied_ids_xyz).
 * The frames of one call may differ in image size, camera and memory space (on_device per frame); host images are staged, a launch set
 * at a time, and all of them have been copied when the call returns.  The work is queued on the map's stream; with stats == NULL and
 * device images only the call waits for nothing, otherwise once, at its end.  n == 0: CHISEL_HIP_OK, zero stats, nothing launched.
 * Refused with nothing touched, every frame being looked at first: CHISEL_HIP_ERR_INVALID for a null map, n < 0, null frames with n > 0,
 * max_ids < 0, emptied_ids_xyz without stats, and any frame chisel_hip_deintegrate_depth refuses (the message names its index);
 * CHISEL_HIP_ERR_UNSUPPORTED for a group or one shard of several. */
int chisel_hip_deintegrate_batch(chisel_hip_map *map, int n, const chisel_hip_depth_frame *frames, int color_rules, chisel_hip_deintegrate_stats *stats,
                                 int *emptied_ids_xyz, int max_ids);
/* ProjectionIntegrator::Integrate<DataType>(depthImage, camera, cameraPose, chunk) / IntegrateColor (ProjectionIntegrator.h:51-52,
 * :101-102): ONE frame into ONE resident chunk -- whether or not the frustum's id range holds it, as the reference's per-chunk call
 * knows nothing of frusta --; color may be NULL (the depth-only update rule).  *updated = the call's return value there ("some voxel
 * changed").  CHISEL_HIP_ERR_NOT_FOUND when the chunk is not resident. */
int chisel_hip_integrate_chunk(chisel_hip_map *map, const int id_xyz[3], const chisel_hip_depth_frame *frame, const chisel_hip_color_frame *color,
                               int *updated);
/* ChunkManager::ExtractInsideVoxelMesh / ExtractBorderVoxelMesh(chunk, index, coordinates, nextMeshIndex, mesh) (src/ChunkManager.cpp:
 * 259-379): the marching-cubes triangles of ONE cube of a resident chunk -- corner voxels index + cubeIndexOffsets, read from the
 * neighbouring chunk where a coordinate leaves [0, N) (index components -1 .. N-1), none when a corner is unobserved (weight <= 0.5) or
 * its chunk absent --, MarchingCubes::MeshCube with the caller's cube coordinates: up to 15 vertices (3 floats each) and their face
 * normals; *occupied: MarchingCubes::IsOccupied (the caller pushes a grid entry).  vertices / normals may be NULL. */
int chisel_hip_mesh_cube(chisel_hip_map *map, const int id_xyz[3], const int voxel_index[3], const float coordinates[3], float *vertices, float *normals,
                         int *n_vertices, int *occupied);
/* ChunkManager::RecomputeMesh(chunkID, mutex) (src/ChunkManager.cpp:91-128): the mesh of one chunk into ChunkManager::allMeshes, leaving
 * meshesToUpdate as it is (chisel_hip_update_meshes_of ends with the meshesToUpdate.clear() of Chisel::UpdateMeshes, Chisel.cpp:57) */
int chisel_hip_recompute_mesh(chisel_hip_map *map, const int id_xyz[3]);
/* ChunkManager::GenerateMesh(chunk, mesh) (src/ChunkManager.cpp:381-447) for one resident chunk into the caller's arrays -- marching
 * cubes with face normals; stages bit 0 adds ComputeNormalsFromGradients, bit 1 ColorizeMesh (stages 3 = what RecomputeMesh stores) --
 * without touching ChunkManager::allMeshes or meshesToUpdate.  Arrays of 3 floats per vertex / grid entry; n_vertices / n_grids are
 * always set, the arrays only when both capacities suffice (a 16^3 chunk has at most 15 * 4096 vertices and 4096 grid entries). */
int chisel_hip_generate_mesh(chisel_hip_map *map, const int id_xyz[3], int stages, int64_t capacity_vertices, int64_t capacity_grids,
                             float *vertices, float *normals, float *colors, float *grids, int64_t *n_vertices, int64_t *n_grids);
/* hipEvent pairs around every kernel launch on the map's stream (off by default) */
int chisel_hip_set_profiling(chisel_hip_map *map, int enable);
/* total milliseconds and launch counts per CHISEL_HIP_KERNEL_* since enabled / last reset */
int chisel_hip_get_profile(chisel_hip_map *map, double *ms_total, int64_t *launches, int reset_profile);
/* The public statics of marching_cubes/MarchingCubes.h:41-146 for a caller's own cube, on the device (no map involved; the current
 * HIP device):
 *   chisel_hip_mc_tables          triangleTable[256][16] (-1 terminated rows) and edgeIndexPairs[12][2] (MarchingCubes.cpp:29-302)
 *   chisel_hip_mesh_cube_values   vertex_coords: 3 x 8 column-major, vertex_sdf: 8 -> CalculateVertexConfiguration (:108-118),
 *                                 InterpolateEdgeVertices (:120-132; edge_coords 3 x 12 column-major, zeros where the reference leaves a
 *                                 column unset; may be null) and MeshCube(.., Mesh*) (:73-106): up to 15 vertices in push order
 *                                 (t + 2, t + 1, t) with each triangle's face normal thrice (vertices / normals: 45 floats each; may be null)
 *   chisel_hip_interpolate_vertex InterpolateVertex (:135-146), "vertex1 + 0.5 * vertex2" included
 * and geometry/Raycast.h:9 / Raycast.cpp:35-128: the cells of [min, max) the segment start -> end meets, in order (cells: capacity x 3
 * ints; *count = cells met, which may exceed capacity). */
int chisel_hip_mc_tables(int *triangle_table, int *edge_index_pairs);
int chisel_hip_mesh_cube_values(const float *vertex_coords, const float *vertex_sdf, float *edge_coords, int *configuration, float *vertices,
                                float *normals, int *n_vertices);
int chisel_hip_interpolate_vertex(const float v1[3], const float v2[3], float sdf1, float sdf2, float out[3]);
int chisel_hip_raycast(const float start[3], const float end[3], const int min_xyz[3], const int max_xyz[3], int *cells, int64_t capacity,
                       int64_t *count);
/* Which shapes the launch heuristics picked since the map was created / last reset of these figures (no reference counterpart: a
 * diagnostic beside chisel_hip_get_profile): out[0..7] = integration launches at 2 voxels per lane, at 4, at 4 with a 2-voxel tail;
 * cull launches with four waves per workgroup, with one wave per frame; launch sets without an order kernel; launch sets in the
 * short single-stream form; launch sets in all; out[8..9] = launch sets queued behind a mesh recompute whose totals the host had not seen
 * yet, and the ones of them that had to be replayed because that recompute did not fit.  A group handle sums its shards. */
#define CHISEL_HIP_NUM_LAUNCH_STATS 10
int chisel_hip_get_launch_stats(chisel_hip_map *map, int64_t *out, int reset_stats);
/* The chunk pool (no reference counterpart: ChunkManager's map has no capacity): out[0] = chunks with voxel memory behind them now,
 * out[1] = the most the pool can grow to (== out[0] for a fixed pool), out[2] = times it has grown, out[3] = 1 if it can grow.  A growing
 * pool commits more memory when its free slots fall under a quarter (checked when a launch set is queued, from the figures the integration
 * kernels report: nothing is waited for, nothing is moved, ids and slots stay what they are); a group handle reports its shards' sums. */
int chisel_hip_pool_info(chisel_hip_map *map, int64_t out[4]);
/* owner shard of a chunk id under (n_shards, shard_block); pure function, same on every rank */
int chisel_hip_chunk_owner(const int id_xyz[3], int n_shards, int shard_block);

#ifdef __cplusplus
}
#endif
#endif /* CHISEL_HIP_H_ */

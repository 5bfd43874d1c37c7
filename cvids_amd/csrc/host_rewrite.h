// host_rewrite.h -- what the entries that rewrite voxels outside the depth-integration path share, as the readers share query_refusal
// (host_render.h): chisel_hip_integrate_pointcloud, chisel_hip_merge_map, chisel_hip_deintegrate_depth.  Each keeps its own refusals.
namespace {

// in front of the first thing queued: a deferred launch set settled, the device, and a recompute in flight (it reads the voxels as they are) seen to
int rewrite_begin(chisel_hip_map *m) {
    SETTLE(m);
    HIP_TRY(hipSetDevice(m->device));
    return check_mesh_totals(m);
}

// behind the last kernel: slots were dirtied without their neighbourhoods listed (the next recompute runs mesh_mark_kernel), the hash may have changed
int rewrite_end(chisel_hip_map *m) {
    m->mesh_mark_needed = true;
    HIP_TRY(note_map_mutation(m));
    return CHISEL_HIP_OK;
}

}  // namespace

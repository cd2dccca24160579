"""ctypes view of include/gie.h.

`bind(lib, prefix)` attaches argtypes/restype for every entry point of the C-ABI to a loaded
shared library whose symbols start with `prefix`.  The product library uses prefix "gie_".
(The test-only CPU oracle exports the same signatures under another prefix and is bound by
tests/, never from this package.)
"""
import ctypes as C

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_i8p = C.POINTER(C.c_int8)
c_u8p = C.POINTER(C.c_uint8)


class Config(C.Structure):
    """gie_config (include/gie.h)."""
    _fields_ = [
        ("voxel_width", C.c_float),
        ("local_size", C.c_int32 * 3),
        ("occupancy_threshold", C.c_int32),
        ("ogm_min_h", C.c_float),
        ("ogm_max_h", C.c_float),
        ("cutoff_grids_sq", C.c_int32),
        ("fast_mode", C.c_int32),
        ("for_motion_planner", C.c_int32),
        ("robot_r2_grids", C.c_int32),
        ("max_blocks", C.c_int32),
        ("device_id", C.c_int32),
        ("retain_radius_blocks", C.c_int32),
        ("wave_workgroups", C.c_int32),
        ("place_tries", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class MultiScanParam(C.Structure):
    _fields_ = [("scan_num", C.c_int32), ("ring_num", C.c_int32), ("max_r", C.c_float),
                ("theta_inc", C.c_float), ("theta_min", C.c_float), ("phi_inc", C.c_float),
                ("phi_min", C.c_float)]


class CamParam(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("cx", C.c_float), ("cy", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("valid_nan", C.c_int32)]


class ScanParam(C.Structure):
    _fields_ = [("scan_num", C.c_int32), ("max_r", C.c_float), ("theta_inc", C.c_float),
                ("theta_min", C.c_float)]


class Voxel(C.Structure):
    _fields_ = [("occ_val", C.c_uint8), ("vox_type", C.c_int8), ("pad", C.c_int16),
                ("dist_sq", C.c_int32), ("coc", C.c_int32 * 3)]


class Nf1Param(C.Structure):
    _fields_ = [("clearance", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class FrontierParam(C.Structure):
    """gie_frontier_param (include/gie.h); clearance in voxel units."""
    _fields_ = [("clearance", C.c_float), ("min_size", C.c_int32), ("connectivity", C.c_int32), ("max_clusters", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class FrontierCluster(C.Structure):
    """gie_frontier_cluster (include/gie.h): 80 bytes, sum at offset 56."""
    _fields_ = [("label", C.c_int32), ("size", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("rep", C.c_int32 * 3),
                ("centroid", C.c_float * 3), ("sum", C.c_int64 * 3)]


class LosParam(C.Structure):
    """gie_los_param (include/gie.h); clearance in voxel units."""
    _fields_ = [("clearance", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class LosHit(C.Structure):
    """gie_los_hit (include/gie.h): 24 bytes."""
    _fields_ = [("first", C.c_int32), ("len", C.c_int32), ("hit", C.c_int32 * 3), ("min_edt", C.c_float)]


class View(C.Structure):
    """gie_view (include/gie.h): 64 bytes."""
    _fields_ = [("pos", C.c_float * 3), ("n_planes", C.c_int32), ("normal", (C.c_int32 * 3) * 4)]


class ViewParam(C.Structure):
    """gie_view_param (include/gie.h); ranges in metres."""
    _fields_ = [("r_min", C.c_float), ("r_max", C.c_float), ("tan2_elev", C.c_float), ("reserved", C.c_int32)]


class ViewScore(C.Structure):
    """gie_view_score (include/gie.h): 16 bytes."""
    _fields_ = [("unknown", C.c_int32), ("frontier", C.c_int32), ("occupied", C.c_int32), ("candidates", C.c_int32)]


class ShortcutParam(C.Structure):
    """gie_shortcut_param (include/gie.h): 16 bytes."""
    _fields_ = [("lookahead", C.c_int32), ("max_wp", C.c_int32), ("reserved", C.c_int32 * 2)]


class Waypoint(C.Structure):
    """gie_waypoint (include/gie.h): 24 bytes."""
    _fields_ = [("xyz", C.c_int32 * 3), ("index", C.c_int32), ("min_edt", C.c_float), ("forced", C.c_int32)]


class ShortcutInfo(C.Structure):
    """gie_shortcut_info (include/gie.h): 16 bytes."""
    _fields_ = [("count", C.c_int32), ("forced", C.c_int32), ("length", C.c_float), ("reserved", C.c_int32)]


class CloudParam(C.Structure):
    """gie_cloud_param (include/gie.h): 32 bytes."""
    _fields_ = [("type_mask", C.c_uint32), ("intensity", C.c_int32), ("z_lo", C.c_int32), ("z_hi", C.c_int32), ("max_points", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class CloudPoint(C.Structure):
    """gie_cloud_point (include/gie.h): 16 bytes."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("intensity", C.c_float)]


class BlocksParam(C.Structure):
    """gie_blocks_param (include/gie.h): 48 bytes."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("flags", C.c_int32), ("min_fnt", C.c_int32), ("max_records", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class BlockSummary(C.Structure):
    """gie_block_summary (include/gie.h): 32 bytes."""
    _fields_ = [("key", C.c_int32 * 3), ("n_free", C.c_uint16), ("n_occupied", C.c_uint16), ("n_fnt", C.c_uint16), ("fnt_voxel", C.c_uint16),
                ("free_voxel", C.c_uint16), ("flags", C.c_uint16), ("min_dist_sq", C.c_int32), ("reserved", C.c_int32)]


class RoutesParam(C.Structure):
    """gie_routes_param (include/gie.h): 48 bytes."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("min_free", C.c_int32), ("min_open", C.c_int32), ("min_fnt", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class RoutesInfo(C.Structure):
    """gie_routes_info (include/gie.h): 32 bytes."""
    _fields_ = [("n_nodes", C.c_int32), ("n_links", C.c_int32), ("n_frontier", C.c_int32), ("n_sources", C.c_int32), ("n_reached", C.c_int32),
                ("max_steps", C.c_int32), ("reserved", C.c_int32 * 2)]


class GroundParam(C.Structure):
    """gie_ground_param (include/gie.h): 32 bytes."""
    _fields_ = [("z_lo", C.c_int32), ("z_hi", C.c_int32), ("min_known", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class GroundCell(C.Structure):
    """gie_ground_cell (include/gie.h): 16 bytes."""
    _fields_ = [("dist_sq", C.c_int32), ("coc_x", C.c_int32), ("coc_y", C.c_int32), ("type", C.c_int8), ("inside", C.c_uint8), ("pad", C.c_uint8 * 2)]


class GroundNf1Param(C.Structure):
    """gie_ground_nf1_param (include/gie.h): 32 bytes."""
    _fields_ = [("clearance_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 6)]


class GroundLosParam(C.Structure):
    """gie_ground_los_param (include/gie.h): 16 bytes."""
    _fields_ = [("clearance_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class GroundHit(C.Structure):
    """gie_ground_hit (include/gie.h): 24 bytes."""
    _fields_ = [("first", C.c_int32), ("len", C.c_int32), ("hit", C.c_int32 * 2), ("min_dist_sq", C.c_int32), ("reserved", C.c_int32)]


class GroundShortcutParam(C.Structure):
    """gie_ground_shortcut_param (include/gie.h): 32 bytes."""
    _fields_ = [("lookahead", C.c_int32), ("max_wp", C.c_int32), ("clearance_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class GroundWaypoint(C.Structure):
    """gie_ground_waypoint (include/gie.h): 24 bytes."""
    _fields_ = [("xy", C.c_int32 * 2), ("index", C.c_int32), ("min_dist_sq", C.c_int32), ("forced", C.c_int32), ("reserved", C.c_int32)]


class GroundViewParam(C.Structure):
    """gie_ground_view_param (include/gie.h): 32 bytes; ranges in metres."""
    _fields_ = [("r_min", C.c_float), ("r_max", C.c_float), ("n_planes", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class GroundRolloutParam(C.Structure):
    """gie_ground_rollout_param (include/gie.h): 32 bytes; clearance_sq and inflate_sq in squared cells."""
    _fields_ = [("clearance_sq", C.c_int32), ("inflate_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 5)]


class GroundRollout(C.Structure):
    """gie_ground_rollout (include/gie.h): 48 bytes, one per trajectory."""
    _fields_ = [("end", C.c_int32), ("poses", C.c_int32), ("hit", C.c_int32 * 2), ("cells", C.c_int32), ("min_dist_sq", C.c_int32), ("cost", C.c_int64),
                ("nf1_end", C.c_int32), ("nf1_min", C.c_int32), ("nf1_min_at", C.c_int32), ("reserved", C.c_int32)]


class GroundFootprintParam(C.Structure):
    """gie_ground_footprint_param (include/gie.h): 32 bytes; the three extents and clearance_sq in squared cells."""
    _fields_ = [("front_sq", C.c_int32), ("back_sq", C.c_int32), ("side_sq", C.c_int32), ("clearance_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class GroundFootprint(C.Structure):
    """gie_ground_footprint (include/gie.h): 32 bytes, one per trajectory."""
    _fields_ = [("end", C.c_int32), ("poses", C.c_int32), ("hit", C.c_int32 * 2), ("hit_cells", C.c_int32), ("min_dist_sq", C.c_int32), ("min_at", C.c_int32),
                ("reserved", C.c_int32)]


class GroundPoseNf1Param(C.Structure):
    """gie_ground_pose_nf1_param (include/gie.h): 32 bytes; the three extents and clearance_sq in squared cells."""
    _fields_ = [("front_sq", C.c_int32), ("back_sq", C.c_int32), ("side_sq", C.c_int32), ("clearance_sq", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class GroundSdfRolloutParam(C.Structure):
    """gie_ground_sdf_rollout_param (include/gie.h): 32 bytes; margin in metres."""
    _fields_ = [("margin", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 6)]


class GroundSdfRollout(C.Structure):
    """gie_ground_sdf_rollout (include/gie.h): 32 bytes, one per trajectory."""
    _fields_ = [("points", C.c_int32), ("argmin", C.c_int32), ("min_dist", C.c_float), ("grad", C.c_float * 2), ("first_below", C.c_int32),
                ("n_below", C.c_int32), ("first_in", C.c_int32)]


class GroundFrontierParam(C.Structure):
    """gie_ground_frontier_param (include/gie.h): 32 bytes; clearance_sq in squared cells."""
    _fields_ = [("clearance_sq", C.c_int32), ("min_size", C.c_int32), ("connectivity", C.c_int32), ("max_clusters", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class GroundFrontierCluster(C.Structure):
    """gie_ground_frontier_cluster (include/gie.h): 64 bytes, sum at offset 40."""
    _fields_ = [("label", C.c_int32), ("size", C.c_int32), ("lo", C.c_int32 * 2), ("hi", C.c_int32 * 2), ("rep", C.c_int32 * 2),
                ("centroid", C.c_float * 2), ("sum", C.c_int64 * 2), ("rep_dist_sq", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(GroundFrontierParam) == 32 and C.sizeof(GroundFrontierCluster) == 64 and GroundFrontierCluster.sum.offset == 40
assert C.sizeof(GroundSdfRolloutParam) == 32 and C.sizeof(GroundSdfRollout) == 32 and GroundSdfRollout.first_below.offset == 20
assert C.sizeof(GroundPoseNf1Param) == 32 and GroundPoseNf1Param.flags.offset == 16
assert C.sizeof(GroundFootprintParam) == 32 and C.sizeof(GroundFootprint) == 32 and GroundFootprintParam.flags.offset == 16 and GroundFootprint.hit_cells.offset == 16
assert C.sizeof(GroundRolloutParam) == 32 and C.sizeof(GroundRollout) == 48 and GroundRollout.cost.offset == 24 and GroundRollout.nf1_end.offset == 32
assert C.sizeof(GroundViewParam) == 32 and GroundViewParam.n_planes.offset == 8 and GroundViewParam.reserved.offset == 16
assert C.sizeof(GroundLosParam) == 16 and C.sizeof(GroundHit) == 24 and C.sizeof(GroundShortcutParam) == 32 and C.sizeof(GroundWaypoint) == 24
assert C.sizeof(GroundParam) == 32 and C.sizeof(GroundCell) == 16 and C.sizeof(GroundNf1Param) == 32
assert C.sizeof(CloudParam) == 32 and C.sizeof(CloudPoint) == 16
assert C.sizeof(BlocksParam) == 48 and C.sizeof(BlockSummary) == 32 and BlockSummary.min_dist_sq.offset == 24
assert C.sizeof(ShortcutParam) == 16 and C.sizeof(Waypoint) == 24 and C.sizeof(ShortcutInfo) == 16
assert C.sizeof(LosHit) == 24 and C.sizeof(View) == 64 and C.sizeof(ViewScore) == 16 and C.sizeof(LosParam) == 16 and C.sizeof(ViewParam) == 16

NF1_UNKNOWN_TRAVERSABLE = 1
NF1_FROM_FRONTIERS = 2
LOS_UNKNOWN_OPAQUE = 1
CLOUD_TYPE = 0
CLOUD_DIST = 1
BLOCKS_DIST = 1
ROUTES_FROM_FRONTIERS = 1
GROUND_UNKNOWN_BLOCKS = 1
GROUND_NF1_UNKNOWN_TRAVERSABLE = 1
GROUND_NF1_FROM_FRONTIERS = 2
GROUND_LOS_UNKNOWN_TRAVERSABLE = 1
GROUND_VIEW_UNKNOWN_OPAQUE = 1
GROUND_VIEW_UNION = 2
GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE = 1
GROUND_ROLLOUT_NF1 = 2
GROUND_ROLLOUT_MAX_POSES = 4096
GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE = 1
GROUND_FOOTPRINT_MARGIN = 2
GROUND_FOOTPRINT_MAX_SQ = 1 << 16
GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE = 1
GROUND_POSE_NF1_FROM_FRONTIERS = 2
GROUND_POSE_NF1_REVERSE = 4
GROUND_POSE_HEADINGS = 8
GROUND_POSE_MAX_SQ = 1 << 12
VOX_UNKNOWN, VOX_FREE, VOX_OCCUPIED, VOX_FNT = 0, 1, 2, 3


class CostMapHdr(C.Structure):
    _fields_ = [("x_size", C.c_int32), ("y_size", C.c_int32), ("z_size", C.c_int32),
                ("x_origin", C.c_float), ("y_origin", C.c_float), ("z_origin", C.c_float),
                ("width", C.c_float), ("type", C.c_uint8), ("pad", C.c_uint8 * 3)]


class FrameStats(C.Structure):
    _fields_ = [("frame", C.c_int32), ("blocks_total", C.c_int32), ("blocks_new", C.c_int32),
                ("seeds_a", C.c_int32), ("seeds_b", C.c_int32), ("seeds_c", C.c_int32),
                ("front_b", C.c_int32), ("front_c", C.c_int32),
                ("visits_a", C.c_int32), ("visits_b", C.c_int32), ("visits_c", C.c_int32),
                ("levels_a", C.c_int32), ("levels_b", C.c_int32), ("levels_c", C.c_int32),
                ("us_ogm", C.c_float), ("us_fuse", C.c_float), ("us_edt", C.c_float),
                ("us_merge", C.c_float),
                ("total_visits_a", C.c_int64), ("total_visits_b", C.c_int64), ("total_visits_c", C.c_int64),
                ("known_tiles", C.c_int32), ("frontier_tiles", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# name -> (restype, argtypes); handle is a void*
_H = C.c_void_p
SIGNATURES = {
    "create": (_H, [C.POINTER(Config)]),
    "destroy": (None, [_H]),
    "set_pose": (C.c_int, [_H, c_f32p, c_f32p]),
    "ogm_pointcloud": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "ogm_multiscan": (C.c_int, [_H, C.c_void_p, C.POINTER(MultiScanParam)]),
    "ogm_depth": (C.c_int, [_H, C.c_void_p, C.POINTER(CamParam)]),
    "ogm_scan2d": (C.c_int, [_H, C.c_void_p, C.POINTER(ScanParam)]),
    "ogm_labels": (C.c_int, [_H, C.c_void_p]),
    "set_ext_boxes": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fuse": (C.c_int, [_H]),
    "batch_edt": (C.c_int, [_H]),
    "merge": (C.c_int, [_H]),
    "merge_begin_tiled": (C.c_int, [_H]),
    "merge_end": (C.c_int, [_H]),
    "step": (C.c_int, [_H]),
    "read_local": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_ogm": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_batch_edt": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_costmap": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "query_global": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "get_stats": (C.c_int, [_H, C.POINTER(FrameStats)]),
    "get_pivot": (C.c_int, [_H, c_i32p]),
    "set_tile": (C.c_int, [_H, c_i32p, c_i32p]),
    "halo_count": (C.c_int, [_H, C.c_int]),
    "halo_export": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "halo_import": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "refine": (C.c_int, [_H, c_i32p]),
    "stream_enable": (C.c_int, [_H, C.c_int]),
    "stream_changed": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, c_i32p]),
}
class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("total_ms", C.c_float), ("launches", C.c_int32)]


# exchange rounds gated on the device: the device library and the test-only emulation of its logic (not the oracle, which has no device)
ROUND_API = {
    "read_costmap_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "costmap_publish": (C.c_int, [_H, C.POINTER(CostMapHdr)]),
    "costmap_acquire": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "query_global_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "round_gate": (C.c_int, [_H, C.c_void_p]),
    "refine_dev": (C.c_int, [_H, C.c_void_p]),
    "round_end": (C.c_int, [_H, C.c_void_p]),
    "round_stats": (C.c_int, [_H, C.POINTER(C.c_int64)]),
    "halo_export_all_dev": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "halo_import_all_dev": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
}

# entry points only the device library has
DEVICE_ONLY = {
    "profile_enable": (C.c_int, [_H, C.c_int]),
    "profile_read": (C.c_int, [_H, C.POINTER(KernelTime), C.c_int]),
    "last_error": (C.c_char_p, []),
    "sync": (C.c_int, [_H]),
    "get_stream": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "ogm_pointcloud_dev": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "halo_export_dev": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "halo_import_dev": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "halo_export_sparse": (C.c_int, [_H, C.c_int, C.c_void_p, c_i32p]),
    "halo_import_sparse": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int32]),
    "halo_export_sparse_dev": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "halo_import_sparse_dev": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "ogm_multiscan_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(MultiScanParam)]),
    "ogm_depth_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(CamParam)]),
    "ogm_labels_dev": (C.c_int, [_H, C.c_void_p]),
    "ogm_labels_dev_borrow": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int)]),
    # signed distance field of the local volume (include/gie.h): not in SIGNATURES, the oracle and the emulation do not have it
    "read_sdf": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_sdf_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "query_sdf": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "query_sdf_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # NF1 navigation function of the local volume (include/gie.h): device library only, like the signed distance field
    "nf1_compute": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(Nf1Param), C.c_void_p]),
    "nf1_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(Nf1Param), C.c_void_p]),
    "read_nf1": (C.c_int, [_H, C.c_void_p]),
    "read_nf1_dev": (C.c_int, [_H, C.c_void_p]),
    "nf1_path": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nf1_path_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "read_costmap_nf1": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "read_costmap_nf1_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    # frontier clusters of the local volume (include/gie.h): device library only
    "frontier_compute": (C.c_int, [_H, C.POINTER(FrontierParam), C.c_void_p, C.c_void_p]),
    "frontier_compute_dev": (C.c_int, [_H, C.POINTER(FrontierParam), C.c_void_p]),
    "read_frontier_clusters": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_frontier_clusters_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_frontier_labels": (C.c_int, [_H, C.c_void_p]),
    "read_frontier_labels_dev": (C.c_int, [_H, C.c_void_p]),
    # line of sight over the local volume (include/gie.h): device library only
    "los_prepare": (C.c_int, [_H, C.POINTER(LosParam), C.c_void_p]),
    "los_prepare_dev": (C.c_int, [_H, C.POINTER(LosParam), C.c_void_p]),
    "read_los_opaque": (C.c_int, [_H, C.c_void_p]),
    "read_los_opaque_dev": (C.c_int, [_H, C.c_void_p]),
    "los_segments": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "los_segments_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "view_gain": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(ViewParam), C.c_void_p]),
    "view_gain_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(ViewParam), C.c_void_p]),
    # path shortcutting over the opaque plane (include/gie.h): device library only
    "path_shortcut": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ShortcutParam), C.c_void_p, C.c_void_p]),
    "path_shortcut_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ShortcutParam), C.c_void_p, C.c_void_p]),
    # display clouds out of the local planes and the block pool (include/gie.h): device library only
    "cloud_local": (C.c_int, [_H, C.POINTER(CloudParam), C.c_void_p, C.c_void_p]),
    "cloud_local_dev": (C.c_int, [_H, C.POINTER(CloudParam), C.c_void_p, C.c_void_p]),
    "cloud_global": (C.c_int, [_H, C.POINTER(CloudParam), C.c_void_p, C.c_void_p]),
    "cloud_global_dev": (C.c_int, [_H, C.POINTER(CloudParam), C.c_void_p, C.c_void_p]),
    # global block summaries: counts, frontier blocks and a coarse grid out of the block pool (include/gie.h): device library only
    "blocks_summary": (C.c_int, [_H, C.POINTER(BlocksParam), C.c_void_p, C.c_void_p, C.c_void_p]),
    "blocks_summary_dev": (C.c_int, [_H, C.POINTER(BlocksParam), C.c_void_p, C.c_void_p, C.c_void_p]),
    # global block routes: face links between blocks and a BFS field on the block grid (include/gie.h): device library only
    "routes_compute": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(RoutesParam), C.c_void_p]),
    "routes_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(RoutesParam), C.c_void_p]),
    "read_routes": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_routes_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "routes_query": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "routes_query_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "routes_path": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "routes_path_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # ground costmap of a height band of the local volume (include/gie.h): device library only
    "ground_compute": (C.c_int, [_H, C.POINTER(GroundParam), C.c_void_p]),
    "ground_compute_dev": (C.c_int, [_H, C.POINTER(GroundParam), C.c_void_p]),
    "read_ground": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_ground_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_costmap_ground": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "read_costmap_ground_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "ground_query": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "ground_query_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    # NF1 navigation function of the ground costmap and its paths (include/gie.h): device library only
    "ground_nf1_compute": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(GroundNf1Param), C.c_void_p]),
    "ground_nf1_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(GroundNf1Param), C.c_void_p]),
    "read_ground_nf1": (C.c_int, [_H, C.c_void_p]),
    "read_ground_nf1_dev": (C.c_int, [_H, C.c_void_p]),
    "ground_nf1_path": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ground_nf1_path_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "read_costmap_ground_nf1": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    "read_costmap_ground_nf1_dev": (C.c_int, [_H, C.c_void_p, C.POINTER(CostMapHdr)]),
    # ground line of sight: segment checks and any-angle paths on the ground costmap (include/gie.h): device library only
    "ground_segments": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundLosParam), C.c_void_p]),
    "ground_segments_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundLosParam), C.c_void_p]),
    "ground_shortcut": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundShortcutParam), C.c_void_p, C.c_void_p]),
    "ground_shortcut_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundShortcutParam), C.c_void_p, C.c_void_p]),
    # ground frontier clusters and the gather of the ground navigation function (include/gie.h): device library only
    "ground_frontier_compute": (C.c_int, [_H, C.POINTER(GroundFrontierParam), C.c_void_p, C.c_void_p]),
    "ground_frontier_compute_dev": (C.c_int, [_H, C.POINTER(GroundFrontierParam), C.c_void_p]),
    "read_ground_frontier_clusters": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_ground_frontier_clusters_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "read_ground_frontier_labels": (C.c_int, [_H, C.c_void_p]),
    "read_ground_frontier_labels_dev": (C.c_int, [_H, C.c_void_p]),
    "ground_nf1_query": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "ground_nf1_query_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    # ground cost matrix: route lengths among points on the ground costmap (include/gie.h): device library only
    "ground_costmat_compute": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(GroundNf1Param), C.c_void_p, C.c_void_p]),
    "ground_costmat_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(GroundNf1Param), C.c_void_p, C.c_void_p]),
    # ground view gain: visible cells per candidate pose on the ground costmap (include/gie.h): device library only
    "ground_view_gain": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundViewParam), C.c_void_p]),
    "ground_view_gain_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundViewParam), C.c_void_p]),
    "ground_view_mask": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(GroundViewParam), C.c_void_p, C.c_void_p]),
    "ground_view_mask_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(GroundViewParam), C.c_void_p, C.c_void_p]),
    # ground rollouts: batched trajectory scoring on the ground costmap (include/gie.h): device library only
    "ground_rollouts": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundRolloutParam), C.c_void_p]),
    "ground_rollouts_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundRolloutParam), C.c_void_p]),
    # ground footprints: oriented-rectangle pose checks on the ground costmap (include/gie.h): device library only
    "ground_footprints": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundFootprintParam), C.c_void_p]),
    "ground_footprints_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundFootprintParam), C.c_void_p]),
    "ground_footprint_mask": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(GroundFootprintParam), C.c_void_p, C.c_void_p]),
    "ground_footprint_mask_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(GroundFootprintParam), C.c_void_p, C.c_void_p]),
    # ground pose navigation function: NF1 over (cell, heading) states of an oriented rectangle (include/gie.h): device library only
    "ground_pose_nf1_compute": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundPoseNf1Param), C.c_void_p]),
    "ground_pose_nf1_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GroundPoseNf1Param), C.c_void_p]),
    "read_ground_pose_nf1": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_ground_pose_nf1_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ground_pose_nf1_query": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ground_pose_nf1_query_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ground_pose_nf1_path": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ground_pose_nf1_path_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # ground signed distance: inside distances, bilinear queries, path clearance (include/gie.h): device library only
    "read_ground_sdf": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "read_ground_sdf_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ground_query_sdf": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ground_query_sdf_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ground_sdf_rollouts": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundSdfRolloutParam), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ground_sdf_rollouts_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(GroundSdfRolloutParam), C.c_void_p, C.c_void_p, C.c_void_p]),
    # goal-to-goal cost matrix of the local volume (include/gie.h): device library only
    "costmat_compute": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(Nf1Param), C.c_void_p, C.c_void_p]),
    "costmat_compute_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(Nf1Param), C.c_void_p, C.c_void_p]),
}
DEVICE_ONLY.update(ROUND_API)


def bind(lib, prefix, extra=None):
    """Return {short_name: ctypes function} for every symbol `prefix+name`."""
    out = {}
    table = dict(SIGNATURES)
    if extra:
        table.update(extra)
    for name, (res, args) in table.items():
        fn = getattr(lib, prefix + name)
        fn.restype = res
        fn.argtypes = args
        out[name] = fn
    return out

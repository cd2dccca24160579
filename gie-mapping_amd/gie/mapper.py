"""Host-side mirror of the reference's per-frame interface, over the C-ABI (include/gie.h).

`Mapper` plays the role of the objects VOLMAPNODE owns (LocMap + the four *MapMaker adapters +
GlbHashMap + the EDT launcher; src/volumetric_mapper.cpp:73-83) and `update()` reproduces the
call order of VOLMAPNODE::publishMap (src/volumetric_mapper.cpp:138-224).  It loads
libgie_hip.so and fails loudly when it is missing — there is no CPU fallback in this package.
"""
import ctypes as C
import math
import os
import sys

import numpy as np

from . import _capi
from ._capi import BLOCKS_DIST, CLOUD_DIST, CLOUD_TYPE, GROUND_POSE_HEADINGS, GROUND_POSE_MAX_SQ, GROUND_POSE_NF1_FROM_FRONTIERS, GROUND_POSE_NF1_REVERSE, GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE, GROUND_FOOTPRINT_MARGIN, GROUND_FOOTPRINT_MAX_SQ, GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE, GROUND_LOS_UNKNOWN_TRAVERSABLE, GROUND_NF1_FROM_FRONTIERS, GROUND_NF1_UNKNOWN_TRAVERSABLE, GROUND_ROLLOUT_MAX_POSES, GROUND_ROLLOUT_NF1, GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE, GROUND_UNKNOWN_BLOCKS, GROUND_VIEW_UNION, GROUND_VIEW_UNKNOWN_OPAQUE, LOS_UNKNOWN_OPAQUE, NF1_FROM_FRONTIERS, NF1_UNKNOWN_TRAVERSABLE, ROUTES_FROM_FRONTIERS, VOX_FNT, VOX_FREE, VOX_OCCUPIED, VOX_UNKNOWN
from ._capi import BlocksParam, CamParam, CloudParam, Config, CostMapHdr, FrameStats, FrontierParam, GroundFootprintParam, GroundFrontierParam, GroundLosParam, GroundNf1Param, GroundParam, GroundPoseNf1Param, GroundRolloutParam, GroundSdfRolloutParam, GroundShortcutParam, GroundViewParam, LosParam, MultiScanParam, Nf1Param, RoutesInfo, RoutesParam, ScanParam, ShortcutParam, ViewParam, Voxel

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "csrc", "libgie_hip.so")

SEENDIST_DTYPE = np.dtype([("d", "<f4"), ("s", "u1"), ("o", "u1"), ("pad", "u1", (2,))])
HALO_DTYPE = np.dtype([("dist_sq", "<i4"), ("coc", "<i4", (3,)), ("vox_type", "i1"), ("occ_val", "u1"), ("pad", "i1", (2,))])
HALO_ENTRY_DTYPE = np.dtype([("index", "<i4"), ("v", HALO_DTYPE)])          # gie_halo_entry: a known voxel of a sparse face layer
# gie_frontier_cluster: 80 bytes, the offsets of the C struct
FRONTIER_CLUSTER_DTYPE = np.dtype([("label", "<i4"), ("size", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("rep", "<i4", (3,)),
                                   ("centroid", "<f4", (3,)), ("sum", "<i8", (3,))])
# gie_los_hit (24 bytes), gie_view (64 bytes), gie_view_score (16 bytes)
LOS_HIT_DTYPE = np.dtype([("first", "<i4"), ("len", "<i4"), ("hit", "<i4", (3,)), ("min_edt", "<f4")])
VIEW_DTYPE = np.dtype([("pos", "<f4", (3,)), ("n_planes", "<i4"), ("normal", "<i4", (4, 3))])
VIEW_SCORE_DTYPE = np.dtype([("unknown", "<i4"), ("frontier", "<i4"), ("occupied", "<i4"), ("candidates", "<i4")])
# gie_waypoint (24 bytes), gie_shortcut_info (16 bytes)
WAYPOINT_DTYPE = np.dtype([("xyz", "<i4", (3,)), ("index", "<i4"), ("min_edt", "<f4"), ("forced", "<i4")])
SHORTCUT_INFO_DTYPE = np.dtype([("count", "<i4"), ("forced", "<i4"), ("length", "<f4"), ("reserved", "<i4")])
# gie_cloud_point (16 bytes)
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
CLOUD_NO_BAND = (-2 ** 31, 2 ** 31 - 1)
# gie_block_summary (32 bytes)
BLOCK_SUMMARY_DTYPE = np.dtype([("key", "<i4", (3,)), ("n_free", "<u2"), ("n_occupied", "<u2"), ("n_fnt", "<u2"), ("fnt_voxel", "<u2"), ("free_voxel", "<u2"),
                                ("flags", "<u2"), ("min_dist_sq", "<i4"), ("reserved", "<i4")])
# gie_routes_param (48 bytes), gie_routes_info (32 bytes)
ROUTES_PARAM = np.dtype([("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("min_free", "<i4"), ("min_open", "<i4"), ("min_fnt", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (2,))])
ROUTES_INFO = np.dtype([("n_nodes", "<i4"), ("n_links", "<i4"), ("n_frontier", "<i4"), ("n_sources", "<i4"), ("n_reached", "<i4"), ("max_steps", "<i4"),
                        ("reserved", "<i4", (2,))])
# gie_ground_cell (16 bytes)
GROUND_CELL_DTYPE = np.dtype([("dist_sq", "<i4"), ("coc", "<i4", (2,)), ("type", "i1"), ("inside", "u1"), ("pad", "u1", (2,))])
GROUND_HIT_DTYPE = np.dtype([("first", "<i4"), ("len", "<i4"), ("hit", "<i4", (2,)), ("min_dist_sq", "<i4"), ("reserved", "<i4")])
GROUND_WAYPOINT_DTYPE = np.dtype([("xy", "<i4", (2,)), ("index", "<i4"), ("min_dist_sq", "<i4"), ("forced", "<i4"), ("reserved", "<i4")])
# gie_ground_rollout (48 bytes)
GROUND_ROLLOUT_DTYPE = np.dtype([("end", "<i4"), ("poses", "<i4"), ("hit", "<i4", (2,)), ("cells", "<i4"), ("min_dist_sq", "<i4"), ("cost", "<i8"),
                                 ("nf1_end", "<i4"), ("nf1_min", "<i4"), ("nf1_min_at", "<i4"), ("reserved", "<i4")])
# gie_ground_sdf_rollout (32 bytes)
GROUND_SDF_ROLLOUT_DTYPE = np.dtype([("points", "<i4"), ("argmin", "<i4"), ("min_dist", "<f4"), ("grad", "<f4", (2,)), ("first_below", "<i4"), ("n_below", "<i4"),
                                     ("first_in", "<i4")])
# gie_ground_footprint (32 bytes)
GROUND_FOOTPRINT_DTYPE = np.dtype([("end", "<i4"), ("poses", "<i4"), ("hit", "<i4", (2,)), ("hit_cells", "<i4"), ("min_dist_sq", "<i4"), ("min_at", "<i4"), ("reserved", "<i4")])
# gie_ground_frontier_cluster: 64 bytes, the offsets of the C struct
GROUND_FRONTIER_CLUSTER_DTYPE = np.dtype([("label", "<i4"), ("size", "<i4"), ("lo", "<i4", (2,)), ("hi", "<i4", (2,)), ("rep", "<i4", (2,)),
                                          ("centroid", "<f4", (2,)), ("sum", "<i8", (2,)), ("rep_dist_sq", "<i4"), ("reserved", "<i4")])
VOXEL_DTYPE = np.dtype([("occ_val", "u1"), ("vox_type", "i1"), ("pad", "<i2"), ("dist_sq", "<i4"),
                        ("coc", "<i4", (3,))])


def flt2grids_sq(rad, voxel_width):
    """Parameters::flt2GridsSq (include/parameters.h:134-138)."""
    g = int(math.ceil(np.float32(rad) / np.float32(voxel_width)))
    return g * g


def make_config(voxel_width, local_size, occupancy_threshold=180, ogm_min_h=-1000.0, ogm_max_h=1000.0,
                cutoff_dist=None, cutoff_grids_sq=None, fast_mode=False, for_motion_planner=False,
                robot_r=0.4, max_blocks=0, device_id=0, retain_radius_blocks=0, wave_workgroups=0, place_tries=0):
    cfg = Config()
    cfg.voxel_width = voxel_width
    cfg.local_size[:] = [int(v) for v in local_size]
    cfg.occupancy_threshold = occupancy_threshold
    cfg.ogm_min_h = ogm_min_h
    cfg.ogm_max_h = ogm_max_h
    if cutoff_grids_sq is None:
        cutoff_grids_sq = flt2grids_sq(6.0 if cutoff_dist is None else cutoff_dist, voxel_width)
    cfg.cutoff_grids_sq = int(cutoff_grids_sq)
    cfg.fast_mode = int(bool(fast_mode))
    cfg.for_motion_planner = int(bool(for_motion_planner))
    cfg.robot_r2_grids = flt2grids_sq(robot_r, voxel_width)
    cfg.max_blocks = int(max_blocks)
    cfg.device_id = int(device_id)
    cfg.retain_radius_blocks = int(retain_radius_blocks)
    cfg.wave_workgroups = int(wave_workgroups)
    cfg.place_tries = int(place_tries)
    return cfg


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def view_frustum(yaw, pitch, hfov, vfov):
    """The four inward normals (int32 [4, 3]) of a camera frustum for gie_view.normal: the camera looks along +x turned by `yaw`
    about z and tilted up by `pitch` (radians), with full opening angles hfov and vfov (each below pi).  Every normal is the unit
    normal times 16384, rounded to integers: a quantisation of the angles to about 1e-4 rad — the planes that are tested are exactly
    these integer ones (include/gie.h), the angles they stand for differ from the arguments by that much."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    fwd = np.array([cp * cy, cp * sy, sp])
    left = np.array([-sy, cy, 0.0])
    up = np.array([-sp * cy, -sp * sy, cp])
    ch, sh, cv, sv = math.cos(hfov / 2), math.sin(hfov / 2), math.cos(vfov / 2), math.sin(vfov / 2)
    n = [sh * fwd + ch * left, sh * fwd - ch * left, sv * fwd + cv * up, sv * fwd - cv * up]
    return np.array([np.rint(16384.0 * v) for v in n]).astype(np.int32)


def make_views(pos, normals=None):
    """gie_view records (VIEW_DTYPE [n]) from positions (n x 3 metres) and, for all of them, one set of 0..4 normals (k x 3 integers)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    v = np.zeros(len(pos), VIEW_DTYPE)
    v["pos"] = pos
    if normals is not None:
        nm = np.asarray(normals, dtype=np.int32).reshape(-1, 3)
        v["n_planes"] = len(nm)
        v["normal"][:, :min(len(nm), 4)] = nm[:4]
    return v


class MapperBase:
    """Everything that only needs a bound function table (see _capi.bind)."""

    def __init__(self, fns, cfg):
        self._f = fns
        self.cfg = cfg
        self.size = tuple(int(v) for v in cfg.local_size)
        self.n = self.size[0] * self.size[1] * self.size[2]
        self._h = fns["create"](C.byref(cfg))
        if not self._h:
            raise RuntimeError("gie_create failed: " + self._err())

    def _err(self):
        f = self._f.get("last_error")
        return f().decode() if f else "error"

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("gie call failed (%d): %s" % (rc, self._err()))

    def close(self):
        if self._h:
            self._f["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- frame input -----------------------------------------------------------------
    def set_pose(self, pos, quat_wxyz=(1.0, 0.0, 0.0, 0.0)):
        p = (C.c_float * 3)(*[float(v) for v in pos])
        q = (C.c_float * 4)(*[float(v) for v in quat_wxyz])
        self._chk(self._f["set_pose"](self._h, p, q))

    def ogm_pointcloud(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._chk(self._f["ogm_pointcloud"](self._h, _ptr(xyz), xyz.shape[0]))

    def ogm_multiscan(self, ranges, theta_inc, theta_min, phi_inc, phi_min, max_r=100.0):
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        p = MultiScanParam(ranges.shape[1], ranges.shape[0], max_r, theta_inc, theta_min, phi_inc, phi_min)
        self._chk(self._f["ogm_multiscan"](self._h, _ptr(ranges), C.byref(p)))

    def ogm_depth(self, depth, cx, cy, fx, fy, valid_nan=False):
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        p = CamParam(depth.shape[0], depth.shape[1], cx, cy, fx, fy, int(valid_nan))
        self._chk(self._f["ogm_depth"](self._h, _ptr(depth), C.byref(p)))

    def ogm_scan2d(self, ranges, theta_inc, theta_min, max_r=30.0):
        ranges = np.ascontiguousarray(ranges, dtype=np.float32).reshape(-1)
        p = ScanParam(ranges.shape[0], max_r, theta_inc, theta_min)
        self._chk(self._f["ogm_scan2d"](self._h, _ptr(ranges), C.byref(p)))

    def ogm_labels(self, labels):
        """A pre-classified scan: int8 [Z][Y][X], 0 unknown / 1 free / 2 occupied."""
        labels = np.ascontiguousarray(labels, dtype=np.int8)
        assert labels.size == self.n
        self._chk(self._f["ogm_labels"](self._h, _ptr(labels)))

    def set_ext_boxes(self, ll, ur, active):
        ll = np.ascontiguousarray(ll, dtype=np.float32).reshape(-1, 3)
        ur = np.ascontiguousarray(ur, dtype=np.float32).reshape(-1, 3)
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(-1)
        self._chk(self._f["set_ext_boxes"](self._h, _ptr(ll), _ptr(ur), _ptr(act), ll.shape[0]))

    # --- stages ----------------------------------------------------------------------
    def fuse(self):
        self._chk(self._f["fuse"](self._h))

    def batch_edt(self):
        self._chk(self._f["batch_edt"](self._h))

    def merge(self):
        self._chk(self._f["merge"](self._h))

    def merge_begin_tiled(self):
        self._chk(self._f["merge_begin_tiled"](self._h))

    def merge_end(self):
        self._chk(self._f["merge_end"](self._h))

    def step(self):
        self._chk(self._f["step"](self._h))

    def step_begin_tiled(self):
        """fuse + batch EDT + the first half of the merge of a tiled run (the face layers are exported next)"""
        self.fuse(); self.batch_edt(); self.merge_begin_tiled()

    def sync(self):
        f = self._f.get("sync")
        if f:
            self._chk(f(self._h))

    # --- readers (arrays come back shaped [Z][Y][X], x fastest) ------------------------
    def _shape(self):
        return (self.size[2], self.size[1], self.size[0])

    def read_local(self, edt=True, vtype=True, dist_sq=True, coc=True):
        out = {}
        e = np.empty(self._shape(), np.float32) if edt else None
        t = np.empty(self._shape(), np.int8) if vtype else None
        d = np.empty(self._shape(), np.int32) if dist_sq else None
        c = np.empty(self._shape() + (3,), np.int32) if coc else None
        self._chk(self._f["read_local"](self._h, _ptr(e), _ptr(t), _ptr(d), _ptr(c)))
        for k, v in (("edt", e), ("type", t), ("dist_sq", d), ("coc", c)):
            if v is not None:
                out[k] = v
        return out

    def read_ogm(self):
        t = np.empty(self._shape(), np.int8)
        r = np.empty(self._shape(), np.int32)
        self._chk(self._f["read_ogm"](self._h, _ptr(t), _ptr(r)))
        return {"inst_type": t, "ray_count": r}

    def read_batch_edt(self):
        d = np.empty(self._shape(), np.int32)
        c = np.empty(self._shape() + (3,), np.int32)
        self._chk(self._f["read_batch_edt"](self._h, _ptr(d), _ptr(c)))
        return {"dist_sq": d, "coc": c}

    def read_costmap(self):
        pay = np.empty(self._shape(), SEENDIST_DTYPE)
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap"](self._h, _ptr(pay), C.byref(hdr)))
        return pay, hdr

    def read_costmap_dev(self, dptr):
        """The SeenDist payload into a device buffer (raw device address), asynchronous on the mapper's stream; returns the header."""
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_dev"](self._h, C.c_void_p(dptr), C.byref(hdr)))
        return hdr

    def costmap_publish(self):
        """Enqueue conversion + asynchronous copy into the library's pinned memory; returns the header at once."""
        hdr = CostMapHdr()
        self._chk(self._f["costmap_publish"](self._h, C.byref(hdr)))
        return hdr

    def costmap_acquire(self, copy=True):
        """Wait for the last publish; the payload as an array over the library's pinned buffer (copy=False: a VIEW that the publish
        after the next one overwrites)."""
        p = C.c_void_p()
        self._chk(self._f["costmap_acquire"](self._h, C.byref(p)))
        buf = (C.c_uint8 * (self.n * SEENDIST_DTYPE.itemsize)).from_address(p.value)
        a = np.frombuffer(buf, dtype=SEENDIST_DTYPE).reshape(self._shape())
        return a.copy() if copy else a

    def query_global_dev(self, d_xyz, n, d_out):
        """n lookups with coordinates (n x 3 int32) and results (n gie_voxel) in DEVICE buffers, enqueued on the mapper's stream."""
        self._chk(self._f["query_global_dev"](self._h, C.c_void_p(d_xyz), int(n), C.c_void_p(d_out)))

    def query_global(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
        out = np.empty(xyz.shape[0], VOXEL_DTYPE)
        self._chk(self._f["query_global"](self._h, _ptr(xyz), xyz.shape[0], _ptr(out)))
        return out

    def stats(self):
        s = FrameStats()
        self._chk(self._f["get_stats"](self._h, C.byref(s)))
        return s.as_dict()

    def pivot(self):
        p = (C.c_int32 * 3)()
        self._chk(self._f["get_pivot"](self._h, p))
        return tuple(p)

    # --- tiling (include/gie.h: halo exchange + refinement) ---------------------------------
    def set_tile(self, off, whole):
        o = (C.c_int32 * 3)(*[int(v) for v in off])
        w = (C.c_int32 * 3)(*[int(v) for v in whole])
        self._chk(self._f["set_tile"](self._h, o, w))

    def halo_count(self, face):
        return self._f["halo_count"](self._h, face)

    def halo_export(self, face):
        n = self._f["halo_count"](self._h, face)
        out = np.empty(n, HALO_DTYPE)
        self._chk(self._f["halo_export"](self._h, face, _ptr(out)))
        return out

    def halo_import(self, face, layer):
        layer = np.ascontiguousarray(layer, dtype=HALO_DTYPE)
        assert layer.shape[0] == self._f["halo_count"](self._h, face)
        self._chk(self._f["halo_import"](self._h, face, _ptr(layer)))

    def halo_export_sparse(self, face):
        """The layer's known voxels only: array of HALO_ENTRY_DTYPE (index in the layer, record), in no particular order."""
        n = self._f["halo_count"](self._h, face)
        out = np.empty(n, HALO_ENTRY_DTYPE)
        cnt = C.c_int32(0)
        self._chk(self._f["halo_export_sparse"](self._h, face, _ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def halo_import_sparse(self, face, entries):
        entries = np.ascontiguousarray(entries, dtype=HALO_ENTRY_DTYPE)
        self._chk(self._f["halo_import_sparse"](self._h, face, _ptr(entries), int(entries.shape[0])))

    # one face at a time, to / from a raw device address (the HIP library only)
    def halo_export_sparse_dev(self, face, dptr, dcount):
        self._chk(self._f["halo_export_sparse_dev"](self._h, face, C.c_void_p(dptr), C.c_void_p(dcount)))

    def halo_import_sparse_dev(self, face, dptr, dcount):
        self._chk(self._f["halo_import_sparse_dev"](self._h, face, C.c_void_p(dptr), C.c_void_p(dcount)))

    def halo_export_dev(self, face, dptr):
        self._chk(self._f["halo_export_dev"](self._h, face, C.c_void_p(dptr)))

    def halo_import_dev(self, face, dptr):
        self._chk(self._f["halo_import_dev"](self._h, face, C.c_void_p(dptr)))

    def refine(self):
        n = C.c_int32(0)
        self._chk(self._f["refine"](self._h, C.byref(n)))
        return n.value

    def refine_async(self):
        self._chk(self._f["refine"](self._h, None))

    def halo_export_all_dev(self, dptrs):
        """dptrs: {face: device pointer}; all faces in one launch."""
        arr = (C.c_void_p * 6)(*[dptrs.get(f) for f in range(6)])
        self._chk(self._f["halo_export_all_dev"](self._h, arr))

    def halo_import_all_dev(self, dptrs):
        arr = (C.c_void_p * 6)(*[dptrs.get(f) for f in range(6)])
        self._chk(self._f["halo_import_all_dev"](self._h, arr))

    # exchange rounds gated on the device (include/gie.h gie_round_gate ...): pointers are raw device addresses
    def round_gate(self, d_go):
        self._chk(self._f["round_gate"](self._h, C.c_void_p(d_go) if d_go else None))

    def refine_dev(self, d_changed):
        self._chk(self._f["refine_dev"](self._h, C.c_void_p(d_changed)))

    def round_end(self, d_go):
        self._chk(self._f["round_end"](self._h, C.c_void_p(d_go) if d_go else None))

    def round_stats(self):
        """{rounds_enqueued, rounds_run, updates, updates_unconverged} since the mapper was created (synchronises)."""
        v = (C.c_int64 * 4)()
        self._chk(self._f["round_stats"](self._h, v))
        return {"rounds_enqueued": int(v[0]), "rounds_run": int(v[1]), "updates": int(v[2]), "updates_unconverged": int(v[3])}

    # --- changed-block streaming (GlbHashMap::streamPipeline, glb_hash_map.cu:209-247) --------
    def stream_enable(self, on=True):
        self._chk(self._f["stream_enable"](self._h, 1 if on else 0))

    def stream_count(self):
        n = C.c_int32(0)
        self._chk(self._f["stream_changed"](self._h, None, None, 0, C.byref(n)))
        return n.value

    def stream_changed(self, max_blocks=None):
        """(keys [n,3] int32, blocks [n,512] VOXEL_DTYPE in get_voxID_in_VB order, flagged-before-call)."""
        total = self.stream_count()
        n = total if max_blocks is None else min(total, int(max_blocks))
        keys = np.empty((n, 3), np.int32)
        blocks = np.empty((n, 512), VOXEL_DTYPE)
        got = C.c_int32(0)
        if n:
            self._chk(self._f["stream_changed"](self._h, _ptr(keys), _ptr(blocks), n, C.byref(got)))
        return keys, blocks, total

    # --- VOLMAPNODE::publishMap call order (volumetric_mapper.cpp:138-224) -------------
    def update(self, pos, quat_wxyz, sensor_kind, sensor_data, tiled=False, **kw):
        """One map update.  tiled=True stops after the first half of the merge (gie_merge_begin_tiled): the exchange
        functions of gie.tiling export / import the face layers and finish the merge (gie_merge_end)."""
        self.set_pose(pos, quat_wxyz)
        if sensor_kind == "depth":
            self.ogm_depth(sensor_data, **kw)
        elif sensor_kind == "scan2d":
            self.ogm_scan2d(sensor_data, **kw)
        elif sensor_kind == "multiscan":
            self.ogm_multiscan(sensor_data, **kw)
        elif sensor_kind == "pointcloud":
            self.ogm_pointcloud(sensor_data)
        elif sensor_kind == "labels":
            self.ogm_labels(sensor_data)
        else:
            raise ValueError(sensor_kind)
        self.fuse()
        self.batch_edt()
        if tiled:
            self.merge_begin_tiled()
        else:
            self.merge()


_lib = None
_fns = None


def load_library(path=None):
    """Load the HIP C-ABI library. Raises if it has not been built (no fallback)."""
    global _lib, _fns
    if _fns is None:
        p = path or os.environ.get("GIE_LIB") or LIB_PATH    # GIE_LIB: another build of the same HIP library (ablation builds of tools/)
        if not os.path.exists(p):
            raise RuntimeError("%s not found: build it with __graft_entry__.build() "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64,
        # and a process that initialises the system runtime first (through this library) leaves torch
        # without a device ("No HIP GPUs are available").  Loaded the other way round, this library
        # binds to the runtime torch brought.  So: if torch is installed, let it load first.
        if "torch" not in sys.modules and not os.environ.get("GIE_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        _lib = C.CDLL(p)
        _fns = _capi.bind(_lib, "gie_", _capi.DEVICE_ONLY)
    return _fns


class Mapper(MapperBase):
    """The MI355X mapper (HIP kernels behind libgie_hip.so)."""

    def __init__(self, cfg):
        super().__init__(load_library(), cfg)

    def profile_enable(self, on=True):
        self._chk(self._f["profile_enable"](self._h, int(on)))

    def profile_read(self):
        """{kernel name: (total_ms, launches)} since the last read (synchronises)."""
        buf = (_capi.KernelTime * 32)()
        n = self._f["profile_read"](self._h, buf, 32)
        if n < 0:
            raise RuntimeError(self._err())
        return {buf[i].name.decode(): (buf[i].total_ms, buf[i].launches) for i in range(n)}

    # --- signed distance field of the local volume (include/gie.h) ---------------------------
    def read_sdf(self, sdf=True, inside_dist_sq=True):
        """{"sdf": float32 (voxel units), "inside_dist_sq": int32}, shaped [Z][Y][X] like read_local (synchronises)."""
        out = {}
        s = np.empty(self._shape(), np.float32) if sdf else None
        d = np.empty(self._shape(), np.int32) if inside_dist_sq else None
        self._chk(self._f["read_sdf"](self._h, _ptr(s), _ptr(d)))
        for k, v in (("sdf", s), ("inside_dist_sq", d)):
            if v is not None:
                out[k] = v
        return out

    def read_sdf_dev(self, d_sdf, d_inside_dist_sq):
        """The same planes into device buffers (raw device addresses, 0 = not wanted), asynchronous on the mapper's stream."""
        self._chk(self._f["read_sdf_dev"](self._h, C.c_void_p(d_sdf or None), C.c_void_p(d_inside_dist_sq or None)))

    def query_sdf(self, xyz):
        """n points (metres, world frame) -> (dist [n] float32 metres, grad [n,3] float32, flags [n] uint8) (synchronises)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        dist = np.empty(n, np.float32)
        grad = np.empty((n, 3), np.float32)
        flags = np.empty(n, np.uint8)
        self._chk(self._f["query_sdf"](self._h, _ptr(xyz), n, _ptr(dist), _ptr(grad), _ptr(flags)))
        return dist, grad, flags

    def query_sdf_dev(self, d_xyz, n, d_dist, d_grad, d_flags):
        """n queries with points (n x 3 float32) and results in DEVICE buffers (raw addresses, e.g. torch .data_ptr(); 0 = not
        wanted), enqueued on the mapper's stream; nothing is copied and the host does not wait."""
        self._chk(self._f["query_sdf_dev"](self._h, C.c_void_p(d_xyz or None), int(n), C.c_void_p(d_dist or None),
                                           C.c_void_p(d_grad or None), C.c_void_p(d_flags or None)))

    # --- NF1 navigation function of the local volume (include/gie.h) -----------------------
    def nf1_param(self, clearance=0.0, unknown_traversable=False, from_frontiers=False):
        """gie_nf1_param for a clearance in METRES: float32(clearance) / float32(voxel_width) voxels."""
        p = Nf1Param()
        p.clearance = float(np.float32(clearance) / np.float32(self.cfg.voxel_width))
        p.flags = (NF1_UNKNOWN_TRAVERSABLE if unknown_traversable else 0) | (NF1_FROM_FRONTIERS if from_frontiers else 0)
        return p

    def nf1_compute(self, goals=(), clearance=0.0, unknown_traversable=False, from_frontiers=False):
        """The field towards goal points (n x 3 metres, world frame) and/or the frontiers; returns the number of sources (synchronises)."""
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.float32).reshape(-1, 3))
        p = self.nf1_param(clearance, unknown_traversable, from_frontiers)
        ns = C.c_int32(0)
        self._chk(self._f["nf1_compute"](self._h, _ptr(g) if g.shape[0] else None, g.shape[0], C.byref(p), C.byref(ns)))
        return ns.value

    def nf1_compute_dev(self, d_goals, n, clearance=0.0, unknown_traversable=False, from_frontiers=False, d_n_sources=0):
        """The same with goals (n x 3 float32) and the source count (int32; 0 = not wanted) in DEVICE buffers, on the mapper's stream."""
        p = self.nf1_param(clearance, unknown_traversable, from_frontiers)
        self._chk(self._f["nf1_compute_dev"](self._h, C.c_void_p(d_goals or None), int(n), C.byref(p), C.c_void_p(d_n_sources or None)))

    def read_nf1(self):
        """int32 field [Z][Y][X] (synchronises)."""
        out = np.empty(self._shape(), np.int32)
        self._chk(self._f["read_nf1"](self._h, _ptr(out)))
        return out

    def read_nf1_dev(self, d_nf1):
        """The field into a device buffer (N int32, raw address), asynchronous on the mapper's stream."""
        self._chk(self._f["read_nf1_dev"](self._h, C.c_void_p(d_nf1 or None)))

    def nf1_path(self, starts, max_len):
        """Descents from start points (n x 3 metres): (list of (min(len, max_len), 3) int32 arrays of global voxels, len [n] int32)
        (synchronises)."""
        xyz = np.ascontiguousarray(np.asarray(starts, dtype=np.float32).reshape(-1, 3))
        n = xyz.shape[0]
        path = np.zeros((n, max(int(max_len), 1), 3), np.int32)
        ln = np.zeros(n, np.int32)
        if n:
            self._chk(self._f["nf1_path"](self._h, _ptr(xyz), n, int(max_len), _ptr(path), _ptr(ln)))
        return [path[i, :min(int(ln[i]), int(max_len))] for i in range(n)], ln

    def nf1_path_dev(self, d_starts, n, max_len, d_path, d_len):
        """n descents with starts (n x 3 float32), points (n x max_len x 3 int32) and lengths (n int32) in DEVICE buffers."""
        self._chk(self._f["nf1_path_dev"](self._h, C.c_void_p(d_starts or None), int(n), int(max_len), C.c_void_p(d_path or None),
                                          C.c_void_p(d_len or None)))

    def read_costmap_nf1(self):
        """The TYPE_NF1 CostMap: (SeenDist payload [Z][Y][X], header) (synchronises)."""
        pay = np.empty(self._shape(), SEENDIST_DTYPE)
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_nf1"](self._h, _ptr(pay), C.byref(hdr)))
        return pay, hdr

    def read_costmap_nf1_dev(self, dptr):
        """The TYPE_NF1 payload into a device buffer (raw address), asynchronous on the mapper's stream; returns the header."""
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_nf1_dev"](self._h, C.c_void_p(dptr or None), C.byref(hdr)))
        return hdr

    # --- goal-to-goal cost matrix of the local volume (include/gie.h) ------------------------
    def costmat(self, points, clearance=0.0, unknown_traversable=False):
        """Path lengths among n <= 64 points (n x 3 metres, world frame), clearance in METRES (as nf1_param):
        (cost [n, n] int32, valid [n] bool) (synchronises)."""
        xyz = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
        n = xyz.shape[0]
        p = self.nf1_param(clearance, unknown_traversable)
        cost = np.empty((n, n), np.int32)
        valid = np.zeros(n, np.uint8)
        self._chk(self._f["costmat_compute"](self._h, _ptr(xyz) if n else None, n, C.byref(p), _ptr(cost) if n else None,
                                             _ptr(valid) if n else None))
        return cost, valid.astype(bool)

    def costmat_dev(self, d_points, n, d_cost, d_valid=0, clearance=0.0, unknown_traversable=False):
        """The same with points (n x 3 float32), the matrix (n x n int32) and valid (n uint8; 0 = not wanted) in DEVICE buffers,
        on the mapper's stream; the host does not wait."""
        p = self.nf1_param(clearance, unknown_traversable)
        self._chk(self._f["costmat_compute_dev"](self._h, C.c_void_p(d_points or None), int(n), C.byref(p), C.c_void_p(d_cost or None),
                                                 C.c_void_p(d_valid or None)))

    # --- frontier clusters of the local volume (include/gie.h) ------------------------------
    def frontier_param(self, clearance=0.0, min_size=1, connectivity=26, max_clusters=256):
        """gie_frontier_param for a clearance in METRES: float32(clearance) / float32(voxel_width) voxels (as nf1_param)."""
        p = FrontierParam()
        p.clearance = float(np.float32(clearance) / np.float32(self.cfg.voxel_width))
        p.min_size, p.connectivity, p.max_clusters = int(min_size), int(connectivity), int(max_clusters)
        return p

    def frontier_compute(self, clearance=0.0, min_size=1, connectivity=26, max_clusters=256):
        """Connected components of the FNT voxels with `clearance` metres of free space, those of at least min_size voxels kept:
        (n_clusters, n_voxels) (synchronises).  n_clusters counts every kept component, also beyond max_clusters."""
        p = self.frontier_param(clearance, min_size, connectivity, max_clusters)
        nc, nv = C.c_int32(0), C.c_int32(0)
        self._chk(self._f["frontier_compute"](self._h, C.byref(p), C.byref(nc), C.byref(nv)))
        self._frontier_cap = p.max_clusters                   # (what the readers' buffers hold)
        return nc.value, nv.value

    def frontier_compute_dev(self, clearance=0.0, min_size=1, connectivity=26, max_clusters=256, d_counts=0):
        """The same on the mapper's stream; d_counts: 2 int32 in a DEVICE buffer (raw address; 0 = not wanted)."""
        p = self.frontier_param(clearance, min_size, connectivity, max_clusters)
        self._chk(self._f["frontier_compute_dev"](self._h, C.byref(p), C.c_void_p(d_counts or None)))
        self._frontier_cap = p.max_clusters

    def read_frontier_clusters(self):
        """(records, goal_xyz, n_clusters): the records produced (FRONTIER_CLUSTER_DTYPE, ascending label; at most the compute's
        max_clusters), the goal array [max_clusters, 3] float32 metres (NaN beyond the records) and the number of kept components
        (synchronises)."""
        cap = getattr(self, "_frontier_cap", 0)
        rec = np.zeros(max(cap, 1), FRONTIER_CLUSTER_DTYPE)
        goal = np.zeros((max(cap, 1), 3), np.float32)
        n = C.c_int32(0)
        self._chk(self._f["read_frontier_clusters"](self._h, _ptr(rec), _ptr(goal), C.byref(n)))
        return rec[:min(n.value, cap)], goal[:cap], n.value

    def read_frontier_clusters_dev(self, d_out, d_goal_xyz, d_n_clusters):
        """Records (max_clusters x 80 bytes), goal points (max_clusters x 3 float32) and the count (int32) into DEVICE buffers
        (raw addresses; 0 = not wanted), asynchronous on the mapper's stream."""
        self._chk(self._f["read_frontier_clusters_dev"](self._h, C.c_void_p(d_out or None), C.c_void_p(d_goal_xyz or None),
                                                        C.c_void_p(d_n_clusters or None)))

    def read_frontier_labels(self):
        """int32 label plane [Z][Y][X]: -1 not a member, -2 member of a filtered component, otherwise the label (synchronises)."""
        out = np.empty(self._shape(), np.int32)
        self._chk(self._f["read_frontier_labels"](self._h, _ptr(out)))
        return out

    def read_frontier_labels_dev(self, d_labels):
        """The label plane into a device buffer (N int32, raw address), asynchronous on the mapper's stream."""
        self._chk(self._f["read_frontier_labels_dev"](self._h, C.c_void_p(d_labels or None)))

    def stream_handle(self):
        """The mapper's HIP stream as an integer (for torch.cuda.ExternalStream)."""
        p = C.c_void_p()
        self._chk(self._f["get_stream"](self._h, C.byref(p)))
        return p.value or 0

    # device-resident sensor frames (pointers are raw device addresses, e.g. torch .data_ptr())
    def ogm_depth_dev(self, dptr, rows, cols, cx, cy, fx, fy, valid_nan=False):
        p = CamParam(rows, cols, cx, cy, fx, fy, int(valid_nan))
        self._chk(self._f["ogm_depth_dev"](self._h, C.c_void_p(dptr), C.byref(p)))

    def ogm_labels_dev(self, dptr, borrow=False):
        """A device-resident label plane.  borrow=True: gie_fuse may read it in place (returns whether it will): the plane must then
        stay unchanged until this update's fuse / step has run on the mapper's stream."""
        if not borrow:
            self._chk(self._f["ogm_labels_dev"](self._h, C.c_void_p(dptr)))
            return False
        b = C.c_int(0)
        self._chk(self._f["ogm_labels_dev_borrow"](self._h, C.c_void_p(dptr), C.byref(b)))
        return bool(b.value)

    def ogm_pointcloud_dev(self, dptr, n):
        self._chk(self._f["ogm_pointcloud_dev"](self._h, C.c_void_p(dptr), n))

    def ogm_multiscan_dev(self, dptr, scan_num, ring_num, theta_inc, theta_min, phi_inc, phi_min, max_r=100.0):
        p = MultiScanParam(scan_num, ring_num, max_r, theta_inc, theta_min, phi_inc, phi_min)
        self._chk(self._f["ogm_multiscan_dev"](self._h, C.c_void_p(dptr), C.byref(p)))

    # --- line of sight over the local volume (include/gie.h) --------------------------------
    def los_param(self, clearance=0.0, flags=0):
        """gie_los_param for a clearance in METRES: float32(clearance) / float32(voxel_width) voxels (as frontier_param)."""
        p = LosParam()
        p.clearance = float(np.float32(clearance) / np.float32(self.cfg.voxel_width))
        p.flags = int(flags)
        return p

    def los_prepare(self, clearance=0.0, flags=0):
        """The opaque plane of the current map (clearance in metres, flags: LOS_UNKNOWN_OPAQUE); returns the number of opaque
        voxels (synchronises)."""
        p = self.los_param(clearance, flags)
        n = C.c_int32(0)
        self._chk(self._f["los_prepare"](self._h, C.byref(p), C.byref(n)))
        return n.value

    def los_prepare_dev(self, clearance=0.0, flags=0, d_n_opaque=0):
        """The same on the mapper's stream; d_n_opaque: one int32 in a DEVICE buffer (raw address; 0 = not wanted)."""
        p = self.los_param(clearance, flags)
        self._chk(self._f["los_prepare_dev"](self._h, C.byref(p), C.c_void_p(d_n_opaque or None)))

    def read_los_opaque(self):
        """uint8 plane [Z][Y][X] of 0 / 1 (synchronises)."""
        out = np.empty(self._shape(), np.uint8)
        self._chk(self._f["read_los_opaque"](self._h, _ptr(out)))
        return out

    def read_los_opaque_dev(self, d_opaque):
        """The plane into a device buffer (N bytes, raw address), asynchronous on the mapper's stream."""
        self._chk(self._f["read_los_opaque_dev"](self._h, C.c_void_p(d_opaque or None)))

    def los_segments(self, a, b):
        """n segments between points a and b (n x 3 metres, world frame) -> LOS_HIT_DTYPE [n] (synchronises)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(-1, 3))
        if len(a) != len(b):
            raise ValueError("los_segments: as many start points as end points")
        out = np.zeros(len(a), LOS_HIT_DTYPE)
        self._chk(self._f["los_segments"](self._h, _ptr(a), _ptr(b), len(a), _ptr(out)))
        return out

    def los_segments_dev(self, d_a, d_b, n, d_out):
        """n segments with endpoints (n x 3 float32 each) and results (n x 24 bytes) in DEVICE buffers (raw addresses)."""
        self._chk(self._f["los_segments_dev"](self._h, C.c_void_p(d_a or None), C.c_void_p(d_b or None), int(n), C.c_void_p(d_out or None)))

    def view_param(self, r_min=0.0, r_max=1.0, tan2_elev=-1.0):
        p = ViewParam()
        p.r_min, p.r_max, p.tan2_elev = float(np.float32(r_min)), float(np.float32(r_max)), float(np.float32(tan2_elev))
        return p

    def view_gain(self, views, r_min=0.0, r_max=1.0, tan2_elev=-1.0):
        """Scores of n views (VIEW_DTYPE, see make_views; ranges in metres; tan2_elev < 0: no band) -> VIEW_SCORE_DTYPE [n]
        (synchronises)."""
        v = np.ascontiguousarray(np.asarray(views, dtype=VIEW_DTYPE).reshape(-1))
        p = self.view_param(r_min, r_max, tan2_elev)
        out = np.zeros(len(v), VIEW_SCORE_DTYPE)
        self._chk(self._f["view_gain"](self._h, _ptr(v), len(v), C.byref(p), _ptr(out)))
        return out

    def view_gain_dev(self, d_views, n, d_out, r_min=0.0, r_max=1.0, tan2_elev=-1.0):
        """n views (n x 64 bytes) and scores (n x 16 bytes) in DEVICE buffers (raw addresses), on the mapper's stream."""
        p = self.view_param(r_min, r_max, tan2_elev)
        self._chk(self._f["view_gain_dev"](self._h, C.c_void_p(d_views or None), int(n), C.byref(p), C.c_void_p(d_out or None)))

    # --- path shortcutting over the opaque plane (include/gie.h) -----------------------------
    def shortcut_param(self, lookahead, max_wp):
        p = ShortcutParam()
        p.lookahead, p.max_wp = int(lookahead), int(max_wp)
        return p

    def path_shortcut(self, paths, lens, lookahead, max_wp, wp=None):
        """Waypoints of n paths (paths: (n, max_len, 3) int32 global voxels and lens [n] int32, as nf1_path_dev leaves them) with a
        look-ahead of `lookahead` points: (wp [n, max_wp] WAYPOINT_DTYPE, info [n] SHORTCUT_INFO_DTYPE) (synchronises).  Only the
        first min(info.count, max_wp) records of a path are written: the rest of wp is zero, or what the caller's `wp` held."""
        pts = np.ascontiguousarray(np.asarray(paths, dtype=np.int32))
        if pts.ndim != 3 or pts.shape[2] != 3:
            raise ValueError("path_shortcut: paths must be (n, max_len, 3)")
        n, max_len = pts.shape[0], pts.shape[1]
        ln = np.ascontiguousarray(np.asarray(lens, dtype=np.int32).reshape(-1))
        if len(ln) != n:
            raise ValueError("path_shortcut: one length per path")
        max_wp = int(max_wp)
        if wp is None:
            wp = np.zeros((n, max(max_wp, 0)), WAYPOINT_DTYPE)
        elif wp.dtype != WAYPOINT_DTYPE or wp.shape != (n, max_wp) or not wp.flags.c_contiguous:
            raise ValueError("path_shortcut: wp must be a contiguous (n, max_wp) WAYPOINT_DTYPE array")
        info = np.zeros(n, SHORTCUT_INFO_DTYPE)
        p = self.shortcut_param(lookahead, max_wp)
        spare = np.zeros(1, WAYPOINT_DTYPE)                   # (an empty array has no address to give: n == 0, or max_wp == 0)
        self._chk(self._f["path_shortcut"](self._h, _ptr(pts) if pts.size else None, _ptr(ln) if n else None, n, max_len, C.byref(p),
                                           _ptr(wp if wp.size else spare), _ptr(info) if n else None))
        return wp, info

    def path_shortcut_dev(self, d_path, d_len, n, max_len, d_wp, d_info, lookahead, max_wp):
        """n paths with points (n x max_len x 3 int32), lengths (n int32), waypoints (n x max_wp x 24 bytes) and infos (n x 16 bytes)
        in DEVICE buffers (raw addresses; 0 = not wanted), on the mapper's stream."""
        p = self.shortcut_param(lookahead, max_wp)
        self._chk(self._f["path_shortcut_dev"](self._h, C.c_void_p(d_path or None), C.c_void_p(d_len or None), int(n), int(max_len), C.byref(p),
                                               C.c_void_p(d_wp or None), C.c_void_p(d_info or None)))

    # --- display clouds (include/gie.h) -------------------------------------------------------
    def cloud_param(self, type_mask, intensity=CLOUD_TYPE, z_lo=None, z_hi=None, max_points=0):
        """gie_cloud_param: type_mask = bits 1 << VOX_*; z_lo / z_hi = GLOBAL voxel z, inclusive (None: open on that side)."""
        p = CloudParam()
        p.type_mask, p.intensity, p.max_points = int(type_mask), int(intensity), int(max_points)
        p.z_lo = CLOUD_NO_BAND[0] if z_lo is None else int(z_lo)
        p.z_hi = CLOUD_NO_BAND[1] if z_hi is None else int(z_hi)
        return p

    def _cloud(self, name, type_mask, intensity, z_lo, z_hi, max_points, out):
        n = C.c_int32(0)
        if max_points is None:                              # count first, then fetch
            if out is not None:
                max_points = len(out)
            else:
                p = self.cloud_param(type_mask, intensity, z_lo, z_hi, 0)
                self._chk(self._f[name](self._h, C.byref(p), None, C.byref(n)))
                max_points = n.value
        max_points = int(max_points)
        if out is None:
            out = np.zeros(max(max_points, 0), CLOUD_DTYPE)
        elif out.dtype != CLOUD_DTYPE or out.ndim != 1 or len(out) < max_points or not out.flags.c_contiguous:
            raise ValueError("%s: out must be a contiguous CLOUD_DTYPE array of at least max_points records" % name)
        p = self.cloud_param(type_mask, intensity, z_lo, z_hi, max_points)
        self._chk(self._f[name](self._h, C.byref(p), _ptr(out) if out.size else None, C.byref(n)))
        return out[:min(n.value, max_points)], n.value

    def cloud_local(self, type_mask, intensity=CLOUD_TYPE, z_lo=None, z_hi=None, max_points=None, out=None):
        """The selected voxels of the local volume -> (points, count): points = the written records (CLOUD_DTYPE, a view of `out`
        when one is given), count = all selected voxels, also beyond max_points.  max_points=None counts first, then fetches all
        (or takes len(out)).  Synchronises."""
        return self._cloud("cloud_local", type_mask, intensity, z_lo, z_hi, max_points, out)

    def cloud_global(self, type_mask, intensity=CLOUD_TYPE, z_lo=None, z_hi=None, max_points=None, out=None):
        """The same over every live block of the global map."""
        return self._cloud("cloud_global", type_mask, intensity, z_lo, z_hi, max_points, out)

    def cloud_local_dev(self, d_out, d_count, type_mask, intensity=CLOUD_TYPE, z_lo=None, z_hi=None, max_points=0):
        """Records (max_points x 16 bytes, 16-byte aligned) and the count (one int32) in DEVICE buffers (raw addresses; 0 = not
        wanted), on the mapper's stream without a host wait."""
        p = self.cloud_param(type_mask, intensity, z_lo, z_hi, max_points)
        self._chk(self._f["cloud_local_dev"](self._h, C.byref(p), C.c_void_p(d_out or None), C.c_void_p(d_count or None)))

    def cloud_global_dev(self, d_out, d_count, type_mask, intensity=CLOUD_TYPE, z_lo=None, z_hi=None, max_points=0):
        p = self.cloud_param(type_mask, intensity, z_lo, z_hi, max_points)
        self._chk(self._f["cloud_global_dev"](self._h, C.byref(p), C.c_void_p(d_out or None), C.c_void_p(d_count or None)))

    # --- global block summaries (include/gie.h) -------------------------------------------------
    def blocks_param(self, lo=None, hi=None, dist=False, min_fnt=0, max_records=0):
        """gie_blocks_param: lo / hi = BLOCK coordinates (global voxel >> 3), both inclusive; None, or None on an axis: open there."""
        p = BlocksParam()
        for k in range(3):
            p.lo[k] = CLOUD_NO_BAND[0] if lo is None or lo[k] is None else int(lo[k])
            p.hi[k] = CLOUD_NO_BAND[1] if hi is None or hi[k] is None else int(hi[k])
        p.flags, p.min_fnt, p.max_records = BLOCKS_DIST if dist else 0, int(min_fnt), int(max_records)
        return p

    def blocks_summary(self, lo=None, hi=None, dist=False, min_fnt=0, max_records=None, grid=False, dev=False):
        """One record per qualifying block of the global map with n_fnt >= min_fnt -> (records, count) or, with grid=True (a finite
        box lo..hi), (records, count, grid): records = the written ones (BLOCK_SUMMARY_DTYPE, unspecified order), count = all of
        them, also beyond max_records (None: count first, then fetch all), grid = uint32 [nz][ny][nx] over the box.  dev=True takes
        the same through gie_blocks_summary_dev and torch buffers on the mapper's stream.  Synchronises."""
        n = C.c_int32(0)
        if max_records is None:
            p = self.blocks_param(lo, hi, dist, min_fnt, 0)
            self._chk(self._f["blocks_summary"](self._h, C.byref(p), None, C.byref(n), None))
            max_records = n.value
        max_records = int(max_records)
        p = self.blocks_param(lo, hi, dist, min_fnt, max_records)
        shape = tuple(int(p.hi[k]) - int(p.lo[k]) + 1 for k in (2, 1, 0)) if grid else None
        if grid and not all(0 < s <= 1024 for s in shape):
            raise ValueError("blocks_summary: a grid needs a finite box of at most 1024 blocks a side")
        out = np.zeros(max(max_records, 0), BLOCK_SUMMARY_DTYPE)
        g = np.zeros(shape, np.uint32) if grid else None
        if dev:
            import torch
            d = torch.device("cuda", int(self.cfg.device_id))
            with torch.cuda.stream(torch.cuda.ExternalStream(self.stream_handle(), device=d)):
                dout = torch.zeros(max(out.nbytes, 16), dtype=torch.uint8, device=d)
                dcnt = torch.zeros(1, dtype=torch.int32, device=d)
                dg = torch.zeros(g.size, dtype=torch.int32, device=d) if grid else None
                self.blocks_summary_dev(dout.data_ptr() if max_records > 0 else 0, dcnt.data_ptr(), dg.data_ptr() if grid else 0, lo, hi, dist, min_fnt, max_records)
            self.sync()
            n.value = int(dcnt.cpu()[0])
            out = dout.cpu().numpy()[:out.nbytes].view(BLOCK_SUMMARY_DTYPE).copy()
            if grid:
                g = dg.cpu().numpy().view(np.uint32).reshape(shape)
        else:
            self._chk(self._f["blocks_summary"](self._h, C.byref(p), _ptr(out) if out.size else None, C.byref(n), _ptr(g)))
        res = (out[:min(n.value, max_records)], n.value)
        return res + (g,) if grid else res

    def blocks_summary_dev(self, d_out, d_count, d_grid, lo=None, hi=None, dist=False, min_fnt=0, max_records=0):
        """Records (max_records x 32 bytes, 16-byte aligned), the count (one int32) and the grid (one uint32 per cell of the box) in
        DEVICE buffers (raw addresses; 0 = not wanted), on the mapper's stream without a host wait."""
        p = self.blocks_param(lo, hi, dist, min_fnt, max_records)
        self._chk(self._f["blocks_summary_dev"](self._h, C.byref(p), C.c_void_p(d_out or None), C.c_void_p(d_count or None), C.c_void_p(d_grid or None)))

    # --- global block routes (include/gie.h) ----------------------------------------------------
    def routes_param(self, lo, hi, min_free=1, min_open=1, min_fnt=1, from_frontiers=False):
        """gie_routes_param: lo / hi = a finite box of BLOCK coordinates (global voxel >> 3), both inclusive."""
        p = RoutesParam()
        for k in range(3):
            p.lo[k] = CLOUD_NO_BAND[0] if lo is None or lo[k] is None else int(lo[k])
            p.hi[k] = CLOUD_NO_BAND[1] if hi is None or hi[k] is None else int(hi[k])
        p.min_free, p.min_open, p.min_fnt, p.flags = int(min_free), int(min_open), int(min_fnt), ROUTES_FROM_FRONTIERS if from_frontiers else 0
        return p

    def routes_compute(self, lo, hi, goals=(), min_free=1, min_open=1, min_fnt=1, from_frontiers=False):
        """Links and BFS field of the blocks of the box lo..hi from goal points (n x 3 metres, world frame) and / or the frontier
        blocks; the result is kept until the next compute.  Returns the info record (ROUTES_INFO scalar; synchronises)."""
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.float32).reshape(-1, 3))
        p = self.routes_param(lo, hi, min_free, min_open, min_fnt, from_frontiers)
        info = np.zeros(1, ROUTES_INFO)
        self._chk(self._f["routes_compute"](self._h, _ptr(g) if g.shape[0] else None, g.shape[0], C.byref(p), _ptr(info)))
        self._routes_shape = tuple(int(p.hi[k]) - int(p.lo[k]) + 1 for k in (2, 1, 0))
        return info[0]

    def routes_compute_dev(self, d_goals, n, lo, hi, min_free=1, min_open=1, min_fnt=1, from_frontiers=False, d_info=0):
        """The same on the mapper's stream without a host wait; goals (n x 3 float32) and the info record (32 bytes; 0 = not wanted)
        in DEVICE buffers (raw addresses)."""
        p = self.routes_param(lo, hi, min_free, min_open, min_fnt, from_frontiers)
        self._chk(self._f["routes_compute_dev"](self._h, C.c_void_p(d_goals or None), int(n), C.byref(p), C.c_void_p(d_info or None)))
        self._routes_shape = tuple(int(p.hi[k]) - int(p.lo[k]) + 1 for k in (2, 1, 0))

    def routes_read(self):
        """(steps int32 [nz][ny][nx], cell bytes uint8 [nz][ny][nx]) of the kept box (synchronises)."""
        shape = getattr(self, "_routes_shape", None)
        if shape is None:
            raise RuntimeError("routes_read: no routes yet (routes_compute first)")
        steps, cells = np.empty(shape, np.int32), np.empty(shape, np.uint8)
        self._chk(self._f["read_routes"](self._h, _ptr(steps), _ptr(cells)))
        return steps, cells

    def routes_read_dev(self, d_steps, d_cells):
        """The field (int32 per cell) and the cell bytes into DEVICE buffers (raw addresses; 0 = not wanted), on the mapper's stream."""
        self._chk(self._f["read_routes_dev"](self._h, C.c_void_p(d_steps or None), C.c_void_p(d_cells or None)))

    def routes_query(self, xyz):
        """The kept field at the blocks of n points (n x 3 metres, world frame): int32 [n] steps, -1 outside the box, for a point
        that is not finite, on a cell without a node and where no source is reachable (synchronises)."""
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        out = np.zeros(xyz.shape[0], np.int32)
        self._chk(self._f["routes_query"](self._h, _ptr(xyz) if len(xyz) else None, len(xyz), _ptr(out) if len(xyz) else None))
        return out

    def routes_query_dev(self, d_xyz, n, d_steps):
        """n points (n x 3 float32) and their steps (n int32) in DEVICE buffers (raw addresses), on the mapper's stream."""
        self._chk(self._f["routes_query_dev"](self._h, C.c_void_p(d_xyz or None), int(n), C.c_void_p(d_steps or None)))

    def routes_path(self, starts, max_len, path=None):
        """Descents from n start points (n x 3 metres): (path [n, max_len, 3] int32 BLOCK coordinates, len [n] int32 = steps + 1, 0
        without a path).  Only the first min(len, max_len) blocks of a path are written: the rest is zero, or what the caller's
        `path` held (synchronises)."""
        xyz = np.ascontiguousarray(np.asarray(starts, dtype=np.float32).reshape(-1, 3))
        n, max_len = xyz.shape[0], int(max_len)
        if path is None:
            path = np.zeros((n, max(max_len, 1), 3), np.int32)
        elif path.dtype != np.int32 or path.shape != (n, max_len, 3) or not path.flags.c_contiguous:
            raise ValueError("routes_path: path must be a contiguous (n, max_len, 3) int32 array")
        ln = np.zeros(n, np.int32)
        self._chk(self._f["routes_path"](self._h, _ptr(xyz) if n else None, n, max_len, _ptr(path) if n else None, _ptr(ln) if n else None))
        return path, ln

    def routes_path_dev(self, d_starts, n, max_len, d_path, d_len):
        """n starts (n x 3 float32), keys (n x max_len x 3 int32) and lengths (n int32) in DEVICE buffers, on the mapper's stream."""
        self._chk(self._f["routes_path_dev"](self._h, C.c_void_p(d_starts or None), int(n), int(max_len), C.c_void_p(d_path or None), C.c_void_p(d_len or None)))

    # --- ground costmap of a height band (include/gie.h) ---------------------------------------
    def ground_param(self, z_lo, z_hi, min_known=1, unknown_blocks=False):
        """gie_ground_param: z_lo / z_hi = GLOBAL voxel z, both inclusive."""
        p = GroundParam()
        p.z_lo, p.z_hi, p.min_known, p.flags = int(z_lo), int(z_hi), int(min_known), GROUND_UNKNOWN_BLOCKS if unknown_blocks else 0
        return p

    def ground_compute(self, z_lo, z_hi, min_known=1, unknown_blocks=False):
        """The column types of the band and their 2-D distance transform; returns the counts [UNKNOWN, FREE, OCCUPIED, FNT] (synchronises)."""
        p = self.ground_param(z_lo, z_hi, min_known, unknown_blocks)
        counts = np.zeros(4, np.int32)
        self._chk(self._f["ground_compute"](self._h, C.byref(p), _ptr(counts)))
        return counts

    def ground_compute_dev(self, z_lo, z_hi, min_known=1, unknown_blocks=False, d_counts=0):
        """The same on the mapper's stream without a host wait; the counts (4 int32; 0 = not wanted) in a DEVICE buffer."""
        p = self.ground_param(z_lo, z_hi, min_known, unknown_blocks)
        self._chk(self._f["ground_compute_dev"](self._h, C.byref(p), C.c_void_p(d_counts or None)))

    def read_ground(self):
        """{"type": int8, "dist_sq": int32, "coc": int32 (.., 2) global x y, "top": int32 global z}, shaped [Y][X] (synchronises)."""
        s = (self.size[1], self.size[0])
        out = {"type": np.empty(s, np.int8), "dist_sq": np.empty(s, np.int32), "coc": np.empty(s + (2,), np.int32), "top": np.empty(s, np.int32)}
        self._chk(self._f["read_ground"](self._h, _ptr(out["type"]), _ptr(out["dist_sq"]), _ptr(out["coc"]), _ptr(out["top"])))
        return out

    def read_ground_dev(self, d_type, d_dist_sq, d_coc_xy, d_top):
        """The same planes into device buffers (raw device addresses, 0 = not wanted), asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_dev"](self._h, C.c_void_p(d_type or None), C.c_void_p(d_dist_sq or None), C.c_void_p(d_coc_xy or None),
                                             C.c_void_p(d_top or None)))

    def read_costmap_ground(self):
        """The one-layer TYPE_EDT CostMap of the ground field: (SeenDist payload [Y][X], header) (synchronises)."""
        pay = np.empty((self.size[1], self.size[0]), SEENDIST_DTYPE)
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_ground"](self._h, _ptr(pay), C.byref(hdr)))
        return pay, hdr

    def read_costmap_ground_dev(self, dptr):
        """That payload into a device buffer (raw address), asynchronous on the mapper's stream; returns the header."""
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_ground_dev"](self._h, C.c_void_p(dptr or None), C.byref(hdr)))
        return hdr

    def ground_query(self, xy):
        """n points (n x 2 metres, world frame) -> their cells' records (GROUND_CELL_DTYPE) (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        out = np.zeros(xy.shape[0], GROUND_CELL_DTYPE)
        self._chk(self._f["ground_query"](self._h, _ptr(xy) if len(xy) else None, len(xy), _ptr(out) if len(xy) else None))
        return out

    def ground_query_dev(self, d_xy, n, d_out):
        """n queries with points (n x 2 float32) and records (n x 16 bytes) in DEVICE buffers, on the mapper's stream."""
        self._chk(self._f["ground_query_dev"](self._h, C.c_void_p(d_xy or None), int(n), C.c_void_p(d_out or None)))

    # --- NF1 navigation function of the ground costmap (include/gie.h) --------------------------
    def ground_nf1_param(self, clearance_sq=0, unknown_traversable=False, from_frontiers=False):
        """gie_ground_nf1_param: clearance_sq in squared CELLS, compared with the ground field's dist_sq."""
        p = GroundNf1Param()
        p.clearance_sq = int(clearance_sq)
        p.flags = (GROUND_NF1_UNKNOWN_TRAVERSABLE if unknown_traversable else 0) | (GROUND_NF1_FROM_FRONTIERS if from_frontiers else 0)
        return p

    def ground_nf1_compute(self, goals=(), clearance_sq=0, unknown_traversable=False, from_frontiers=False):
        """NF1 of the current ground field from goal points (n x 2 metres, world frame) and / or its FNT cells; returns the number
        of sources (synchronises)."""
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.float32).reshape(-1, 2))
        p = self.ground_nf1_param(clearance_sq, unknown_traversable, from_frontiers)
        ns = C.c_int32(0)
        self._chk(self._f["ground_nf1_compute"](self._h, _ptr(g) if g.shape[0] else None, g.shape[0], C.byref(p), C.byref(ns)))
        return ns.value

    def ground_nf1_compute_dev(self, d_goals, n, clearance_sq=0, unknown_traversable=False, from_frontiers=False, d_n_sources=0):
        """The same on the mapper's stream without a host wait; goals (n x 2 float32) and the source count (one int32; 0 = not
        wanted) in DEVICE buffers (raw addresses)."""
        p = self.ground_nf1_param(clearance_sq, unknown_traversable, from_frontiers)
        self._chk(self._f["ground_nf1_compute_dev"](self._h, C.c_void_p(d_goals or None), int(n), C.byref(p), C.c_void_p(d_n_sources or None)))

    def read_ground_nf1(self):
        """int32 field [Y][X]: steps to the nearest source, -1 where none is reachable (synchronises)."""
        out = np.empty((self.size[1], self.size[0]), np.int32)
        self._chk(self._f["read_ground_nf1"](self._h, _ptr(out)))
        return out

    def read_ground_nf1_dev(self, d_nf1):
        """The field into a device buffer (X * Y int32, raw address), asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_nf1_dev"](self._h, C.c_void_p(d_nf1 or None)))

    def ground_nf1_path(self, starts, max_len, path=None):
        """Descents from n start points (n x 2 metres): (path [n, max_len, 2] int32 GLOBAL x y, len [n] int32 = nf1(start) + 1, 0
        without a path).  Only the first min(len, max_len) points of a path are written: the rest is zero, or what the caller's
        `path` held (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(starts, dtype=np.float32).reshape(-1, 2))
        n, max_len = xy.shape[0], int(max_len)
        if path is None:
            path = np.zeros((n, max(max_len, 1), 2), np.int32)
        elif path.dtype != np.int32 or path.shape != (n, max_len, 2) or not path.flags.c_contiguous:
            raise ValueError("ground_nf1_path: path must be a contiguous (n, max_len, 2) int32 array")
        ln = np.zeros(n, np.int32)
        self._chk(self._f["ground_nf1_path"](self._h, _ptr(xy) if n else None, n, max_len, _ptr(path) if n else None, _ptr(ln) if n else None))
        return path, ln

    def ground_nf1_path_dev(self, d_starts, n, max_len, d_path, d_len):
        """n starts (n x 2 float32), points (n x max_len x 2 int32) and lengths (n int32) in DEVICE buffers, on the mapper's stream."""
        self._chk(self._f["ground_nf1_path_dev"](self._h, C.c_void_p(d_starts or None), int(n), int(max_len), C.c_void_p(d_path or None),
                                                 C.c_void_p(d_len or None)))

    # --- ground line of sight: segment checks and any-angle paths on the ground costmap (include/gie.h) ---
    def ground_los_param(self, clearance_sq=0, unknown_traversable=False):
        """gie_ground_los_param: clearance_sq in squared CELLS, compared with the ground field's dist_sq."""
        p = GroundLosParam()
        p.clearance_sq, p.flags = int(clearance_sq), GROUND_LOS_UNKNOWN_TRAVERSABLE if unknown_traversable else 0
        return p

    def ground_segments(self, a, b, clearance_sq=0, unknown_traversable=False):
        """n segments between points a and b (n x 2 metres, world frame) over the current ground field -> GROUND_HIT_DTYPE [n]
        (synchronises)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 2))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(-1, 2))
        if len(a) != len(b):
            raise ValueError("ground_segments: as many start points as end points")
        out = np.zeros(len(a), GROUND_HIT_DTYPE)
        p = self.ground_los_param(clearance_sq, unknown_traversable)
        n = len(a)
        self._chk(self._f["ground_segments"](self._h, _ptr(a) if n else None, _ptr(b) if n else None, n, C.byref(p), _ptr(out) if n else None))
        return out

    def ground_segments_dev(self, d_a, d_b, n, d_out, clearance_sq=0, unknown_traversable=False):
        """n segments with endpoints (n x 2 float32 each) and results (n x 24 bytes) in DEVICE buffers (raw addresses), on the
        mapper's stream."""
        p = self.ground_los_param(clearance_sq, unknown_traversable)
        self._chk(self._f["ground_segments_dev"](self._h, C.c_void_p(d_a or None), C.c_void_p(d_b or None), int(n), C.byref(p), C.c_void_p(d_out or None)))

    def ground_shortcut_param(self, lookahead, max_wp, clearance_sq=0, unknown_traversable=False):
        p = GroundShortcutParam()
        p.lookahead, p.max_wp, p.clearance_sq = int(lookahead), int(max_wp), int(clearance_sq)
        p.flags = GROUND_LOS_UNKNOWN_TRAVERSABLE if unknown_traversable else 0
        return p

    def ground_shortcut(self, paths, lens, lookahead, max_wp, clearance_sq=0, unknown_traversable=False, wp=None):
        """Waypoints of n paths (paths: (n, max_len, 2) int32 global cells and lens [n] int32, as ground_nf1_path leaves them) with a
        look-ahead of `lookahead` points: (wp [n, max_wp] GROUND_WAYPOINT_DTYPE, info [n] SHORTCUT_INFO_DTYPE) (synchronises).  Only
        the first min(info.count, max_wp) records of a path are written: the rest of wp is zero, or what the caller's `wp` held."""
        pts = np.ascontiguousarray(np.asarray(paths, dtype=np.int32))
        if pts.ndim != 3 or pts.shape[2] != 2:
            raise ValueError("ground_shortcut: paths must be (n, max_len, 2)")
        n, max_len = pts.shape[0], pts.shape[1]
        ln = np.ascontiguousarray(np.asarray(lens, dtype=np.int32).reshape(-1))
        if len(ln) != n:
            raise ValueError("ground_shortcut: one length per path")
        max_wp = int(max_wp)
        if wp is None:
            wp = np.zeros((n, max(max_wp, 0)), GROUND_WAYPOINT_DTYPE)
        elif wp.dtype != GROUND_WAYPOINT_DTYPE or wp.shape != (n, max_wp) or not wp.flags.c_contiguous:
            raise ValueError("ground_shortcut: wp must be a contiguous (n, max_wp) GROUND_WAYPOINT_DTYPE array")
        info = np.zeros(n, SHORTCUT_INFO_DTYPE)
        p = self.ground_shortcut_param(lookahead, max_wp, clearance_sq, unknown_traversable)
        spare = np.zeros(1, GROUND_WAYPOINT_DTYPE)            # (an empty array has no address to give: n == 0, or max_wp == 0)
        self._chk(self._f["ground_shortcut"](self._h, _ptr(pts) if pts.size else None, _ptr(ln) if n else None, n, max_len, C.byref(p),
                                             _ptr(wp if wp.size else spare), _ptr(info) if n else None))
        return wp, info

    def ground_shortcut_dev(self, d_path, d_len, n, max_len, d_wp, d_info, lookahead, max_wp, clearance_sq=0, unknown_traversable=False):
        """n paths with points (n x max_len x 2 int32), lengths (n int32), waypoints (n x max_wp x 24 bytes) and infos (n x 16 bytes)
        in DEVICE buffers (raw addresses; 0 = not wanted), on the mapper's stream."""
        p = self.ground_shortcut_param(lookahead, max_wp, clearance_sq, unknown_traversable)
        self._chk(self._f["ground_shortcut_dev"](self._h, C.c_void_p(d_path or None), C.c_void_p(d_len or None), int(n), int(max_len), C.byref(p),
                                                 C.c_void_p(d_wp or None), C.c_void_p(d_info or None)))

    # --- ground frontier clusters and route costs to them (include/gie.h) ------------------------
    def ground_frontier_param(self, clearance_sq=0, min_size=1, connectivity=8, max_clusters=256):
        """gie_ground_frontier_param: clearance_sq in squared CELLS, compared with the ground field's dist_sq (as ground_nf1_param)."""
        p = GroundFrontierParam()
        p.clearance_sq, p.min_size, p.connectivity, p.max_clusters = int(clearance_sq), int(min_size), int(connectivity), int(max_clusters)
        return p

    def ground_frontier_compute(self, clearance_sq=0, min_size=1, connectivity=8, max_clusters=256):
        """Connected components (connectivity 4 or 8) of the current ground field's FNT cells with clearance_sq, those of at least
        min_size cells kept: (n_clusters, n_cells) (synchronises).  n_clusters counts every kept component, also beyond max_clusters."""
        p = self.ground_frontier_param(clearance_sq, min_size, connectivity, max_clusters)
        nc, nv = C.c_int32(0), C.c_int32(0)
        self._chk(self._f["ground_frontier_compute"](self._h, C.byref(p), C.byref(nc), C.byref(nv)))
        self._ground_frontier_cap = p.max_clusters            # (what the readers' buffers hold)
        return nc.value, nv.value

    def ground_frontier_compute_dev(self, clearance_sq=0, min_size=1, connectivity=8, max_clusters=256, d_counts=0):
        """The same on the mapper's stream without a host wait; d_counts: 2 int32 in a DEVICE buffer (raw address; 0 = not wanted)."""
        p = self.ground_frontier_param(clearance_sq, min_size, connectivity, max_clusters)
        self._chk(self._f["ground_frontier_compute_dev"](self._h, C.byref(p), C.c_void_p(d_counts or None)))
        self._ground_frontier_cap = p.max_clusters

    def read_ground_frontier_clusters(self):
        """(records, goal_xy, n_clusters): the records produced (GROUND_FRONTIER_CLUSTER_DTYPE, ascending label; at most the
        compute's max_clusters), the goal array [max_clusters, 2] float32 metres (NaN beyond the records) and the number of kept
        components (synchronises)."""
        cap = getattr(self, "_ground_frontier_cap", 0)
        rec = np.zeros(max(cap, 1), GROUND_FRONTIER_CLUSTER_DTYPE)
        goal = np.zeros((max(cap, 1), 2), np.float32)
        n = C.c_int32(0)
        self._chk(self._f["read_ground_frontier_clusters"](self._h, _ptr(rec), _ptr(goal), C.byref(n)))
        return rec[:min(n.value, cap)], goal[:cap], n.value

    def read_ground_frontier_clusters_dev(self, d_out, d_goal_xy, d_n_clusters):
        """Records (max_clusters x 64 bytes), goal points (max_clusters x 2 float32) and the count (int32) into DEVICE buffers
        (raw addresses; 0 = not wanted, not both of the first two), asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_frontier_clusters_dev"](self._h, C.c_void_p(d_out or None), C.c_void_p(d_goal_xy or None),
                                                               C.c_void_p(d_n_clusters or None)))

    def read_ground_frontier_labels(self):
        """int32 label plane [Y][X]: -1 not a member, -2 member of a filtered component, otherwise the label (synchronises)."""
        out = np.empty((self.size[1], self.size[0]), np.int32)
        self._chk(self._f["read_ground_frontier_labels"](self._h, _ptr(out)))
        return out

    def read_ground_frontier_labels_dev(self, d_labels):
        """The label plane into a device buffer (X * Y int32, raw address), asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_frontier_labels_dev"](self._h, C.c_void_p(d_labels or None)))

    def ground_nf1_query(self, xy):
        """The current ground navigation function at n points (n x 2 metres, world frame): int32 [n] steps, -1 outside the field,
        for a point that is not finite and where no source is reachable (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        out = np.zeros(xy.shape[0], np.int32)
        self._chk(self._f["ground_nf1_query"](self._h, _ptr(xy) if len(xy) else None, len(xy), _ptr(out) if len(xy) else None))
        return out

    def ground_nf1_query_dev(self, d_xy, n, d_steps):
        """n points (n x 2 float32) and their steps (n int32) in DEVICE buffers (raw addresses), on the mapper's stream."""
        self._chk(self._f["ground_nf1_query_dev"](self._h, C.c_void_p(d_xy or None), int(n), C.c_void_p(d_steps or None)))

    # --- ground cost matrix: route lengths among points on the ground costmap (include/gie.h) -----
    def ground_costmat(self, points, clearance_sq=0, unknown_traversable=False):
        """4-connected route lengths among n <= 256 points (n x 2 metres, world frame) over the current ground field, clearance_sq
        in squared CELLS (as ground_nf1_param): (cost [n, n] int32, valid [n] bool) (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 2))
        n = xy.shape[0]
        p = self.ground_nf1_param(clearance_sq, unknown_traversable)
        cost = np.empty((n, n), np.int32)
        valid = np.zeros(n, np.uint8)
        self._chk(self._f["ground_costmat_compute"](self._h, _ptr(xy) if n else None, n, C.byref(p), _ptr(cost) if n else None,
                                                    _ptr(valid) if n else None))
        return cost, valid.astype(bool)

    def ground_costmat_dev(self, d_points, n, d_cost, d_valid=0, clearance_sq=0, unknown_traversable=False):
        """The same with points (n x 2 float32), the matrix (n x n int32) and valid (n uint8; 0 = not wanted) in DEVICE buffers
        (raw addresses), on the mapper's stream; the host does not wait."""
        p = self.ground_nf1_param(clearance_sq, unknown_traversable)
        self._chk(self._f["ground_costmat_compute_dev"](self._h, C.c_void_p(d_points or None), int(n), C.byref(p), C.c_void_p(d_cost or None),
                                                        C.c_void_p(d_valid or None)))

    # --- ground view gain: visible cells per candidate pose on the ground costmap (include/gie.h) ---
    def ground_view_param(self, r_min=0.0, r_max=1.0, n_planes=0, unknown_opaque=False, union=False):
        """gie_ground_view_param: ranges in metres; n_planes half planes per view, `union` for a sector wider than 180 degrees."""
        p = GroundViewParam()
        p.r_min, p.r_max, p.n_planes = float(r_min), float(r_max), int(n_planes)
        p.flags = (GROUND_VIEW_UNKNOWN_OPAQUE if unknown_opaque else 0) | (GROUND_VIEW_UNION if union else 0)
        return p

    @staticmethod
    def _ground_view_arrays(who, xy, normals, n_planes):
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        nr = None
        if n_planes > 0:
            nr = np.ascontiguousarray(np.asarray(normals, dtype=np.int32).reshape(-1, n_planes, 2))
            if len(nr) != len(xy):
                raise ValueError(who + ": n_planes normals per view")
        return xy, nr

    def ground_view_gain(self, xy, r_min=0.0, r_max=1.0, normals=None, n_planes=0, unknown_opaque=False, union=False):
        """Scores of n views at points xy (n x 2 metres, world frame) over the current ground field, each cut by n_planes half planes
        (normals: n x n_planes x 2 int32, x then y) -> VIEW_SCORE_DTYPE [n] (synchronises)."""
        xy, nr = self._ground_view_arrays("ground_view_gain", xy, normals, int(n_planes))
        n = len(xy)
        out = np.zeros(n, VIEW_SCORE_DTYPE)
        p = self.ground_view_param(r_min, r_max, n_planes, unknown_opaque, union)
        self._chk(self._f["ground_view_gain"](self._h, _ptr(xy) if n else None, _ptr(nr) if nr is not None and n else None, n, C.byref(p),
                                              _ptr(out) if n else None))
        return out

    def ground_view_gain_dev(self, d_xy, d_normals, n, d_out, r_min=0.0, r_max=1.0, n_planes=0, unknown_opaque=False, union=False):
        """n views with points (n x 2 float32), normals (n x n_planes x 2 int32; 0 with n_planes == 0) and scores (n x 16 bytes) in
        DEVICE buffers (raw addresses), on the mapper's stream."""
        p = self.ground_view_param(r_min, r_max, n_planes, unknown_opaque, union)
        self._chk(self._f["ground_view_gain_dev"](self._h, C.c_void_p(d_xy or None), C.c_void_p(d_normals or None), int(n), C.byref(p), C.c_void_p(d_out or None)))

    def ground_view_mask(self, xy, r_min=0.0, r_max=1.0, normals=None, n_planes=0, unknown_opaque=False, union=False):
        """One view: (mask uint8 [Y][X]: 0 not a candidate, 1 hidden, 2 visible; its VIEW_SCORE_DTYPE record) (synchronises)."""
        xy, nr = self._ground_view_arrays("ground_view_mask", xy, normals, int(n_planes))
        if len(xy) != 1:
            raise ValueError("ground_view_mask: one view")
        mask = np.zeros((self.size[1], self.size[0]), np.uint8)
        score = np.zeros(1, VIEW_SCORE_DTYPE)
        p = self.ground_view_param(r_min, r_max, n_planes, unknown_opaque, union)
        self._chk(self._f["ground_view_mask"](self._h, _ptr(xy), _ptr(nr) if nr is not None else None, C.byref(p), _ptr(mask), _ptr(score)))
        return mask, score[0]

    def ground_view_mask_dev(self, d_xy, d_normals, d_mask, d_score=0, r_min=0.0, r_max=1.0, n_planes=0, unknown_opaque=False, union=False):
        """The same with the point, the normals, the mask (X * Y bytes) and the score (16 bytes; 0 = not wanted) in DEVICE buffers
        (raw addresses), on the mapper's stream."""
        p = self.ground_view_param(r_min, r_max, n_planes, unknown_opaque, union)
        self._chk(self._f["ground_view_mask_dev"](self._h, C.c_void_p(d_xy or None), C.c_void_p(d_normals or None), C.byref(p), C.c_void_p(d_mask or None),
                                                  C.c_void_p(d_score or None)))

    # --- ground rollouts: batched trajectory scoring on the ground costmap (include/gie.h) ---
    def ground_rollout_param(self, clearance_sq=0, inflate_sq=0, unknown_traversable=False, nf1=False):
        """gie_ground_rollout_param: clearance_sq and inflate_sq in squared CELLS, compared with the ground field's dist_sq."""
        p = GroundRolloutParam()
        p.clearance_sq, p.inflate_sq = int(clearance_sq), int(inflate_sq)
        p.flags = (GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE if unknown_traversable else 0) | (GROUND_ROLLOUT_NF1 if nf1 else 0)
        return p

    def ground_rollouts(self, xy, clearance_sq=0, inflate_sq=0, unknown_traversable=False, nf1=False):
        """n trajectories of T poses (an (n, T, 2) float32 array, metres, world frame; a NaN tail ends a shorter one) over the current
        ground field, with `nf1` also over its navigation function -> GROUND_ROLLOUT_DTYPE [n] (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32))
        if xy.ndim != 3 or xy.shape[2] != 2:
            raise ValueError("ground_rollouts: an (n, T, 2) array")
        n, T = xy.shape[0], xy.shape[1]
        out = np.zeros(n, GROUND_ROLLOUT_DTYPE)
        p = self.ground_rollout_param(clearance_sq, inflate_sq, unknown_traversable, nf1)
        self._chk(self._f["ground_rollouts"](self._h, _ptr(xy) if n and T else None, n, T, C.byref(p), _ptr(out) if n else None))
        return out

    def ground_rollouts_dev(self, d_xy, n, T, d_out, clearance_sq=0, inflate_sq=0, unknown_traversable=False, nf1=False):
        """n trajectories with poses (n x T x 2 float32) and records (n x 48 bytes) in DEVICE buffers (raw addresses), on the mapper's
        stream."""
        p = self.ground_rollout_param(clearance_sq, inflate_sq, unknown_traversable, nf1)
        self._chk(self._f["ground_rollouts_dev"](self._h, C.c_void_p(d_xy or None), int(n), int(T), C.byref(p), C.c_void_p(d_out or None)))

    # --- ground signed distance: inside distances, bilinear queries, path clearance (include/gie.h) ---
    def read_ground_sdf(self, sdf=True, inside_dist_sq=True):
        """{"sdf": float32 (cell units), "inside_dist_sq": int32}, shaped [Y][X] like read_ground (synchronises)."""
        shape = (self.size[1], self.size[0])
        s = np.empty(shape, np.float32) if sdf else None
        d = np.empty(shape, np.int32) if inside_dist_sq else None
        self._chk(self._f["read_ground_sdf"](self._h, _ptr(s), _ptr(d)))
        return {k: v for k, v in (("sdf", s), ("inside_dist_sq", d)) if v is not None}

    def read_ground_sdf_dev(self, d_sdf, d_inside_dist_sq):
        """The same planes into device buffers (raw device addresses, 0 = not wanted), asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_sdf_dev"](self._h, C.c_void_p(d_sdf or None), C.c_void_p(d_inside_dist_sq or None)))

    def ground_query_sdf(self, xy, dist=True, grad=True, flags=True):
        """n points (metres, world frame) -> (dist [n] float32 metres, grad [n, 2] float32, flags [n] uint8), None for an output that
        is not wanted (synchronises)."""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n = xy.shape[0]
        d = np.empty(n, np.float32) if dist else None
        g = np.empty((n, 2), np.float32) if grad else None
        f = np.empty(n, np.uint8) if flags else None
        self._chk(self._f["ground_query_sdf"](self._h, _ptr(xy) if n else None, n, _ptr(d), _ptr(g), _ptr(f)))
        return d, g, f

    def ground_query_sdf_dev(self, d_xy, n, d_dist, d_grad, d_flags):
        """n queries with points (n x 2 float32) and results in DEVICE buffers (raw addresses, 0 = not wanted), on the mapper's stream."""
        self._chk(self._f["ground_query_sdf_dev"](self._h, C.c_void_p(d_xy or None), int(n), C.c_void_p(d_dist or None), C.c_void_p(d_grad or None),
                                                  C.c_void_p(d_flags or None)))

    def ground_sdf_rollout_param(self, margin=0.0):
        """gie_ground_sdf_rollout_param: margin in METRES, compared with the queries' dist."""
        p = GroundSdfRolloutParam()
        p.margin = float(margin)
        return p

    def ground_sdf_rollouts(self, xy, margin=0.0, dist=False, grad=False):
        """n trajectories of T points (an (n, T, 2) float32 array, metres, world frame; a NaN tail ends a shorter one) over the current
        ground field -> (GROUND_SDF_ROLLOUT_DTYPE [n], dist [n, T] float32 or None, grad [n, T, 2] float32 or None) (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32))
        if xy.ndim != 3 or xy.shape[2] != 2:
            raise ValueError("ground_sdf_rollouts: an (n, T, 2) array")
        n, T = xy.shape[0], xy.shape[1]
        out = np.zeros(n, GROUND_SDF_ROLLOUT_DTYPE)
        d = np.empty((n, T), np.float32) if dist else None
        g = np.empty((n, T, 2), np.float32) if grad else None
        p = self.ground_sdf_rollout_param(margin)
        self._chk(self._f["ground_sdf_rollouts"](self._h, _ptr(xy) if n and T else None, n, T, C.byref(p), _ptr(out) if n else None, _ptr(d), _ptr(g)))
        return out, d, g

    def ground_sdf_rollouts_dev(self, d_xy, n, T, d_out, d_dist=0, d_grad=0, margin=0.0):
        """n trajectories with points (n x T x 2 float32), records (n x 32 bytes) and the optional per-point outputs (0 = not wanted) in
        DEVICE buffers (raw addresses), on the mapper's stream."""
        p = self.ground_sdf_rollout_param(margin)
        self._chk(self._f["ground_sdf_rollouts_dev"](self._h, C.c_void_p(d_xy or None), int(n), int(T), C.byref(p), C.c_void_p(d_out or None),
                                                     C.c_void_p(d_dist or None), C.c_void_p(d_grad or None)))

    # --- ground footprints: oriented-rectangle pose checks on the ground costmap (include/gie.h) ---
    def ground_footprint_param(self, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, margin=False):
        """gie_ground_footprint_param: the extents and clearance_sq in squared CELLS."""
        p = GroundFootprintParam()
        p.front_sq, p.back_sq, p.side_sq, p.clearance_sq = int(front_sq), int(back_sq), int(side_sq), int(clearance_sq)
        p.flags = (GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE if unknown_traversable else 0) | (GROUND_FOOTPRINT_MARGIN if margin else 0)
        return p

    def ground_footprints(self, xy, heading, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, margin=False):
        """n trajectories of T poses (xy: an (n, T, 2) float32 array, metres, world frame; heading: (n, T, 2) int32 direction vectors; a
        NaN or zero-heading tail ends a shorter one), each pose an oriented rectangle of cells on the current ground field
        -> GROUND_FOOTPRINT_DTYPE [n] (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32))
        heading = np.ascontiguousarray(np.asarray(heading, dtype=np.int32))
        if xy.ndim != 3 or xy.shape[2] != 2 or heading.shape != xy.shape:
            raise ValueError("ground_footprints: two (n, T, 2) arrays")
        n, T = xy.shape[0], xy.shape[1]
        out = np.zeros(n, GROUND_FOOTPRINT_DTYPE)
        p = self.ground_footprint_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, margin)
        some = n and T
        self._chk(self._f["ground_footprints"](self._h, _ptr(xy) if some else None, _ptr(heading) if some else None, n, T, C.byref(p), _ptr(out) if n else None))
        return out

    def ground_footprints_dev(self, d_xy, d_heading, n, T, d_out, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, margin=False):
        """n trajectories with poses (n x T x 2 float32), headings (n x T x 2 int32) and records (n x 32 bytes) in DEVICE buffers (raw
        addresses), on the mapper's stream."""
        p = self.ground_footprint_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, margin)
        self._chk(self._f["ground_footprints_dev"](self._h, C.c_void_p(d_xy or None), C.c_void_p(d_heading or None), int(n), int(T), C.byref(p), C.c_void_p(d_out or None)))

    def ground_footprint_mask(self, xy, heading, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, margin=False):
        """The footprint of ONE pose (xy: 2 floats, heading: 2 ints) -> (mask uint8 [Y][X]: 0 / 1 footprint / 2 blocked footprint, its
        GROUND_FOOTPRINT_DTYPE record) (synchronises)."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(2))
        heading = np.ascontiguousarray(np.asarray(heading, dtype=np.int32).reshape(2))
        mask = np.empty((self.size[1], self.size[0]), np.uint8)
        rec = np.zeros(1, GROUND_FOOTPRINT_DTYPE)
        p = self.ground_footprint_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, margin)
        self._chk(self._f["ground_footprint_mask"](self._h, _ptr(xy), _ptr(heading), C.byref(p), _ptr(mask), _ptr(rec)))
        return mask, rec[0]

    def ground_footprint_mask_dev(self, d_xy, d_heading, d_mask, d_rec, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, margin=False):
        """One pose, its mask (X * Y bytes) and its record (32 bytes, or 0) in DEVICE buffers (raw addresses), on the mapper's stream."""
        p = self.ground_footprint_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, margin)
        self._chk(self._f["ground_footprint_mask_dev"](self._h, C.c_void_p(d_xy or None), C.c_void_p(d_heading or None), C.byref(p), C.c_void_p(d_mask or None),
                                                       C.c_void_p(d_rec or None)))

    # --- ground pose navigation function: NF1 over (cell, heading) states of an oriented rectangle (include/gie.h) ---
    def ground_pose_nf1_param(self, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, from_frontiers=False, reverse=False):
        """gie_ground_pose_nf1_param: the extents and clearance_sq in squared CELLS."""
        p = GroundPoseNf1Param()
        p.front_sq, p.back_sq, p.side_sq, p.clearance_sq = int(front_sq), int(back_sq), int(side_sq), int(clearance_sq)
        p.flags = ((GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE if unknown_traversable else 0) | (GROUND_POSE_NF1_FROM_FRONTIERS if from_frontiers else 0) |
                   (GROUND_POSE_NF1_REVERSE if reverse else 0))
        return p

    @staticmethod
    def _pose_arrays(who, xy, k):
        xy = np.ascontiguousarray(np.asarray(xy if xy is not None else [], dtype=np.float32).reshape(-1, 2))
        if k is not None:
            k = np.ascontiguousarray(np.asarray(k, dtype=np.int32).reshape(-1))
            if len(k) != len(xy):
                raise ValueError(who + ": one heading index per point")
        return xy, k

    def ground_pose_nf1_compute(self, goals, goal_k, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False, from_frontiers=False,
                                reverse=False):
        """The pose navigation function of the current ground field from n goals (n x 2 metres, world frame; goal_k: n heading
        indices 0..7, -1 = all eight, or None) -> [source states, free states] (synchronises)."""
        xy, k = self._pose_arrays("ground_pose_nf1_compute", goals, goal_k)
        n = len(xy)
        counts = np.zeros(2, np.int32)
        p = self.ground_pose_nf1_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, from_frontiers, reverse)
        self._chk(self._f["ground_pose_nf1_compute"](self._h, _ptr(xy) if n else None, _ptr(k) if k is not None and n else None, n, C.byref(p), _ptr(counts)))
        return [int(counts[0]), int(counts[1])]

    def ground_pose_nf1_compute_dev(self, d_goals, d_goal_k, n, d_counts, front_sq, back_sq, side_sq, clearance_sq=0, unknown_traversable=False,
                                    from_frontiers=False, reverse=False):
        """The same with the goals (n x 2 float32), their heading indices (n int32; 0 = all eight) and the counts (2 int32; 0 = not
        wanted) in DEVICE buffers (raw addresses), on the mapper's stream; the host does not wait."""
        p = self.ground_pose_nf1_param(front_sq, back_sq, side_sq, clearance_sq, unknown_traversable, from_frontiers, reverse)
        self._chk(self._f["ground_pose_nf1_compute_dev"](self._h, C.c_void_p(d_goals or None), C.c_void_p(d_goal_k or None), int(n), C.byref(p),
                                                         C.c_void_p(d_counts or None)))

    def read_ground_pose_nf1(self):
        """(pnf1 int32 [8][Y][X], cspace uint8 [Y][X]: bit k set iff (cell, k) is not free) (synchronises)."""
        f = np.empty((GROUND_POSE_HEADINGS, self.size[1], self.size[0]), np.int32)
        cs = np.empty((self.size[1], self.size[0]), np.uint8)
        self._chk(self._f["read_ground_pose_nf1"](self._h, _ptr(f), _ptr(cs)))
        return f, cs

    def read_ground_pose_nf1_dev(self, d_pnf1, d_cspace):
        """The field (8 * X * Y int32) and the C-space bytes (X * Y) into DEVICE buffers (raw addresses; 0 = not wanted, not both),
        asynchronous on the mapper's stream."""
        self._chk(self._f["read_ground_pose_nf1_dev"](self._h, C.c_void_p(d_pnf1 or None), C.c_void_p(d_cspace or None)))

    def ground_pose_nf1_query(self, xy, k=None):
        """The current pose navigation function at n states (xy: n x 2 metres; k: n heading indices, -1 = the least over the eight,
        None = -1 for all): int32 [n] moves, -1 where there is none (synchronises)."""
        xy, k = self._pose_arrays("ground_pose_nf1_query", xy, k)
        n = len(xy)
        out = np.zeros(n, np.int32)
        self._chk(self._f["ground_pose_nf1_query"](self._h, _ptr(xy) if n else None, _ptr(k) if k is not None and n else None, n, _ptr(out) if n else None))
        return out

    def ground_pose_nf1_query_dev(self, d_xy, d_k, n, d_steps):
        """n points (n x 2 float32), their heading indices (n int32, or 0) and the moves (n int32) in DEVICE buffers, on the mapper's stream."""
        self._chk(self._f["ground_pose_nf1_query_dev"](self._h, C.c_void_p(d_xy or None), C.c_void_p(d_k or None), int(n), C.c_void_p(d_steps or None)))

    def ground_pose_nf1_path(self, starts, start_k, max_len, fill=0):
        """Descents from n start states -> (path int32 [n][max_len][3] GLOBAL x, y and heading index, len int32 [n]); triples beyond
        min(len, max_len) keep `fill` (synchronises)."""
        xy, k = self._pose_arrays("ground_pose_nf1_path", starts, start_k)
        n = len(xy)
        path = np.full((n, int(max_len), 3), fill, np.int32)
        ln = np.zeros(n, np.int32)
        self._chk(self._f["ground_pose_nf1_path"](self._h, _ptr(xy) if n else None, _ptr(k) if k is not None and n else None, n, int(max_len),
                                                  _ptr(path) if n else None, _ptr(ln) if n else None))
        return path, ln

    def ground_pose_nf1_path_dev(self, d_starts, d_start_k, n, max_len, d_path, d_len):
        """n starts (n x 2 float32), their heading indices (n int32, or 0), the triples (n x max_len x 3 int32) and the lengths (n
        int32) in DEVICE buffers (raw addresses), on the mapper's stream."""
        self._chk(self._f["ground_pose_nf1_path_dev"](self._h, C.c_void_p(d_starts or None), C.c_void_p(d_start_k or None), int(n), int(max_len),
                                                      C.c_void_p(d_path or None), C.c_void_p(d_len or None)))

    def read_costmap_ground_nf1(self):
        """The one-layer TYPE_NF1 CostMap of the ground navigation function: (SeenDist payload [Y][X], header) (synchronises)."""
        pay = np.empty((self.size[1], self.size[0]), SEENDIST_DTYPE)
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_ground_nf1"](self._h, _ptr(pay), C.byref(hdr)))
        return pay, hdr

    def read_costmap_ground_nf1_dev(self, dptr):
        """That payload into a device buffer (raw address), asynchronous on the mapper's stream; returns the header."""
        hdr = CostMapHdr()
        self._chk(self._f["read_costmap_ground_nf1_dev"](self._h, C.c_void_p(dptr or None), C.byref(hdr)))
        return hdr

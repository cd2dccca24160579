"""Shared parity driver: runs the same seeded multi-frame scenario through two mappers that speak
the C-ABI of include/gie.h (the CPU oracle and either the HIP library or the test-only host
emulation) and compares every stage bit for bit."""
import numpy as np

import gie
import stream_mirror
from gie import scenes


class Scenario:
    def __init__(self, name, size, voxel=0.1, sensor="depth", frames=6, delta_vox=5, yaw_deg=40.0, seed=2,
                 cutoff_dist=2.0, fast_mode=False, n_boxes=30, extent=(4.0, 4.0, 1.5), for_motion_planner=False,
                 img=(120, 160, 130.0), toggle=0.25, lidar_az=360, ext_boxes=False, min_h=-1000.0, max_h=1000.0,
                 max_depth=6.0, p_occ=0.01, retain=0, max_blocks=0, probe_margin=12, turn=0, steps=None, base_vox=(0, 0, 0)):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def shift(self):
        """base_vox in metres: what every pose of the drive is moved by (exact in float32 where the voxel width is a power of two)"""
        return tuple(int(b) * float(self.voxel) for b in self.base_vox)

    def _shifted(self, pos):
        # the scene is made at the unshifted pose (sensor data are in the sensor frame, a label plane is the hash world at the unshifted
        # pivot); only the pose the mappers are given moves: the run is the translation twin of the one at base_vox = (0, 0, 0)
        if not any(self.base_vox):
            return pos
        return tuple(np.float32(float(pos[i]) + d) for i, d in enumerate(self.shift()))

    def config(self):
        return gie.make_config(self.voxel, self.size, cutoff_dist=self.cutoff_dist, fast_mode=self.fast_mode,
                               for_motion_planner=self.for_motion_planner, ogm_min_h=self.min_h, ogm_max_h=self.max_h,
                               retain_radius_blocks=self.retain, max_blocks=self.max_blocks)

    def frames_iter(self):
        for pos, q, kind, data, kw in self._frames_unshifted():
            yield self._shifted(pos), q, kind, data, kw

    def _frames_unshifted(self):
        world = scenes.BoxWorld(self.seed, extent=self.extent, n_boxes=self.n_boxes, toggle_frac=self.toggle)
        rows, cols, f = self.img
        cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
        for k in range(self.frames):
            kp = k if not self.turn else (k % (2 * self.turn) if k % (2 * self.turn) <= self.turn else 2 * self.turn - k % (2 * self.turn))
            pos, q = scenes.pose(kp, self.voxel, delta_vox=self.delta_vox, yaw_deg=self.yaw_deg)     # turn > 0: out and back
            if self.steps is not None:
                # a drive given step by step: frame k stands at the sum of the first k displacements (voxels, any axis, any sign)
                at = np.sum(np.asarray(self.steps[:k], np.int64).reshape(-1, 3), axis=0)
                pos = tuple(np.float32(int(at[i]) * self.voxel) for i in range(3))
            kind = self.sensor
            if kind == "mixed":
                kind = ("depth", "pointcloud", "multiscan")[k % 3]
            if kind in ("depth", "pointcloud"):
                depth = scenes.depth_frame(world, k, pos, q, rows=rows, cols=cols, fx=f, fy=f, cx=cx, cy=cy,
                                           max_depth=self.max_depth)
                if kind == "depth":
                    yield pos, q, "depth", depth, dict(cx=cx, cy=cy, fx=f, fy=f, valid_nan=True)
                else:
                    yield pos, q, "pointcloud", scenes.depth_to_points(depth, f, f, cx, cy), {}
            elif kind == "lidar_points":
                pts, _ = scenes.lidar_frame(world, k, pos, q, az=self.lidar_az, max_range=30.0)
                yield pos, q, "pointcloud", pts, {}
            elif kind == "multiscan":
                pts, _ = scenes.lidar_frame(world, k, pos, q, az=self.lidar_az * 4, max_range=30.0)
                img = scenes.range_image(pts)
                yield pos, q, "multiscan", img, dict(theta_inc=2.0 * np.pi / 440, theta_min=-np.pi,
                                                     phi_inc=np.radians(2.0), phi_min=np.radians(-15.0))
            elif kind == "labels":
                # BASELINE config 5's sensor-less world: occupancy from a hash of the global voxel, full observation
                pvt = scenes.local_pivot(pos, self.voxel, self.size, getattr(self, "tile_off", (0, 0, 0)))
                yield pos, q, "labels", scenes.hash_world_labels(pvt, self.size, k, seed=self.seed, p_occ=self.p_occ,
                                                                 toggle_frac=self.toggle).astype(np.int8), {}
            elif kind == "labels_blink":
                # the hash world with every third scan free of obstacles altogether: in those map updates the batch EDT has nothing
                # (pairs EMPTY, nothing committed) except where limited observation keeps an old obstacle outside the volume
                pvt = scenes.local_pivot(pos, self.voxel, self.size)
                lab = scenes.hash_world_labels(pvt, self.size, k, seed=self.seed, p_occ=self.p_occ, toggle_frac=self.toggle).astype(np.int8)
                if k % 3 == 2:
                    lab[:] = 1
                yield pos, q, "labels", lab, {}
            elif kind == "scan2d":
                pts, rng = scenes.lidar_frame(world, k, pos, q, rings=1, az=360, phi_min_deg=0.0, max_range=30.0)
                r = np.where(np.isfinite(rng[0]), rng[0], np.nan).astype(np.float32)
                yield pos, q, "scan2d", r, dict(theta_inc=2.0 * np.pi / 360, theta_min=-np.pi + np.pi / 360)
            else:
                raise ValueError(kind)


# Drives that change speed and direction in volumes whose sides are no multiples of 8 (round 6): slow updates leave
# tiles flagged 2 ("deferred records") next to the partial tile of a face, then a jump of 6-9 voxels puts a NEW tile across the old
# volume's face — it reaches past the old face tile into such a tile, whose records gie_tile_oldskip used not to catch up.  The
# first is the advisor's reproduction, the second a find of the same search on the unfixed sources; both fail there.
UNEVEN_DRIVES = [
    Scenario("uneven_drive_40x29x40", (40, 29, 40), sensor="labels", seed=893, p_occ=0.03, toggle=0.5, frames=4,
             steps=[(1, 0, -1), (-1, 0, 0), (-8, 7, -4)]),
    Scenario("uneven_drive_21x21x43", (21, 21, 43), voxel=0.05, sensor="labels", seed=245, p_occ=0.03, toggle=0.5, frames=7, cutoff_dist=1.0,
             steps=[(-1, -1, 0), (0, 0, -1), (-8, 7, -9), (9, 8, -9), (0, 1, -6), (-8, 6, 1)]),
    Scenario("uneven_drive_lidar_37x29x35", (37, 29, 35), sensor="mixed", seed=11, frames=8, extent=(3.2, 3.2, 1.9),
             steps=[(1, 0, 0), (0, 1, 0), (7, -6, 0), (0, 0, 1), (-1, 1, 0), (-9, 8, 6), (1, 0, -1)]),
]


# A fuse WITHOUT a merge, then a jump (round 6): the tiles the abandoned fuse flagged 1 — "the sweep will store them" — still held
# voxels whose records the merge before had left to its pair plane, and only the tiles flagged 2 were caught up; found while the
# lazy pairs were built (the unfixed sources fail frame 4: 95 voxels near a corner of the volume keep a stale closest obstacle).
FUSE_ONLY_THEN_JUMP = Scenario("fuse_only_then_jump", (64, 64, 64), voxel=0.05, sensor="labels", seed=5, p_occ=0.01, toggle=0.25, frames=7, cutoff_dist=1.0,
                               steps=[(1, 0, 0), (2, 1, 0), (1, 0, -1), (9, -7, 6), (1, 1, 1), (0, 0, 1)])


def _feed(m, kind, data, kw):
    if kind == "depth":
        m.ogm_depth(data, **kw)
    elif kind == "pointcloud":
        m.ogm_pointcloud(data)
    elif kind == "multiscan":
        m.ogm_multiscan(data, **kw)
    elif kind == "scan2d":
        m.ogm_scan2d(data, **kw)
    elif kind == "labels":
        m.ogm_labels(data)


def probe_coords(pvt, size, rng, n=4000, margin=12):
    """Global voxels in and around the local volume (margin 12 voxels)."""
    lo = np.array(pvt) - margin
    hi = np.array(pvt) + np.array(size) + margin
    return rng.integers(lo, hi, size=(n, 3)).astype(np.int32)


def probe_left_behind(prev_pvt, pvt, size, rng, n=6000):
    """Global voxels of the volume at `prev_pvt` that the volume at `pvt` no longer holds (the slabs the robot has just left: their
    records were the pair plane's until the voxels left — gie_ops.h "deferred records").  Drawn slab by slab (the part of the old
    box beyond the new one on each axis), so a slow drive gets its n probes too; empty when the volume did not move."""
    lo, sz, new = np.array(prev_pvt, np.int64), np.array(size, np.int64), np.array(pvt, np.int64)
    out = []
    for ax in range(3):
        d = int(new[ax] - lo[ax])
        if d == 0:
            continue
        w = min(abs(d), int(sz[ax]))
        a0 = lo[ax] if d > 0 else lo[ax] + sz[ax] - w          # the old box's layers the new box has left behind on this axis
        xyz = rng.integers(lo, lo + sz, size=(n, 3))
        xyz[:, ax] = rng.integers(a0, a0 + w, size=n)
        out.append(xyz)
    if not out:
        return np.zeros((0, 3), np.int32)
    xyz = np.concatenate(out)
    gone = ((xyz < new) | (xyz >= new + sz)).any(-1)
    assert gone.all()
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))[:n]], dtype=np.int32)


def set_ext_boxes(*mappers, shift=(0.0, 0.0, 0.0)):
    """the two boxes of the scenarios with ext_boxes=True (one of them inactive), moved by `shift` metres"""
    ll = (np.array([[-100, -100, -100], [0.5, -1.0, -1.0]], np.float64) + np.asarray(shift, np.float64)).astype(np.float32)
    ur = (np.array([[100, 100, 100], [1.0, 1.0, 0.5]], np.float64) + np.asarray(shift, np.float64)).astype(np.float32)
    act = np.array([0, 1], np.uint8)
    for m in mappers:
        m.set_ext_boxes(ll, ur, act)


def compare_global(tag, a, b, xyz):
    if len(xyz) == 0:
        return
    ga, gb = a.query_global(xyz), b.query_global(xyz)
    for key in ("occ_val", "vox_type", "dist_sq", "coc"):
        assert np.array_equal(ga[key], gb[key]), "%s: global %s differs in %d of %d probes" % (
            tag, key, int((ga[key] != gb[key]).reshape(len(xyz), -1).any(-1).sum()), len(xyz))


def _compare_after_merge(sc, k, a, b, rng, check_stats):
    ra, rb = a.read_local(), b.read_local()
    for key in ("type", "dist_sq", "coc"):
        assert np.array_equal(ra[key], rb[key]), "%s frame %d: post-merge %s differs in %d voxels" % (
            sc.name, k, key, int((ra[key] != rb[key]).reshape(ra["type"].shape + (-1,)).any(-1).sum()))
    assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0.0), "%s frame %d: edt differs" % (sc.name, k)
    xyz = probe_coords(a.pivot(), sc.size, rng, margin=sc.probe_margin)
    ga, gb = a.query_global(xyz), b.query_global(xyz)
    for key in ("occ_val", "vox_type", "dist_sq", "coc"):
        assert np.array_equal(ga[key], gb[key]), "%s frame %d: global %s differs in %d probes" % (
            sc.name, k, key, int((ga[key] != gb[key]).reshape(len(xyz), -1).any(-1).sum()))
    sa, sb = a.stats(), b.stats()
    if check_stats:
        for key in ("seeds_a", "seeds_b", "seeds_c", "levels_a", "levels_b", "levels_c", "visits_a", "visits_b", "visits_c", "blocks_total"):
            assert sa[key] == sb[key], "%s frame %d: stat %s %d != %d" % (sc.name, k, key, sa[key], sb[key])


def run_and_compare(sc, make_a, make_b, check_stats=True, verbose=False, production=False, before_frame=None, after_frame=None):
    """make_a: reference mapper factory (oracle); make_b: mapper under test. Raises on mismatch.
    Returns a list of per-frame stats dicts of the reference mapper.
    production=True drives both mappers with set_pose / ogm / step() only — the sequence a node runs — and compares
    what is left after the map update.  (The stage-by-stage form reads the scan and the batch EDT in between, and
    those readers complete what the update itself leaves out: scan labels of a ray-cast scan, pass Z of tiles nobody
    reads.)  before_frame(k, a, b), if given, runs ahead of frame k's set_pose (tests that set the frame counter: debug_set_frame),
    after_frame(k, a, b) when frame k has been compared."""
    cfg = sc.config()
    a, b = make_a(cfg), make_b(cfg)
    rng = np.random.default_rng(sc.seed + 77)
    out = []
    try:
        if sc.ext_boxes:
            set_ext_boxes(a, b, shift=sc.shift())
        for k, (pos, q, kind, data, kw) in enumerate(sc.frames_iter()):
            if before_frame is not None:
                before_frame(k, a, b)
            a.set_pose(pos, q)
            b.set_pose(pos, q)
            assert a.pivot() == b.pivot()
            _feed(a, kind, data, kw)
            _feed(b, kind, data, kw)
            if production:
                a.step()
                b.step()
                _compare_after_merge(sc, k, a, b, rng, check_stats)
                out.append(a.stats())
                if after_frame is not None:
                    after_frame(k, a, b)
                continue
            oa, ob = a.read_ogm(), b.read_ogm()
            for key in ("inst_type", "ray_count"):
                bad = int((oa[key] != ob[key]).sum())
                assert bad == 0, "%s frame %d: OGM %s differs in %d voxels" % (sc.name, k, key, bad)
            a.fuse()
            b.fuse()
            ta, tb = a.read_local(edt=False, dist_sq=False, coc=False)["type"], b.read_local(edt=False, dist_sq=False, coc=False)["type"]
            assert np.array_equal(ta, tb), "%s frame %d: fused types differ in %d voxels" % (sc.name, k, int((ta != tb).sum()))
            a.batch_edt()
            b.batch_edt()
            ea, eb = a.read_batch_edt(), b.read_batch_edt()
            assert np.array_equal(ea["dist_sq"], eb["dist_sq"]), "%s frame %d: batch EDT dist differs in %d voxels" % (
                sc.name, k, int((ea["dist_sq"] != eb["dist_sq"]).sum()))
            assert np.array_equal(ea["coc"], eb["coc"]), "%s frame %d: batch EDT coc differs in %d voxels" % (
                sc.name, k, int((ea["coc"] != eb["coc"]).any(-1).sum()))
            a.merge()
            b.merge()
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), "%s frame %d: post-merge %s differs in %d voxels" % (
                    sc.name, k, key, int((ra[key] != rb[key]).reshape(ra["type"].shape + (-1,)).any(-1).sum()))
            # float distance: sqrtf of an int, tolerance 1e-6 relative (north_star)
            assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0.0), "%s frame %d: edt differs" % (sc.name, k)
            xyz = probe_coords(a.pivot(), sc.size, rng, margin=sc.probe_margin)
            ga, gb = a.query_global(xyz), b.query_global(xyz)
            for key in ("occ_val", "vox_type", "dist_sq", "coc"):
                assert np.array_equal(ga[key], gb[key]), "%s frame %d: global %s differs in %d probes" % (
                    sc.name, k, key, int((ga[key] != gb[key]).reshape(len(xyz), -1).any(-1).sum()))
            sa, sb = a.stats(), b.stats()
            if check_stats:
                for key in ("seeds_a", "seeds_b", "seeds_c", "levels_a", "levels_b", "levels_c", "visits_a", "visits_b", "visits_c",
                            "blocks_total"):
                    assert sa[key] == sb[key], "%s frame %d: stat %s %d != %d" % (sc.name, k, key, sa[key], sb[key])
            if hasattr(b, "debug_nbr_check"):       # test builds (emulation, -DGIE_TEST_HOOKS): the neighbour table of waves A / B against the hash
                bad = b.debug_nbr_check()
                assert bad == 0, "%s frame %d: %d rows of the neighbour table disagree with the hash" % (sc.name, k, bad)
            if verbose:
                print(sc.name, k, {kk: sa[kk] for kk in ("seeds_a", "seeds_b", "seeds_c", "visits_a", "visits_b",
                                                         "visits_c", "levels_a", "levels_b", "levels_c")},
                      "known", int((ra["type"] != 0).sum()))
            out.append(sa)
            if after_frame is not None:
                after_frame(k, a, b)
    finally:
        a.close()
        b.close()
    return out


def run_irregular(sc, make_a, make_b, fuse_only=(), stream_on=(), compare_margin=None, before_frame=None, after_frame=None):
    """The staged ABI driven off the beaten path: map updates that stop after gie_fuse (`fuse_only`: frame numbers
    without batch EDT and merge -- a node that skips the EDT of a frame, or an update that failed half way) and updates that run
    with the changed-block flags on (`stream_on`: frame numbers; the mapper then uses the reference's order Mark ... commit instead
    of the fused sweep, so the run changes between the two forms).  After every COMPLETE update everything is compared as in
    run_and_compare, and what the two mappers deliver of a stream-on update; after a fuse-only update the fused types and the stored
    occupancy.  before_frame(k, a, b), after_frame(k, a, b): as in run_and_compare (after complete updates only)."""
    cfg = sc.config()
    a, b = make_a(cfg), make_b(cfg)
    rng = np.random.default_rng(sc.seed + 78)
    margin = sc.probe_margin if compare_margin is None else compare_margin
    try:
        for k, (pos, q, kind, data, kw) in enumerate(sc.frames_iter()):
            on = k in stream_on
            if before_frame is not None:
                before_frame(k, a, b)
            for m in (a, b):
                m.stream_enable(on)
                m.set_pose(pos, q)
                _feed(m, kind, data, kw)
                m.fuse()
            if k in fuse_only:
                ta, tb = a.read_local(edt=False, dist_sq=False, coc=False)["type"], b.read_local(edt=False, dist_sq=False, coc=False)["type"]
                assert np.array_equal(ta, tb), "%s frame %d (fuse only): fused types differ" % (sc.name, k)
                xyz = probe_coords(a.pivot(), sc.size, rng, margin=margin)
                ga, gb = a.query_global(xyz), b.query_global(xyz)
                for key in ("occ_val", "vox_type", "dist_sq", "coc"):
                    assert np.array_equal(ga[key], gb[key]), "%s frame %d (fuse only): global %s differs in %d probes" % (
                        sc.name, k, key, int((ga[key] != gb[key]).reshape(len(xyz), -1).any(-1).sum()))
                continue
            for m in (a, b):
                m.batch_edt(); m.merge()
            if on:                                           # drain the flags: both mappers deliver the same blocks (stream_mirror I1)
                ka, ba, _ = a.stream_changed()
                kb, bb, _ = b.stream_changed()
                stream_mirror.check_oracle_equal("%s frame %d" % (sc.name, k), (kb, bb), (ka, ba))
            _compare_after_merge(sc, k, a, b, rng, True)
            if after_frame is not None:
                after_frame(k, a, b)
    finally:
        a.close()
        b.close()

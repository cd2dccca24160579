"""The two limits gie_set_pose states (include/gie.h), driven up to: poses out to +-900000 voxels per axis, and the frame counter
through a multiple of 2^18, where the 18-bit stamps of the wave planes start again and gie_set_pose clears both planes.

Every parity test has a CPU form (the oracle against the host emulation of the device logic) and a GPU form (the oracle against
the HIP library).  Voxel widths are powers of two, so poses, pivots and the exact test points are float32 numbers without
rounding out to 900000 voxels, and a labels drive moved by `base_vox` (parity.Scenario) sees the same world in the same local
voxels as the drive it was moved from: its translation twin (see "translation twin" below for what has to be a multiple of 16).

What base (iii) guards on the device: the block kernels of waves A and B keep one validity flag per voxel in LDS, computed when a
block is loaded, where the reference reads a neighbour's stored obstacle whenever it looks at it.  A voxel whose obstacle changes
sides of 900000 within a block-run (raised by obtainFrontiers to an obstacle inside the volume and lowered to a valid one by wave
A; committed by wave B to an obstacle above 900000) has to change its flag with it.  The loop drive below gives these kernels
hundreds of visits per update at that base, compared by arrays and statistics.

The bases, per axis, of a drive whose poses span [lo, hi] voxels about its start:
  (i)   "neg":   the all-negative corner, lowest pose at -900000 + 3;
  (ii)  "pos":   highest pose at 900000 - ceil(size / 2) - 16: the volume, the blocks round it and the probes' margin stay
                 at or below 900000, where the reference's invalid-obstacle rule (coordinate > 900000, one-sided) cannot fire;
  (iii) "edge":  highest pose at exactly +900000: half the volume lies above the rule.  The labels drive is mirrored in x and z
                 for this base so that it ENDS there on every axis (a pose beyond 900000 is refused, so a drive can only end
                 on the limit on an axis whose last pose is its highest).
"""
import functools

import numpy as np
import pytest

import gie
import parity
from emu_py import EmuMapper
from oracle_py import OracleMapper
from gie import scenes

W = 0.125
LIM = 900000
EMPTY_KEY = 999999                        # closest obstacle of a record that has none (voxmap_utils.cuh:8-9)
HIGH = dict(min_h=-2.0e5, max_h=2.0e5)    # 900000 voxels of 0.125 m are 112.5 km up: the default +-1000 m band would drop every obstacle


def _hip():
    return gie.Mapper


def _hooks():
    from hooks_py import HooksMapper
    return HooksMapper


def drive_vox(kw):
    """the voxel the pose of every frame stands on, about the drive's start: [frames, 3]"""
    n = kw["frames"]
    if kw.get("steps") is not None:
        return np.array([np.sum(np.asarray(kw["steps"][:k], np.int64).reshape(-1, 3), axis=0) for k in range(n)])
    return np.array([(k * kw.get("delta_vox", 5), 0, 0) for k in range(n)], np.int64)


def base_of(kw, which):
    at = drive_vox(kw)
    lo, hi, half = at.min(0), at.max(0), (np.array(kw["size"]) + 1) // 2
    if which == "origin":
        return (0, 0, 0)
    if which == "neg":
        return tuple(int(v) for v in (-LIM + 3 - lo))
    if which == "pos":
        return tuple(int(v) for v in (LIM - half - 16 - hi))
    assert which == "edge"
    return tuple(int(v) for v in (LIM - hi))


def scene(kw, which, **more):
    kw = dict(kw, **more)
    if which == "edge" and "steps_edge" in kw:
        kw["steps"] = kw["steps_edge"]
    kw.pop("steps_edge", None)
    return parity.Scenario(base_vox=base_of(kw, which), **dict(kw, name="%s_%s" % (kw["name"], which)))


_U0 = parity.UNEVEN_DRIVES[0]
LABELS = dict(name="far_labels", size=_U0.size, voxel=W, sensor="labels", seed=_U0.seed, p_occ=_U0.p_occ, toggle=_U0.toggle, frames=_U0.frames,
              steps=_U0.steps, steps_edge=[(-s[0], s[1], -s[2]) for s in _U0.steps])
_FJ = parity.FUSE_ONLY_THEN_JUMP
FUSE_JUMP = dict(name="far_fuse_only_then_jump", size=(48, 40, 24), voxel=0.0625, sensor="labels", seed=_FJ.seed, p_occ=_FJ.p_occ, toggle=_FJ.toggle,
                 frames=_FJ.frames, cutoff_dist=1.0, steps=_FJ.steps)
MIXED = dict(name="far_mixed", size=(48, 40, 24), voxel=W, sensor="mixed", frames=6, delta_vox=3, yaw_deg=47.0, **HIGH)
LIDAR = dict(name="far_lidar_points", size=(40, 29, 40), voxel=W, sensor="lidar_points", frames=5, delta_vox=4, yaw_deg=31.0, **HIGH)
SCAN2D = dict(name="far_scan2d", size=(21, 21, 43), voxel=W, sensor="scan2d", frames=5, delta_vox=2, yaw_deg=10.0, extent=(1.5, 1.5, 1.5), n_boxes=40, **HIGH)
RETAIN = dict(name="far_retain", size=(21, 21, 43), voxel=0.0625, sensor="labels", seed=7, p_occ=0.02, toggle=0.5, frames=8, delta_vox=8, cutoff_dist=1.0,
              retain=1, probe_margin=40)
FAST = dict(LABELS, name="far_fast_mode", fast_mode=True)
BOXES = dict(name="far_ext_boxes", size=(48, 40, 24), voxel=W, sensor="mixed", frames=5, delta_vox=4, yaw_deg=30.0, for_motion_planner=True, ext_boxes=True)

BASES = ("neg", "pos", "edge")
DRIVEN = [LABELS, FUSE_JUMP, MIXED, LIDAR, SCAN2D]
VARIANTS = [(RETAIN, "neg"), (RETAIN, "edge"), (FAST, "edge"), (BOXES, "neg"), (BOXES, "edge")]


def _boxes_scene(which):
    # the height band of the planner configuration is a world height: it moves with the base like the boxes do
    b = base_of(BOXES, which)
    return scene(BOXES, which, min_h=-0.8 + b[2] * W, max_h=1.0 + b[2] * W)


def _far_parity(kw, which, make):
    """stage by stage and as a node drives it; the scene has to hold obstacles, or it tests nothing"""
    sc = _boxes_scene(which) if kw is BOXES else scene(kw, which)
    seen = []

    def count(k, a, b):
        seen.append(int((a.read_local(edt=False, dist_sq=False, coc=False)["type"] == 2).sum()))
    parity.run_and_compare(sc, OracleMapper, make, after_frame=count)
    assert min(seen[1:]) > 0, (sc.name, seen)
    parity.run_and_compare(sc, OracleMapper, make, production=True)


_ids = lambda cases: ["%s-%s" % (kw["name"], which) for kw, which in cases]      # noqa: E731
FAR_CASES = [(kw, which) for kw in DRIVEN for which in BASES] + VARIANTS


@pytest.mark.parametrize("kw,which", FAR_CASES, ids=_ids(FAR_CASES))
def test_far_pose_parity_emulation(oracle_lib, kw, which):
    _far_parity(kw, which, EmuMapper)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,which", FAR_CASES, ids=_ids(FAR_CASES))
def test_far_pose_parity(oracle_lib, kw, which):
    _far_parity(kw, which, _hip())


# the staged ABI off the beaten path: updates with the changed-block flags on, and a fuse without a merge right before the jump
IRREGULAR = [(LABELS, (), (1, 3)), (FUSE_JUMP, (3,), ()), (FUSE_JUMP, (3,), (5,)), (FUSE_JUMP, (2, 3), ())]
_irr = [(kw, which, f, s) for kw, f, s in IRREGULAR for which in BASES]
_irr_ids = ["%s-%s-f%s-s%s" % (kw["name"], which, "_".join(map(str, f)), "_".join(map(str, s))) for kw, which, f, s in _irr]


@pytest.mark.parametrize("kw,which,fuse_only,stream_on", _irr, ids=_irr_ids)
def test_far_pose_irregular_call_orders_emulation(oracle_lib, kw, which, fuse_only, stream_on):
    parity.run_irregular(scene(kw, which), OracleMapper, EmuMapper, fuse_only=set(fuse_only), stream_on=set(stream_on))


@pytest.mark.gpu
@pytest.mark.parametrize("kw,which,fuse_only,stream_on", _irr, ids=_irr_ids)
def test_far_pose_irregular_call_orders(oracle_lib, kw, which, fuse_only, stream_on):
    parity.run_irregular(scene(kw, which), OracleMapper, _hip(), fuse_only=set(fuse_only), stream_on=set(stream_on))


# ---- the second statement of the merge (tests/merge_checker.py) follows the labels drives themselves
# Its schedule is another one, and the records the two schedules leave outside the volume may differ (both witnesses; bounded
# below as in test_merge_second_opinion.py).  These scenes are dense enough for such a record to sit right next to the volume,
# where it moves a face voxel of the next update from one wave's seeds to another's: the seed counts are compared within the
# number of differing records (run_scene, equal_seeds=False), everything else by test_merge_second_opinion.py's bounds.
def _second_opinion(kw, which, make, before_frame=None):
    from test_merge_second_opinion import run_scene
    st = run_scene(scene(kw, which), make, before_frame=before_frame, equal_seeds=False)
    assert st["voxels"] > 0 and min(st["waves"]) > 0, st
    assert st["inside_diff"] <= 5e-4 * st["voxels"], st
    assert st["outside_diff"] <= 0.006 * max(1, st["outside_cmp"]), st
    assert st.get("outside_max", 0.0) <= 3.0, st
    return st


@pytest.mark.parametrize("which", BASES)
def test_far_pose_second_statement_oracle(oracle_lib, which):
    _second_opinion(LABELS, which, OracleMapper)


@pytest.mark.gpu
@pytest.mark.parametrize("which", BASES)
def test_far_pose_second_statement(which):
    _second_opinion(LABELS, which, _hip())


# ---- translation twin: the same drive next to the origin
# The global map is kept in blocks of 8 x 8 x 8 voxels on a fixed lattice: which blocks a volume touches (statistics, what a lookup
# outside them answers) goes by the pivot modulo 8, and the canonical schedule of waves A and B colours the blocks by the parity
# of bx + by + bz and begins with colour 0, which decides the round counts, the visits and which of two equally near
# obstacles a voxel outside the volume keeps.  The twin of a drive at `base` is therefore the drive at base mod 16, a few voxels
# from the origin: the two are an even number of blocks apart on every axis, and then every record and statistic is the same.
def _record(kw, base):
    """(scenario, what is subtracted from coordinates) -> everything a labels drive leaves, frame by frame, in coordinates about
    `base`: local planes, the global probes of parity (the same random voxels about the pivot at every base), the statistics
    parity compares"""
    def run(make):
        sc = parity.Scenario(base_vox=tuple(int(b) for b in base), **kw)
        off = np.array(base, np.int64)
        m = make(sc.config())
        rng = np.random.default_rng(5)
        out = []
        try:
            for pos, q, kind, data, kw_ in sc.frames_iter():
                m.set_pose(pos, q)
                parity._feed(m, kind, data, kw_)
                m.step()
                r = m.read_local()
                pvt = np.array(m.pivot(), np.int64) - off
                xyz = parity.probe_coords(pvt, sc.size, rng, margin=sc.probe_margin)
                st = m.stats()
                out.append(dict(type=r["type"], dist_sq=r["dist_sq"], coc=r["coc"], g=m.query_global((xyz + off).astype(np.int32)), pivot=pvt,
                                stats=tuple(st[k] for k in ("seeds_a", "seeds_b", "seeds_c", "levels_a", "levels_b", "levels_c", "visits_a",
                                                            "visits_b", "visits_c", "blocks_total"))))
        finally:
            m.close()
        return out
    return run


@functools.lru_cache(maxsize=None)
def _record_near(name, edge, near, make):
    return _record(_twin_kw(name, edge), near)(make)


def _twin_kw(name, edge):
    kw = dict({k["name"]: k for k in (LABELS, FUSE_JUMP)}[name])
    if edge and "steps_edge" in kw:
        kw["steps"] = kw["steps_edge"]
    kw.pop("steps_edge", None)
    return kw


def _moved(coc, by):
    """a closest obstacle of the near run, where the far run must hold it: moved by the whole blocks between the two, a record
    without an obstacle as it is"""
    none = (coc == EMPTY_KEY).all(-1, keepdims=True)
    return np.where(none, coc, coc + by)


def _twin_differences(kw, which, make):
    """(voxel-frames whose local record differs, probes whose global record differs, frames whose statistics differ) between the
    drive at the base and its twin next to the origin"""
    edge = which == "edge"
    tk = _twin_kw(kw["name"], edge)
    base = np.array(base_of(tk, which), np.int64)
    near = base % 16
    far = _record(tk, base)(make)
    loc = glb = stat = 0
    for f, n in zip(far, _record_near(kw["name"], edge, tuple(int(v) for v in near), make)):
        assert np.array_equal(f["pivot"], n["pivot"])
        assert np.array_equal(f["g"]["occ_val"], n["g"]["occ_val"])           # what was observed is the same world
        loc += int(((f["type"] != n["type"]) | (f["dist_sq"] != n["dist_sq"]) | (f["coc"] != _moved(n["coc"].astype(np.int64), base - near)).any(-1)).sum())
        glb += int(((f["g"]["vox_type"] != n["g"]["vox_type"]) | (f["g"]["dist_sq"] != n["g"]["dist_sq"])
                    | (f["g"]["coc"] != _moved(n["g"]["coc"].astype(np.int64), base - near)).any(-1)).sum())
        stat += f["stats"] != n["stats"]
    return loc, glb, stat


TWINS = [(kw, which) for kw in (LABELS, FUSE_JUMP) for which in ("neg", "pos")]


@pytest.mark.parametrize("make", [OracleMapper, EmuMapper], ids=["oracle", "emulation"])
@pytest.mark.parametrize("kw,which", TWINS, ids=_ids(TWINS))
def test_far_drive_is_the_twin_of_the_drive_at_the_origin_cpu(oracle_lib, kw, which, make):
    assert _twin_differences(kw, which, make) == (0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,which", TWINS, ids=_ids(TWINS))
def test_far_drive_is_the_twin_of_the_drive_at_the_origin(kw, which):
    assert _twin_differences(kw, which, _hip()) == (0, 0, 0)


@pytest.mark.parametrize("kw", [LABELS, FUSE_JUMP], ids=["far_labels", "far_fuse_only_then_jump"])
def test_the_900000_rule_fires_at_the_edge_base(oracle_lib, kw):
    """base (iii) is not vacuous: on the oracle alone, the drive that ends on +900000 is NOT the twin of the drive at the origin —
    obstacles above 900000 are no valid closest obstacles for the waves outside the volume, and the global records show it"""
    loc, glb, stat = _twin_differences(kw, "edge", OracleMapper)
    assert glb > 0, (loc, glb, stat)


# ---- the edge of what gie_set_pose accepts
def _acceptance_edge(make):
    size = (21, 21, 43)
    lab = scenes.hash_world_labels((0, 0, 0), size, 0, seed=3, p_occ=0.03).astype(np.int8)
    for sign in (1, -1):
        cfg = gie.make_config(W, size, cutoff_dist=1.0)
        m, o = make(cfg), OracleMapper(cfg)
        try:
            on = tuple(np.float32(sign * LIM * W) for _ in range(3))
            assert float(on[0]) == sign * 112500.0
            m.set_pose(on)                                                    # +-900000 voxels on every axis: accepted
            o.set_pose(on)
            pvt, frame = m.pivot(), m.stats()["frame"]
            assert pvt == o.pivot() == tuple(sign * LIM - s // 2 for s in size) and frame == 1
            for ax in range(3):                                               # one voxel further on any axis: refused, nothing changes
                bad = [np.float32(0.0)] * 3
                bad[ax] = np.float32(sign * (LIM + 1) * W)
                assert float(bad[ax]) == sign * (LIM + 1) * W                 # (exact: 1/128 m is one ulp out there)
                with pytest.raises(RuntimeError):
                    m.set_pose(bad)
                assert m.pivot() == pvt and m.stats()["frame"] == frame
            for mm in (m, o):                                                 # the update the accepted pose began goes on as if nothing had been asked
                mm.ogm_labels(lab)
                mm.step()
            ra, rb = o.read_local(), m.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), (sign, key)
            assert (ra["type"] == 2).any() and m.stats()["frame"] == o.stats()["frame"] == 1
        finally:
            m.close(); o.close()
    # the limit in metres: with voxels of 2 m, 1.0e6 m are 500000 voxels
    m = make(gie.make_config(2.0, size, cutoff_dist=8.0))
    try:
        for sign in (1.0, -1.0):
            m.set_pose((np.float32(sign * 1.0e6), 0.0, 0.0))
            assert m.pivot()[0] == int(sign * 500000) - size[0] // 2
            pvt, frame = m.pivot(), m.stats()["frame"]
            with pytest.raises(RuntimeError):
                m.set_pose((0.0, np.nextafter(np.float32(sign * 1.0e6), np.float32(sign * np.inf)), 0.0))
            assert m.pivot() == pvt and m.stats()["frame"] == frame
    finally:
        m.close()


def test_acceptance_edge_emulation(oracle_lib):
    _acceptance_edge(EmuMapper)


@pytest.mark.gpu
def test_acceptance_edge(oracle_lib):
    _acceptance_edge(_hip())


# ---- the frame counter through a multiple of 2^18
WRAP = 1 << 18
# A loop of six moves of four voxels, one along each direction, then the first three again, in a dense hash world half of whose
# obstacles toggle with period 2: update k + 6 stands where update k stood, moves as it moved and sees the world it saw, so it
# stamps and asks about the local indices update k stamped — on the face the move left behind, which the moves in between (other
# faces) leave alone.  In "collide" that pairs the updates at counts 2, 3, 4 with those at 2^18 + 2, + 3, + 4, whose stamp bases are
# theirs.  Waves A, B and C run in every update after the first.
WRAP_STEPS = [(4, 0, 0), (0, 4, 0), (0, 0, 4), (-4, 0, 0), (0, -4, 0), (0, 0, -4), (4, 0, 0), (0, 4, 0), (0, 0, 4)]
WRAP_SCENE = dict(name="wrap", size=(40, 29, 40), voxel=W, sensor="labels", seed=893, p_occ=0.03, toggle=0.5, frames=10, steps=WRAP_STEPS)
# The second statement follows the same drive with a quarter of the obstacles toggling: with half of them its serial schedule and
# the canonical one differ by 0.76 voxel in a voxel INSIDE the volume in update 5 — at the origin, with an untouched counter —
# which is beyond the half voxel test_merge_second_opinion.py's run_scene allows two witnesses (a bound that stays as it is).
WRAP_SCENE_2ND = dict(WRAP_SCENE, name="wrap_2nd", toggle=0.25)
# drive -> {frame number: what the counter is set to ahead of that frame}
WRAP_DRIVES = {
    "through_2^18": {0: WRAP - 5},                         # counts 2^18 - 4 ... 2^18 + 5: the wrap is the fifth update
    "through_2^30": {0: (1 << 30) - 5},                    # a later multiple: the counter's magnitude in the raise stamp -map_ct
    "collide": {5: WRAP - 1},                              # counts 1 ... 5, then 2^18 (the wrap) and 2^18 + 1 ... + 4, whose stamps are those of counts 1 ... 4
}


def _wrap_hooks(sets, first=0):
    want = {}

    def before(k, *mappers):
        if k in sets:
            for m in mappers:
                if hasattr(m, "debug_set_frame"):
                    m.debug_set_frame(sets[k])
                else:
                    m.map_ct = sets[k]                     # MergeChecker: a plain attribute
            want["ct"] = sets[k]
        want["ct"] = want.get("ct", first) + 1

    def after(k, a, b):
        assert a.stats()["frame"] == b.stats()["frame"] == want["ct"], (k, a.stats()["frame"], b.stats()["frame"], want["ct"])
    return before, after


def _loop_drive(sc, make, mode, fast, before=None, after=None, idle=0):
    """the loop drive staged, as a node runs it, or with the changed-block flags on in most updates; waves A, B and C must have
    work in every update after the first (fast mode runs wave C alone) but `idle` of them"""
    if mode == "stream":
        parity.run_irregular(sc, OracleMapper, make, stream_on={2, 3, 4, 5, 6, 8}, before_frame=before, after_frame=after)
        return
    stats = parity.run_and_compare(sc, OracleMapper, make, production=(mode == "production"), before_frame=before, after_frame=after)
    # the traffic the stamps, and the 900000 rule, decide about
    busy = [(st["visits_c"] if fast else min(st["visits_a"], st["visits_b"], st["visits_c"])) > 0 for st in stats[1:]]
    assert sum(busy) >= len(busy) - idle, [(st["visits_a"], st["visits_b"], st["visits_c"]) for st in stats]


def _wrap(make, drive, mode, fast):
    before, after = _wrap_hooks(WRAP_DRIVES[drive])
    _loop_drive(scene(WRAP_SCENE, "origin", fast_mode=fast), make, mode, fast, before, after)


_wrap_cases = [(d, mode, fast) for d in WRAP_DRIVES for mode in ("staged", "production", "stream") for fast in (False, True)]
_wrap_ids = ["%s-%s-%s" % (d, mode, "fast" if fast else "full") for d, mode, fast in _wrap_cases]


@pytest.mark.parametrize("drive,mode,fast", _wrap_cases, ids=_wrap_ids)
def test_frame_wrap_emulation(oracle_lib, drive, mode, fast):
    _wrap(EmuMapper, drive, mode, fast)


@pytest.mark.gpu
@pytest.mark.parametrize("drive,mode,fast", _wrap_cases, ids=_wrap_ids)
def test_frame_wrap(oracle_lib, drive, mode, fast):
    _wrap(_hooks(), drive, mode, fast)


# the same loop drive at the far bases: at "edge" it ends on +900000 on every axis, with hundreds of wave A and wave B visits in
# every update among obstacles on both sides of the 900000 rule — but the one that moves down in z from there: the face it leaves
# behind lies above 900000 altogether, where no stored obstacle is valid and waves A and B find nothing to do
_loop_cases = [(which, mode) for which in BASES for mode in ("staged", "production", "stream")]


@pytest.mark.parametrize("which,mode", _loop_cases, ids=["%s-%s" % c for c in _loop_cases])
def test_far_pose_loop_drive_emulation(oracle_lib, which, mode):
    _loop_drive(scene(dict(WRAP_SCENE, name="far_loop"), which), EmuMapper, mode, False, idle=(which == "edge"))


@pytest.mark.gpu
@pytest.mark.parametrize("which,mode", _loop_cases, ids=["%s-%s" % c for c in _loop_cases])
def test_far_pose_loop_drive(oracle_lib, which, mode):
    _loop_drive(scene(dict(WRAP_SCENE, name="far_loop"), which), _hip(), mode, False, idle=(which == "edge"))


@pytest.mark.parametrize("drive", list(WRAP_DRIVES))
def test_frame_wrap_second_statement_emulation(oracle_lib, drive):
    before, _ = _wrap_hooks(WRAP_DRIVES[drive])
    _second_opinion(WRAP_SCENE_2ND, "origin", EmuMapper, before_frame=before)


@pytest.mark.gpu
@pytest.mark.parametrize("drive", list(WRAP_DRIVES))
def test_frame_wrap_second_statement(drive):
    before, _ = _wrap_hooks(WRAP_DRIVES[drive])
    _second_opinion(WRAP_SCENE_2ND, "origin", _hooks(), before_frame=before)


def _set_frame_hook(make):
    """gie_debug_set_frame sets the counter and nothing else; it refuses a negative count and a call inside an open merge"""
    size = (21, 21, 43)
    cfg = gie.make_config(W, size, cutoff_dist=1.0)
    m = make(cfg)
    try:
        with pytest.raises(RuntimeError):
            m.debug_set_frame(-1)
        m.debug_set_frame(41)
        assert m.stats()["frame"] == 41
        m.set_pose((0.0, 0.0, 0.0))
        assert m.stats()["frame"] == 42 and m.pivot() == tuple(-(s // 2) for s in size)
        m.ogm_labels(scenes.hash_world_labels(m.pivot(), size, 0, seed=3, p_occ=0.03).astype(np.int8))
        m.fuse(); m.batch_edt(); m.merge_begin_tiled()
        with pytest.raises(RuntimeError):
            m.debug_set_frame(7)
        assert m.stats()["frame"] == 42
        m.merge_end()
        before = m.read_local()
        m.debug_set_frame(7)
        after = m.read_local()
        assert m.stats()["frame"] == 7 and all(np.array_equal(before[k], after[k]) for k in before)
    finally:
        m.close()


def test_set_frame_hook_emulation():
    _set_frame_hook(EmuMapper)


@pytest.mark.gpu
def test_set_frame_hook():
    _set_frame_hook(_hooks())


# ---- the planner stages at far poses (HIP only: the oracle and the emulation do not have them)
P_SIZE = (97, 61, 45)
P_CLEAR = 0.25                  # metres: two voxels, for frontier members, NF1 and the opaque plane alike
P_CAP, P_MIN = 12, 3
P_LEN, P_LOOK, P_WP = 64, 8, 16
P_GAIN = (0.0, 1.5, 0.7)        # r_min, r_max (metres), tan2_elev


def _exact_points(rng, pvt, n, lo=-3):
    """world points on multiples of w / 16 about the volume (some outside): float32 holds them without rounding out to 900000 voxels"""
    u = rng.integers(lo * 16, (np.array(P_SIZE) - lo) * 16, size=(n, 3)).astype(np.float64) / 16.0
    xyz = ((u + np.asarray(pvt, np.float64)) * W).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), (u + np.asarray(pvt, np.float64)) * W)
    return xyz


def _jittered_points(rng, pvt, n):
    """voxel centres jittered by +-0.3 voxel the way the stages' own tests make them (float32 sum, then float32 product)"""
    v = (rng.integers(0, np.array(P_SIZE), size=(n, 3)).astype(np.float64) + np.asarray(pvt, np.float64)).astype(np.float32)
    return ((v + rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)) * np.float32(W)).astype(np.float32)


def _planner_stages(base):
    """every planner stage of a solid scene at pose `base` (voxels) against its numpy reference at that pivot, by the equality or
    tolerance the stage's own GPU test uses; returns the integer outputs in coordinates about `base` for the twin comparison"""
    import cloud_ref
    import frontier_ref as fr
    import los_ref as lr
    import nf1_ref
    import path_ref
    import planner_scenes as ps
    import sdf_ref
    from stage_common import bits, closed_room
    off = np.array(base, np.int64)
    w = np.float32(W)
    m = gie.Mapper(gie.make_config(W, P_SIZE, fast_mode=False, cutoff_dist=3.0))
    out = {}
    try:
        lab = ps.solid_labels(P_SIZE, 3)
        closed_room(lab, 12, 10, P_SIZE[2] // 2 - 5, (9, 9, 9), (3, 3, 3))
        pos = tuple(np.float32(int(b) * W) for b in base)
        for _ in range(2):
            m.set_pose(pos)
            m.ogm_labels(lab)
            m.step()
        pvt = m.pivot()
        assert pvt == tuple(int(b) - s // 2 for b, s in zip(base, P_SIZE))
        loc = m.read_local()
        ty, edt = loc["type"], loc["edt"]
        c = np.float32(P_CLEAR) / w
        rng = np.random.default_rng(11)                                       # the same draws at every base
        # the costmap headers: the origin is (float)pvt * w
        _, ch = m.read_costmap()
        want_origin = [np.float32(np.float32(p) * w) for p in pvt]
        assert [np.float32(ch.x_origin), np.float32(ch.y_origin), np.float32(ch.z_origin)] == want_origin and ch.width == w
        # signed distance: the planes, then the queries against the interpolant of the plane (tests/test_sdf_gpu.py's standard)
        r = m.read_sdf()
        ids = sdf_ref.inside_dist_sq(ty)
        assert np.array_equal(r["inside_dist_sq"], ids)
        assert np.allclose(r["sdf"], sdf_ref.sdf(ids, edt, P_SIZE), rtol=1e-6, atol=0)
        out["inside_dist_sq"] = ids
        for name, xyz in (("exact", _exact_points(rng, pvt, 3000)), ("jitter", _jittered_points(rng, pvt, 3000))):
            d, g, f = m.query_sdf(xyz)
            rd, rg, rf = sdf_ref.query(r["sdf"], ty, P_SIZE, pvt, W, xyz)
            assert np.array_equal(f, rf) and np.array_equal(np.isnan(d), np.isnan(rd)), name
            ok = ~np.isnan(rd)
            assert ok.sum() > 1000 and np.allclose(d[ok], rd[ok], rtol=1e-5, atol=1e-5) and np.allclose(g, rg, rtol=1e-5, atol=1e-5), name
            if name == "exact":
                out["sdf_flags"] = f
        # frontier clusters (tests/test_frontier_gpu.py _check)
        nc, nv = m.frontier_compute(P_CLEAR, P_MIN, 26, P_CAP)
        labels = m.read_frontier_labels()
        rec, goal, n = m.read_frontier_clusters()
        ref = fr.clusters(fr.members(ty, edt, c), 26, P_MIN, P_CAP, pvt, W)
        assert np.array_equal(labels, ref["labels"])
        assert (nc, nv, n) == (ref["n_clusters"], ref["n_voxels"], ref["n_clusters"]) and nc >= 2
        assert rec.tobytes() == ref["records"].tobytes() and np.array_equal(bits(goal), bits(ref["goals"]))
        out.update(frontier_labels=labels, frontier_counts=(nc, nv), frontier_size=rec["size"].copy(), frontier_sum=rec["sum"].copy(),
                   frontier_box=np.stack([rec["lo"], rec["hi"], rec["rep"]]).astype(np.int64) - off)
        # NF1 towards the clusters' goals and two points of the exact set; paths from both point sets; the costmap
        free = np.argwhere((ty == 1) & (edt > c + 1))[:, ::-1]
        pick = free[rng.choice(len(free), 2, replace=False)]
        goals = np.concatenate([goal[:min(nc, P_CAP)], ((pick + np.asarray(pvt, np.float64) + 0.25) * W).astype(np.float32)])
        ns = m.nf1_compute(goals, P_CLEAR)
        f = m.read_nf1()
        rf_, trav, src = nf1_ref.field(ty, edt, c, 0, goals, W, pvt)
        assert ns == int(src.sum()) and ns >= 3 and np.array_equal(f, rf_)
        out["nf1"] = f
        reach = np.argwhere(f > 20)[:, ::-1]
        assert len(reach) > 100
        at = reach[rng.choice(len(reach), 24, replace=False)]
        starts = {"exact": ((at + np.asarray(pvt, np.float64) + rng.integers(-4, 5, at.shape) / 16.0) * W).astype(np.float32),
                  "jitter": (((at + np.asarray(pvt, np.float64)).astype(np.float32) + rng.uniform(-0.3, 0.3, at.shape).astype(np.float32)) * w).astype(np.float32)}
        for name, st in starts.items():
            st = np.concatenate([st, _exact_points(rng, pvt, 4, lo=-6)])       # (and a few anywhere: obstacles, outside)
            got, glen = m.nf1_path(st, P_LEN)
            rp, rlen = nf1_ref.paths(f, st, W, pvt, P_LEN)
            assert np.array_equal(glen, rlen) and all(np.array_equal(a, b) for a, b in zip(got, rp)), name
            assert (rlen > 20).sum() >= 20
            if name == "exact":
                path = np.zeros((len(st), P_LEN, 3), np.int32)
                for i, p in enumerate(got):
                    path[i, :len(p)] = p
                lens = glen
                out["path_lens"] = glen
                out["paths"] = [np.asarray(p, np.int64) - off for p in got]
        pay, hdr = m.read_costmap_nf1()
        assert hdr.type == 2 and [np.float32(hdr.x_origin), np.float32(hdr.y_origin), np.float32(hdr.z_origin)] == want_origin
        assert (hdr.x_size, hdr.y_size, hdr.z_size, hdr.width) == (ch.x_size, ch.y_size, ch.z_size, ch.width)
        assert np.array_equal(pay["d"].view(np.uint32), np.where(f >= 0, f.astype(np.float32), np.float32(-1.0)).view(np.uint32))
        assert np.array_equal(pay["o"], (ty != 0).astype(np.uint8))
        # line of sight: the plane, segments between points of both sets, the gain at the goals
        n_op = m.los_prepare(P_CLEAR, 0)
        opq = lr.opaque(ty, edt, c, 0)
        assert n_op == int(opq.sum()) and np.array_equal(m.read_los_opaque(), opq.astype(np.uint8))
        out.update(opaque=opq, n_opaque=n_op)
        for name, mk in (("exact", lambda k: _exact_points(rng, pvt, k, lo=-1)), ("jitter", lambda k: _jittered_points(rng, pvt, k))):
            a, b = mk(600), mk(600)
            seg = m.los_segments(a, b)
            want = lr.segments(edt, opq, a, b, W, pvt)
            assert seg.tobytes() == want.tobytes(), name
            assert (want["first"] == -1).sum() > 10 and (want["first"] >= 0).sum() > 10
            if name == "exact":
                out["seg"] = (seg["first"].copy(), seg["len"].copy(), np.where((seg["first"] != -2)[:, None], seg["hit"].astype(np.int64) - off, 0))
        views = gie.make_views(goals)
        gain = m.view_gain(views, *P_GAIN)
        assert gain.tobytes() == lr.view_gain(ty, opq, views, P_GAIN[0], P_GAIN[1], P_GAIN[2], W, pvt).tobytes()
        assert (gain["candidates"] > 0).all()
        out["gain"] = gain
        # path shortcutting over that plane, on the paths of the exact starts
        wp, info = m.path_shortcut(path, lens, P_LOOK, P_WP)
        rwp, rinfo = path_ref.shortcut(edt, opq, path, lens, pvt, P_LOOK, P_WP)
        assert wp.tobytes() == rwp.tobytes() and info.tobytes() == rinfo.tobytes()
        assert (info["count"] > 2).any()
        written = np.arange(P_WP)[None, :] < np.minimum(info["count"], P_WP)[:, None]
        out["shortcut"] = (info["count"].copy(), info["forced"].copy(), np.where(written, wp["index"], -9), wp["forced"].copy(),
                           np.where(written[..., None], wp["xyz"].astype(np.int64) - off, 0))
        # display clouds, local and global, in both intensity modes
        box_lo, box_hi = np.array(pvt) - 8, np.array(pvt) + np.array(P_SIZE) + 8
        gxyz = cloud_ref.box_coords(box_lo, box_hi)
        grec = m.query_global(gxyz)
        for name, p in (("ogm", cloud_ref.param(1 << cloud_ref.OCCUPIED, cloud_ref.TYPE)), ("edt", cloud_ref.param(cloud_ref.KNOWN, cloud_ref.DIST))):
            for form, want in (("local", cloud_ref.local_cloud(ty, edt, pvt, W, p)), ("global", cloud_ref.global_cloud(grec, gxyz, W, p))):
                got, count = (m.cloud_local if form == "local" else m.cloud_global)(p["type_mask"], p["intensity"])
                assert count == len(want) == len(got) > 0, (name, form, count, len(want))
                assert cloud_ref.canon(got).tobytes() == cloud_ref.canon(want).tobytes(), (name, form)
                vox = np.stack([np.rint(got[k].astype(np.float64) / W).astype(np.int64) for k in ("x", "y", "z")], -1)
                assert np.array_equal((vox * W).astype(np.float32), np.stack([got[k] for k in ("x", "y", "z")], -1))
                rows = np.concatenate([vox - off, got["intensity"].view(np.uint32).astype(np.int64)[:, None]], 1)
                out["cloud_%s_%s" % (name, form)] = rows[np.lexsort(rows.T[::-1])]
    finally:
        m.close()
    return out


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _planner_near(near):
    return _planner_stages(near)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["neg", "edge"])
def test_planner_stages_at_far_poses(which):
    """read_sdf / query_sdf, frontier_compute and its readers, nf1_compute / nf1_path / read_costmap_nf1, los_prepare /
    los_segments / view_gain, path_shortcut, cloud_local / cloud_global: each against its tests/*_ref.py at the far pivot, and the
    integer outputs against the twin next to the origin (base mod 16, as the translation twins above)."""
    base = np.array({"neg": (-LIM + 3,) * 3, "edge": (LIM,) * 3}[which], np.int64)
    far = _planner_stages(tuple(int(b) for b in base))
    near = _planner_near(tuple(int(b) for b in base % 16))
    assert far.keys() == near.keys()
    for key in far:
        assert _same(far[key], near[key]), key

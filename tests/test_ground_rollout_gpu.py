"""Ground rollouts on the device (include/gie.h "ground rollouts", gie_ground_rollout.inc.h) against the numpy statement of
tests/ground_rollout_ref.py, evaluated on the planes the same mapper's read_ground() and read_ground_nf1() return.  Every comparison
is of bytes."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import gie
import ground_ref as R
import ground_rollout_ref as Q
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, ground as _ground, xy as _xy, scene as _scene, open_cells as _open, same as _same, arc
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries of a mapper without frontier clusters
RD = gie.GROUND_ROLLOUT_DTYPE
# clearance_sq x inflate_sq x the two flags: every combination, in an order that mixes them
COMBOS = [(c, i, u, nf) for (u, nf), c, i in itertools.product(((False, False), (True, True), (False, True), (True, False)), (0, 1, 4, 9), (0, 16, 1 << 22))]


def _flags(unknown, nf1):
    return (Q.UNKNOWN_TRAVERSABLE if unknown else 0) | (Q.NF1 if nf1 else 0)


def _both_forms(m, st, xy, c, i, u, nf, want, what):
    """the host form and the _dev form over a buffer one record longer, with a poisoned tail: the reference's bytes, nothing beyond"""
    import torch
    n, T = xy.shape[0], xy.shape[1]
    got = m.ground_rollouts(xy, c, i, u, nf)
    assert got.dtype == RD
    _same(got, want, what)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(st):
        dxy = torch.from_numpy(xy).to(dev)
        dout = torch.full(((n + 1) * 48,), 0x5a, dtype=torch.uint8, device=dev)
        m.ground_rollouts_dev(dxy.data_ptr(), n, T, dout.data_ptr(), c, i, u, nf)
    m.sync()
    o = dout.cpu().numpy()
    assert o[:n * 48].tobytes() == want.tobytes() and o[n * 48:].tobytes() == P5A * 48, what
    return got


def _fan(g, pvt, size, T, rng, n=37):
    """n trajectories of T poses (cells, fractions) from FREE (or FNT) cells: straight lines and arcs with steps of 0.3 .. 3 cells, small circles
    in the most open places (the long clear ones), horizontal sweeps over x = 63 | 64 and 127 | 128, and poses on gie_pos2coord's ties"""
    X, Y = size[0], size[1]
    t, d = np.asarray(g["type"]), np.asarray(g["dist_sq"])
    free = np.argwhere(_open(g))[:, ::-1]
    inner = free[(free[:, 0] >= 3) & (free[:, 0] < X - 3) & (free[:, 1] >= 3) & (free[:, 1] < Y - 3)]
    far = inner[np.argsort(-d[inner[:, 1], inner[:, 0]], kind="stable")[:8]]    # the cells farthest from every obstacle column, off the border
    out = []
    for j in range(n):
        kind = j % 6
        if kind in (0, 1):                                      # a straight line; every other one with long steps: legs that jump over cells
            out.append(arc(free[rng.integers(len(free))] + rng.uniform(-0.4, 0.4, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.3 if kind == 0 else 2.0, 3.0), 0.0, T)[0])
        elif kind == 2:                                         # an arc
            out.append(arc(free[rng.integers(len(free))] + rng.uniform(-0.4, 0.4, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 3.0), rng.uniform(-0.2, 0.2), T)[0])
        elif kind == 3:                                         # a small circle in an open place: the long clear ones
            out.append(arc(far[(j // 6) % len(far)], rng.uniform(0, 2 * np.pi), 0.3, rng.choice([-1, 1]) * rng.uniform(0.2, 0.5), T)[0])
        elif kind == 4:                                         # along x towards a word boundary of the bit plane and over it
            x0 = [max(64 - T // 2, 0), max(128 - T // 2, 0), 60, 0][(j // 6) % 4]
            out.append(arc((min(x0, X - 1), int(rng.integers(0, Y))), 0.0, 1.0, 0.0, T)[0])
        else:                                                   # every pose on a tie of the rounding: (cell + 0.5), both axes
            out.append(np.floor(arc(free[rng.integers(len(free))], rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 1.5), 0.0, T)[0]) + 0.5)
    return np.stack(out)


def _calibrated(g, pvt, fan, targets, clearance_sq=0):
    """rows whose first blocked leg is leg `target`, for every target: a blocked trajectory of the fan with its pose 0 repeated in front
    (equal consecutive cells add nothing) — the first bad lane of the chunk is then 63, 0 of the next, ..."""
    T = fan.shape[1]
    ref = Q.rollouts(g, _xy(pvt, fan), pvt, W, clearance_sq)
    rows = []
    for tg in targets:
        pick = [i for i in range(len(fan)) if ref["end"][i] == 1 and 1 <= ref["poses"][i] <= tg]
        if tg >= T or not pick:
            continue
        i = pick[tg % len(pick)]
        k = tg - int(ref["poses"][i])
        rows.append((np.concatenate([np.repeat(fan[i][:1], k, 0), fan[i][:T - k]]), tg))
    return rows


# ---------------------------------------------------------------------------------------------------------- 1. box scenes
def _box_cases(g, nf, pvt, size):
    """the calls of one box scene, from its planes alone: (T, n, xy, (clearance_sq, inflate_sq, unknown, nf1), the reference's records,
    how many calibrated rows ended at their leg) for n in {1, 3, 4, 5, 37} x T in {1, 2, 63, 64, 65, 129, 130}, two parameter
    combinations each, 70 calls over the 48 combinations"""
    rng = np.random.default_rng(size[0])
    call = 0
    for T in (1, 2, 63, 64, 65, 129, 130):
        fan = _fan(g, pvt, size, T, rng)
        cal = _calibrated(g, pvt, fan, (63, 64, 65, 127, 128))
        for k, (row, tg) in enumerate(cal):
            fan[6 * k] = row                                    # (in the place of a straight line; the first of them is row 0: in every n)
        xy_all = _xy(pvt, fan)
        if T > 2:
            xy_all[7, T // 2:] = np.nan                         # a rollout shorter than T
        for n in (1, 3, 4, 5, 37):
            xy = np.ascontiguousarray(xy_all[:n])
            for _ in range(2):
                c, i, u, f1 = COMBOS[call % len(COMBOS)]
                call += 1
                want = Q.rollouts(g, xy, pvt, W, c, i, _flags(u, f1), nf)
                hits = 0
                if c == 0 and not u:                            # the calibrated rows end where they were made to
                    hits = sum(1 for k, (row, tg) in enumerate(cal) if 6 * k < n and want["end"][6 * k] == 1 and want["poses"][6 * k] == tg)
                yield T, n, xy, (c, i, u, f1), want, hits


def _box_conditions(cases, pvt, shape):
    """no case passes vacuously: over the scene's calls at least a tenth of the trajectories complete, a tenth blocked, one left;
    a tenth of the blocked ones inside a leg (the hit is not the cell of pose m); a prefix beyond one chunk; first bad legs on lane
    63 of a chunk and on lane 0 of the next.  All of it from the reference's records."""
    ends, interior, longest, at_target = [], 0, 0, 0
    for T, n, xy, combo, want, hits in cases:
        ends += want["end"].tolist()
        longest = max(longest, int(want["poses"].max()))
        cells = np.array([[-1, -1] if v is None else v for v in Q.N.cells_of(xy[np.arange(n), np.minimum(want["poses"], T - 1)], pvt, W, shape)])
        interior += int(((want["end"] == 1) & (want["poses"] > 0) & np.any(cells + np.array(pvt[:2]) != want["hit"], axis=1)).sum())
        at_target += hits
    cnt = [ends.count(e) for e in (0, 1, 2)]
    print("trajectories %d: complete %d blocked %d left %d; blocked inside a leg %d; longest prefix %d; at a calibrated leg %d" %
          (len(ends), cnt[0], cnt[1], cnt[2], interior, longest, at_target))
    assert len(cases) >= len(COMBOS)                            # every combination of the parameters has run
    assert cnt[0] * 10 >= len(ends) and cnt[1] * 10 >= len(ends) and cnt[2] >= 1
    assert interior * 10 >= cnt[1] and longest > 64 and at_target >= 2


@pytest.mark.parametrize("size", [(64, 24, 8), (65, 24, 8), (70, 24, 8), (130, 24, 8)])
def test_rollouts_equal_the_reference(size):
    import torch
    pos, lab = _scene(size, 100 + size[0] + size[1])
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        t = np.asarray(g["type"])
        assert (t == R.UNKNOWN).any() and (t == R.OCCUPIED).any() and _open(g).sum() > 100
        free = np.argwhere(_open(g))[:, ::-1]
        m.ground_nf1_compute(_xy(pvt, free[len(free) // 2][None]), 2)
        nf = m.read_ground_nf1()
        assert (nf >= 0).sum() > 100 and ((nf < 0) & _open(g)).any()      # (clearance 2: the cells beside an obstacle have no value)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        cases = list(_box_cases(g, nf, pvt, size))
        for T, n, xy, (c, i, u, f1), want, hits in cases:
            _both_forms(m, st, xy, c, i, u, f1, want, (size, T, n, c, i, u, f1))
        _box_conditions(cases, pvt, t.shape)
        assert len(m.ground_rollouts(np.zeros((0, 5, 2), np.float32))) == 0                     # n == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. against the parent's calls
def _from_segments(m, xy, clearance_sq, unknown):
    """end, poses, hit and min_dist_sq from gie_ground_segments over the consecutive poses (leg 0: pose 0 to itself), and the NF1 fields
    from gie_ground_nf1_query at the poses"""
    n, T = xy.shape[0], xy.shape[1]
    a = np.concatenate([xy[:, :1], xy[:, :-1]], 1)
    seg = m.ground_segments(a.reshape(-1, 2), xy.reshape(-1, 2), clearance_sq, unknown).reshape(n, T)
    steps = m.ground_nf1_query(xy.reshape(-1, 2)).reshape(n, T)
    out = np.zeros(n, RD)
    for i in range(n):
        bad = np.flatnonzero(seg["first"][i] != -1)             # -2: a pose without a cell; >= 0: a blocked cell
        k = int(bad[0]) if len(bad) else T
        out[i]["poses"] = k
        if k < T:
            out[i]["end"] = 2 if seg["first"][i, k] == -2 else 1
            if out[i]["end"] == 1:
                out[i]["hit"] = seg["hit"][i, k]
        out[i]["min_dist_sq"] = seg["min_dist_sq"][i, :k].min() if k else 0
        good = steps[i, :k][steps[i, :k] >= 0]
        out[i]["nf1_end"] = steps[i, k - 1] if k else -1
        out[i]["nf1_min"] = good.min() if len(good) else -1
        out[i]["nf1_min_at"] = int(np.flatnonzero(steps[i, :k] == good.min())[0]) if len(good) else -1
    return out


def test_agrees_with_segments_and_nf1_query_on_the_same_poses():
    size = (70, 24, 8)
    pos, lab = _scene(size, 77)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        free = np.argwhere(_open(g))[:, ::-1]
        m.ground_nf1_compute(_xy(pvt, free[::40]), 0, True)
        rng = np.random.default_rng(3)
        for T in (2, 65):
            xy = _xy(pvt, _fan(g, pvt, size, T, rng))
            xy[5, T - 1] = np.nan
            for c, u in ((0, False), (4, False), (1, True)):
                got = m.ground_rollouts(xy, c, 16, u, True)
                want = _from_segments(m, xy, c, u)
                for key in ("end", "poses", "hit", "min_dist_sq", "nf1_end", "nf1_min", "nf1_min_at"):
                    assert np.array_equal(got[key], want[key]), (T, c, u, key, got[key].tolist(), want[key].tolist())
                assert len(set(got["end"].tolist())) == 3 and (got["nf1_min"] >= 0).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. sizes
def test_4096_poses():
    import torch
    size = (130, 24, 8)
    pos, lab = _scene(size, 100 + size[0] + size[1])
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        m.ground_nf1_compute(_xy(pvt, [(64, 12)]), 0, True)
        nf = m.read_ground_nf1()
        rng = np.random.default_rng(4096)
        fan = _fan(g, pvt, size, 4096, rng, n=6)
        xy = _xy(pvt, np.stack([fan[3], arc(fan[0][0], 0.3, 0.02, 0.0005, 4096)[0]]))   # a small circle, and a slow drift across the field
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        want = Q.rollouts(g, xy, pvt, W, 0, 1 << 22, Q.NF1, nf)
        got = _both_forms(m, st, xy, 0, 1 << 22, False, True, want, "T = 4096")
        assert got["poses"][0] == 4096 and got["end"][0] == 0 and got["cost"][0] > 2 ** 31 and got["poses"][1] > 64
        with pytest.raises(Exception):
            m.ground_rollouts(np.zeros((1, 4097, 2), np.float32))
    finally:
        m.close()


def test_66000_trajectories_in_one_call():
    import torch
    size = (64, 24, 8)
    pos, lab = _scene(size, 188)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        m.ground_nf1_compute(_xy(pvt, [(30, 12)]), 0, True)
        nf = m.read_ground_nf1()
        n = 66000                                               # beyond 65535: the trajectories are not a grid dimension of their own
        rng = np.random.default_rng(66)
        a = np.stack([rng.integers(-1, size[0] + 1, 3000), rng.integers(-1, size[1] + 1, 3000)], 1)
        uniq = _xy(pvt, np.stack([a, a + rng.integers(-4, 5, (3000, 2))], 1))
        idx = rng.integers(0, 3000, n)
        xy = np.ascontiguousarray(uniq[idx])
        want = Q.rollouts(g, uniq, pvt, W, 1, 16, Q.NF1, nf)[idx]
        assert min((want["end"] == e).sum() for e in (0, 1, 2)) > 2000
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        _both_forms(m, st, xy, 1, 16, False, True, want, "66000")
    finally:
        m.close()


@pytest.mark.parametrize("size,wall", [((1024, 3, 1), None), ((1024, 3, 1), 600), ((3, 1024, 1), None), ((3, 1024, 1), 600)])
def test_one_straight_rollout_end_to_end_at_the_largest_side(size, wall):
    X, Y = size[0], size[1]
    axis = 0 if X > Y else 1
    lab = np.ones((1, Y, X), np.int8)
    if wall is not None:
        lab[(0, slice(None), wall) if axis == 0 else (0, wall, slice(None))] = 2
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pvt = _settle(m, lab)
        g = _ground(m, size)
        assert (np.asarray(g["type"]) == R.OCCUPIED).sum() == (0 if wall is None else 3)
        cells = np.ones((2, 1024, 2), np.int64)
        cells[0, :, axis] = np.arange(1024)
        cells[1, :, axis] = np.arange(1023, -1, -1)
        xy = _xy(pvt, cells)
        got = m.ground_rollouts(xy, 0, 1 << 22)
        _same(got, Q.rollouts(g, xy, pvt, W, 0, 1 << 22), (size, wall))
        if wall is None:
            assert got["end"].tolist() == [0, 0] and got["poses"].tolist() == [1024, 1024] and got["cells"].tolist() == [1024, 1024]
            assert got["min_dist_sq"].tolist() == [-1, -1] and got["cost"].tolist() == [0, 0]
        else:
            hit = [0, 0]
            hit[axis], hit[1 - axis] = wall + pvt[axis], 1 + pvt[1 - axis]
            assert got["end"].tolist() == [1, 1] and got["poses"].tolist() == [600, 1023 - 600] and got["hit"].tolist() == [hit, hit]
            assert got["cost"][0] == sum((1 << 22) - k * k for k in range(1, 601)) and got["min_dist_sq"].tolist() == [1, 1]
    finally:
        m.close()


def test_a_field_without_an_obstacle_column():
    size = (70, 24, 8)
    lab = np.ones((8, 24, 70), np.int8)
    lab[:, :, :5] = 0                                           # a never-seen slab: UNKNOWN columns, no obstacle
    m = _mapper(size)
    try:
        pvt = _settle(m, lab)
        g = _ground(m, size)
        assert (g["dist_sq"] == -1).all() and (g["type"] == R.UNKNOWN).any()
        rng = np.random.default_rng(9)
        xy = _xy(pvt, _fan(g, pvt, size, 65, rng))
        for c, i, u in ((0, 0, False), (9, 1 << 22, False), (100000, 16, True)):
            want = Q.rollouts(g, xy, pvt, W, c, i, _flags(u, False))
            _same(m.ground_rollouts(xy, c, i, u), want, (c, i, u))
            assert (want["cost"] == 0).all() and (want["min_dist_sq"][want["poses"] > 0] == -1).all() and (want["poses"] > 0).sum() > 20
        with pytest.raises(Exception):                          # no navigation function yet
            m.ground_rollouts(xy, 0, 0, False, True)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. chained
def test_chained_behind_the_ground_field_and_its_nf1_with_one_sync():
    import torch
    size = (70, 40, 8)
    pos, lab = _scene(size, 91, n_boxes=10)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        z = pvt[2]
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(1)
        goal = _xy(pvt, [(40, 20), (10, 30)])
        fan = np.stack([arc((35, 20) + rng.uniform(-8, 8, 2), rng.uniform(0, 6.28), rng.uniform(0.3, 2.0), rng.uniform(-0.1, 0.1), 40)[0] for _ in range(33)])
        xy = _xy(pvt, fan)
        n, T = xy.shape[0], xy.shape[1]
        with torch.cuda.stream(torch.cuda.ExternalStream(m.stream_handle(), device=dev)):
            dgoal = torch.from_numpy(goal).to(dev)
            dxy = torch.from_numpy(xy).to(dev)
            dout = torch.full(((n + 1) * 48,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_compute_dev(z, z + size[2] - 1, 1, False, 0)
            m.ground_nf1_compute_dev(dgoal.data_ptr(), 2, 1, False, True, 0)
            m.ground_rollouts_dev(dxy.data_ptr(), n, T, dout.data_ptr(), 1, 16, False, True)
        m.sync()                                                # the only wait
        o = dout.cpu().numpy()
        want = Q.rollouts(m.read_ground(), xy, pvt, W, 1, 16, Q.NF1, m.read_ground_nf1())
        assert o[:n * 48].tobytes() == want.tobytes() and o[n * 48:].tobytes() == P5A * 48
        assert (want["poses"] > 1).sum() > 10 and (want["nf1_min"] >= 0).sum() > 10 and (want["cost"] > 0).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. lifetime
def test_the_field_decides_and_a_map_update_does_not():
    size = (64, 48, 8)
    rng = np.random.default_rng(7)
    boxes = []
    for _ in range(40):
        s = rng.integers(3, 10, size=3)
        c = rng.integers((-40, -28, -6), (60, 24, 4))
        boxes.append((c, c + s))
    m = _mapper(size)
    try:
        def step(k):
            pos, q = scenes.pose(k, W, delta_vox=5, yaw_deg=0.0)
            pvt = scenes.local_pivot(pos, W, size)
            m.set_pose(pos, q)
            m.ogm_labels(box_labels(pvt, size, k, boxes, unknown_slab=2))
            m.step()
            return pvt
        pvt0 = step(0)
        g0 = _ground(m, size)
        m.ground_nf1_compute(_xy(pvt0, [(30, 24)]), 1, False, True)
        nf0 = m.read_ground_nf1()
        xy = _xy(pvt0, _fan(g0, pvt0, size, 20, np.random.default_rng(2), n=24))
        r0 = m.ground_rollouts(xy, 1, 16, False, True)
        _same(r0, Q.rollouts(g0, xy, pvt0, W, 1, 16, Q.NF1, nf0), "before")
        assert len(set(r0["end"].tolist())) >= 2
        # the calls wrote nothing of the ground field or of its navigation function
        g0b = m.read_ground()
        assert all(np.array_equal(g0[k], g0b[k]) for k in g0) and np.array_equal(m.read_ground_nf1(), nf0)
        # a map update between two calls changes no result: the field stays at its own pivot
        pvt1 = step(1)
        assert tuple(pvt1) != tuple(pvt0)
        assert m.ground_rollouts(xy, 1, 16, False, True).tobytes() == r0.tobytes()
        # a new ground field does: later calls see it, at its pivot, with no prepare in between; its navigation function is gone
        g1 = _ground(m, size)
        r1 = m.ground_rollouts(xy, 1, 16)
        _same(r1, Q.rollouts(g1, xy, pvt1, W, 1, 16), "after")
        assert any(r1[k].tobytes() != r0[k].tobytes() for k in ("end", "poses", "hit", "cells", "min_dist_sq", "cost"))
        with pytest.raises(Exception):
            m.ground_rollouts(xy, 1, 16, False, True)
        m.ground_nf1_compute(_xy(pvt1, [(30, 24)]), 1, False, True)
        _same(m.ground_rollouts(xy, 1, 16, False, True), Q.rollouts(g1, xy, pvt1, W, 1, 16, Q.NF1, m.read_ground_nf1()), "with the new function")
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, t = _mapper(size), _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        f = m._f
        n, T = 4, 3
        host = np.frombuffer(P5A * 4096, np.uint8).copy()
        dbuf = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [[(3, 3), (4, 4), (5, 5)], [(9, 9), (9, 10), (9, 11)], [(20, 4), (21, 4), (22, 4)], [(1, 1), (1, 1), (1, 1)]])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())

        def RP(**kw):
            p = _capi.GroundRolloutParam(0, 0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert host.tobytes() == P5A * host.size and bool((dbuf == 0x5a).all())

        def refused(h, who, p="default", n_=n, T_=T, a=True, out=True):
            p = RP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_rollouts"](h, ptr(xy) if a else None, n_, T_, pr, ptr(host) if out else None) == INVALID, who
            assert f["ground_rollouts_dev"](h, dp if a else None, n_, T_, pr, dp if out else None) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            refused(h, who)
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper
        refused(t._h, "tiled")
        unwritten()
        z = pvt[2]
        m.ground_compute(z, z + 7)
        refused(m._h, "null param", None)
        bad = [RP(clearance_sq=-1), RP(clearance_sq=-2 ** 31), RP(inflate_sq=-1), RP(inflate_sq=(1 << 22) + 1), RP(inflate_sq=2 ** 31 - 1), RP(flags=4), RP(flags=7),
               RP(flags=-2 ** 31), RP(flags=8)] + [RP(reserved=i) for i in range(5)]
        for p in bad:
            refused(m._h, (p.clearance_sq, p.inflate_sq, p.flags, list(p.reserved)), p)
        refused(m._h, "the NF1 flag without a navigation function", RP(flags=2))
        refused(m._h, "the NF1 flag without a navigation function", RP(flags=3))
        refused(m._h, "n < 0", n_=-1)
        for bad_T in (0, -1, 4097, 2 ** 31 - 1):
            refused(m._h, "T", T_=bad_T)
            refused(m._h, "T with n == 0", n_=0, T_=bad_T)
        refused(m._h, "null xy", a=False)
        refused(m._h, "null out", out=False)
        unwritten()
        # (the same calls with good arguments work; n == 0 is valid with NULL arrays)
        assert f["ground_rollouts"](m._h, None, 0, 1, C.byref(RP()), None) == 0 and f["ground_rollouts_dev"](m._h, None, 0, 4096, C.byref(RP()), None) == 0
        unwritten()
        assert f["ground_rollouts"](m._h, ptr(xy), n, T, C.byref(RP(inflate_sq=1 << 22, flags=1)), ptr(host)) == 0
        rec = host[:48 * n].view(RD)
        assert rec["poses"].tolist() == [3] * 4 and rec["cells"].tolist() == [3, 3, 3, 1] and host[48 * n:].tobytes() == P5A * (4096 - 48 * n)
        m.ground_nf1_compute(_xy(pvt, [(3, 3)]))
        assert f["ground_rollouts"](m._h, ptr(xy), n, T, C.byref(RP(flags=2)), ptr(host)) == 0
        assert rec["nf1_min"].tolist() == [0, 12, 18, 4] and rec["nf1_min_at"].tolist() == [0, 0, 0, 0] and rec["nf1_end"].tolist() == [4, 14, 20, 4]
        m.ground_compute(z, z + 7)                              # a new field: the function is not of it
        refused(m._h, "the NF1 flag after a new ground field", RP(flags=2))
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 7. nothing else is written
def test_section_calls_change_nothing_of_the_map_update():
    size = (48, 40, 16)
    rng = np.random.default_rng(5)
    boxes = []
    for _ in range(40):
        s = rng.integers(3, 10, size=3)
        c = rng.integers((-30, -24, -10), (50, 20, 8))
        boxes.append((c, c + s))

    def frame(k):
        pos, q = scenes.pose(k, W, delta_vox=3, yaw_deg=0.0)
        return pos, q, box_labels(scenes.local_pivot(pos, W, size), size, k, boxes, unknown_slab=3)

    field = {}

    def calls(a, k, phase, pos):
        if phase == "fuse" and k % 2 == 0:                       # a new ground field and function every other frame, between fuse and merge
            field["pvt"] = scenes.local_pivot(pos, W, size)
            a.ground_compute(field["pvt"][2] + 2, field["pvt"][2] + 9, 2, k % 4 == 2)
            a.ground_nf1_compute(_xy(field["pvt"], [(24, 20)]), 0, True)
        if phase in ("fuse", "edt", "merge"):
            r = np.random.default_rng(k)
            xy = _xy(field["pvt"], np.stack([arc(r.uniform(0, 40, 2), r.uniform(0, 6.28), r.uniform(0.3, 2.0), 0.05, 70)[0] for _ in range(30)]))
            a.ground_rollouts(xy, k % 3, 16, k % 2 == 0, True)

    stage_calls_change_nothing(size, (frame(k) for k in range(5)), _mapper, calls, n_probe=2000)


def test_profile_counts_under_ground_query():
    import torch
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.ground_nf1_compute(_xy(pvt, [(3, 3)]))
        m.profile_enable(True)
        m.profile_read()
        xy = _xy(pvt, [[(3, 3), (20, 9)], [(5, 5), (6, 6)]])
        m.ground_rollouts(xy)
        prof = m.profile_read()
        assert prof["ground_query"][1] == 1 and prof["ground_query"][0] > 0
        m.ground_rollouts(xy, 1, 16, True, True)
        d = torch.zeros((256,), dtype=torch.uint8, device="cuda:0")
        dxy = torch.from_numpy(xy).to("cuda:0")
        m.ground_rollouts_dev(dxy.data_ptr(), 2, 2, d.data_ptr(), 0, 0, False, True)
        m.ground_rollouts(np.zeros((0, 2, 2), np.float32))                  # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_query"][1] == 2 and prof["ground_query"][0] > 0
        assert all(v[1] == 0 for k, v in prof.items() if k != "ground_query")
        assert list(prof) == NAMES
    finally:
        m.close()


_TRACE_CHILD = r"""
import sys
import numpy as np
from hooks_py import HooksMapper
import gie
m = HooksMapper(gie.make_config(0.1, (32, 24, 8), fast_mode=False, cutoff_dist=3.0))
for _ in range(2):
    m.set_pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    m.ogm_labels(np.ones((8, 24, 32), np.int8))
    m.step()
pvt = m.pivot()
m.ground_compute(pvt[2], pvt[2] + 7)
xy = ((np.array([[(3, 3), (20, 9), (21, 9)], [(5, 5), (6, 6), (7, 7)]], np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(0.1)).astype(np.float32)
m.ground_nf1_compute(xy[0, :1])
for nf1 in (False, True):
    sys.stderr.write("BEGIN\n"); sys.stderr.flush()
    r = m.ground_rollouts(xy, 1, 16, False, nf1)
    sys.stderr.write("END\n"); sys.stderr.flush()
    assert r["poses"].tolist() == [3, 3]
sys.stderr.write("BEGIN\n"); sys.stderr.flush()
m.ground_rollouts(xy[:0])
sys.stderr.write("END\n"); sys.stderr.flush()
m.close()
"""


def test_a_call_is_two_launches():
    """the launches themselves, named by the test build's launch trace (a switch read once per process: a child process)"""
    import os
    import sys
    env = dict(os.environ, GIE_TRACE_LAUNCHES="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    res = subprocess.run([sys.executable, "-c", _TRACE_CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr)
    calls = [blk.split("END")[0] for blk in res.stderr.split("BEGIN\n")[1:]]
    names = [[ln.split("launch ")[1].strip() for ln in c.splitlines() if "launch " in ln] for c in calls]
    assert names == [["k_glos_prep", "k_ground_rollouts<false>"], ["k_glos_prep", "k_ground_rollouts<true>"], []], names


# ---------------------------------------------------------------------------------------------------------- 8. host layer
def test_host_layer_ground_local_plan_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_local_plan_probe")
    size, w, cutoff, gmin, gmax, min_known, radius = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15
    yaw, dt, T, inflate, v_min, v_max, omega_max = 2.4, 0.25, 20, 0.45, 0.1, 0.8, 1.5       # (the heading of the second goal, the one that can be reached)
    frames, fpath = lidar_frames(tmp_path)
    robot = np.asarray(frames[-1][0][:2], np.float32)
    goal = np.array([[robot[0] + 1.5, robot[1] - 1.0], [robot[0] - 1.4, robot[1] + 1.2]], np.float32)
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    tail = [repr(radius), repr(yaw), repr(dt), str(T), repr(inflate), repr(v_min), repr(v_max), repr(omega_max)] + [repr(float(x)) for x in goal.ravel()]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known)] + tail, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 best " in res.stdout and "poses %d records 81" % (81 * T * 2) in res.stdout, (res.stdout, res.stderr)
    v, omega = np.fromfile(out + ".v", np.float32), np.fromfile(out + ".omega", np.float32)
    poses = np.fromfile(out + ".poses", np.float32).reshape(81, T, 2)
    rec = np.fromfile(out + ".rec", RD)
    best, csq = np.fromfile(out + ".info", np.int32).tolist()
    assert csq == int(np.ceil(np.float32(radius) / np.float32(w))) ** 2 == 4 and len(rec) == 81
    assert np.allclose(v.reshape(9, 9)[:, 0], np.linspace(v_min, v_max, 9), atol=1e-6) and np.allclose(omega.reshape(9, 9)[0], np.linspace(-omega_max, omega_max, 9), atol=1e-6)
    # the poses: numpy's arcs
    k = np.arange(T)[None, :]
    th = yaw + omega.astype(np.float64)[:, None] * np.float64(np.float32(dt)) * k
    d = v.astype(np.float64)[:, None] * np.float64(np.float32(dt))
    want_x = robot[0] + np.concatenate([np.zeros((81, 1)), np.cumsum(d * np.cos(th), 1)[:, :-1]], 1)
    want_y = robot[1] + np.concatenate([np.zeros((81, 1)), np.cumsum(d * np.sin(th), 1)[:, :-1]], 1)
    assert np.abs(poses[:, :, 0] - want_x).max() < 1e-5 and np.abs(poses[:, :, 1] - want_y).max() < 1e-5
    assert np.array_equal(poses[:, 0], np.broadcast_to(robot, (81, 2)))
    # the records: the Mapper's, on those poses
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        assert m.ground_nf1_compute(goal, csq) >= 1
        isq = int(np.ceil(np.float32(inflate) / np.float32(w))) ** 2
        got = m.ground_rollouts(poses, csq, isq, False, True)
        _same(got, Q.rollouts(m.read_ground(), poses, m.pivot(), w, csq, isq, Q.NF1, m.read_ground_nf1()), "the mapper against the reference")
    finally:
        m.close()
    assert rec.tobytes() == got.tobytes()
    # the index: the stated rule
    ok = np.flatnonzero((rec["poses"] >= 2) & (rec["nf1_min"] >= 0))
    want_best = -1 if not len(ok) else int(ok[np.lexsort((ok, rec["cost"][ok], rec["nf1_min"][ok]))[0]])
    assert best == want_best and len(ok) >= 10 and best >= 0 and len(set(rec["nf1_min"][ok].tolist())) > 3
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1"] + tail, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 best -1 poses 3 records 2" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == P5A * 96 and np.fromfile(out + ".poses", np.float32).tolist() == [-7.0] * 3
    assert np.fromfile(out + ".info", np.int32).tolist() == [-1, 4]

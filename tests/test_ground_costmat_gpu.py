"""The ground cost matrix on the device (include/gie.h "ground cost matrix", gie_ground_costmat.inc.h) against the numpy statement of
tests/ground_costmat_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is exact.

A scene is a label plane, the same on every layer (tests/test_ground_frontier_gpu.py says why).  Every case asserts FROM THE
REFERENCE ALONE that it holds what it is about — valid points without a path between them, thousands of levels, duplicates —
before the device is compared.  _check runs the four forms of a call: the host form and the _dev form, each with and without
`valid`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ground_costmat_ref as M
import ground_frontier_ref as F
import ground_nf1_ref as N
import ground_ref as R
import gie
from gie import _capi, scenes
from ground_common import INVALID, POISON, P5A, settle as _settle, plane as _plane, ground as _ground, xy as _xy, framed as _framed, serpentine as _serpentine, chain_scene as _chain_scene
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
LDS_BUDGET = 144 * 1024                                         # bytes of the three bit planes a search keeps in LDS


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _host(m, xy, csq, ut, with_valid):
    """the host form through the raw binding, into poisoned arrays one entry longer than the result"""
    n = len(xy)
    cost = np.full(n * n + 1, POISON, np.int32)
    valid = np.full(n + 1, 0x5a, np.uint8)
    p = m.ground_nf1_param(csq, ut)
    src = xy if n else np.zeros((1, 2), np.float32)
    assert m._f["ground_costmat_compute"](m._h, _ptr(src), n, C.byref(p), _ptr(cost), _ptr(valid) if with_valid else None) == 0
    assert cost[n * n] == POISON and valid[n] == 0x5a
    if not with_valid:
        assert (valid == 0x5a).all()
    return cost[:n * n].reshape(n, n), valid[:n]


def _dev(m, xy, csq, ut, with_valid):
    """the _dev form on the mapper's stream, into poisoned device buffers one entry longer than the result"""
    import torch
    n = len(xy)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(torch.cuda.ExternalStream(m.stream_handle(), device=dev)):
        d_xy = torch.from_numpy(np.concatenate([xy, np.zeros((1, 2), np.float32)])).to(dev)
        d_cost = torch.full((n * n + 1,), POISON, dtype=torch.int32, device=dev)
        d_valid = torch.full((n + 1,), 0x5a, dtype=torch.uint8, device=dev)
        m.ground_costmat_dev(d_xy.data_ptr(), n, d_cost.data_ptr(), d_valid.data_ptr() if with_valid else 0, csq, ut)
    m.sync()
    cost, valid = d_cost.cpu().numpy(), d_valid.cpu().numpy()
    assert cost[n * n] == POISON and valid[n] == 0x5a
    if not with_valid:
        assert (valid == 0x5a).all()
    return cost[:n * n].reshape(n, n), valid[:n]


def _check(m, g, pvt, xy, csq=0, ut=False, forms=4):
    """the reference on the planes g, then Mapper.ground_costmat and the four forms against it; returns the reference's (cost, valid)"""
    xy = np.ascontiguousarray(np.asarray(xy, np.float32).reshape(-1, 2))
    want, ok = M.matrix(g, xy, pvt, W, csq, N.UNKNOWN_TRAVERSABLE if ut else 0)
    cost, valid = m.ground_costmat(xy, csq, ut)
    assert cost.dtype == np.int32 and cost.shape == want.shape and valid.dtype == bool
    assert np.array_equal(valid, ok), (csq, ut, valid, ok)
    assert np.array_equal(cost, want), (csq, ut, int((cost != want).sum()))
    for form, with_valid in [(_dev, True), (_host, False), (_dev, False), (_host, True)][:forms - 1]:
        c, v = form(m, xy, csq, ut, with_valid)
        assert c.tobytes() == want.tobytes(), (form.__name__, with_valid)
        if with_valid:
            assert v.tolist() == ok.astype(np.uint8).tolist(), form.__name__
    return want, ok


def _chain_mapper():
    size = (64, 40, 3)
    m = _mapper(size)
    pvt = _settle(m, _plane(size, _chain_scene(pillars=True)))
    return m, size, pvt, _ground(m, size, (1, 1))


# ---------------------------------------------------------------------------------------------------------- 1. word boundaries
@pytest.mark.parametrize("X", [1, 63, 64, 65, 130])
def test_corridors_across_word_boundaries_and_padding_bits(X):
    """corridors along x between walls: rows 1 and 7 with a wall in the last column, rows 3 and 5 up to the LAST column with a wall
    row between them — a padding bit beyond X that was open would join them behind the wall"""
    size = (X, 9, 2)
    lab = np.full((9, X), 2, np.int8)
    lab[1, :X - 1] = 1
    lab[7, :X - 1] = 1
    lab[3, :] = 1
    lab[5, :] = 1
    cells = [(0, 3), (X - 1, 3), (X - 1, 5), (0, 5), (0, 1), (max(X - 2, 0), 1), (X // 2, 1), (X // 2, 7), (X - 1, 7), (X // 2, 3), (X, 3), (min(63, X - 1), 5),
             (min(64, X - 1), 5)]
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        want, ok = _check(m, g, pvt, _xy(pvt, cells))
        assert ok[:4].all() and not ok[8] and not ok[10]        # (X - 1, 7) is the wall of the last column, (X, 3) is outside
        assert want[0, 1] == X - 1 and want[2, 3] == X - 1 and want[1, 2] == -1 and want[0, 3] == -1     # not joined behind the wall
        assert want[0, 9] == X // 2 and want[11, 12] == (1 if X > 64 else 0) and want[3, 12] == min(64, X - 1)
        if X > 1:
            assert ok[4:8].all() and want[4, 5] == X - 2 and want[4, 7] == -1 and want[6, 0] == -1 and want[4, 6] == X // 2
        else:
            assert not ok[4:8].any()
        _, ok2 = _check(m, g, pvt, _xy(pvt, cells), 2, forms=2)  # no cell is that far from a wall: every point invalid
        assert not ok2.any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. depth, 3. early end
@pytest.mark.parametrize("where", ["spread", "first50"])
def test_a_serpentine_maze_of_thousands_of_levels(where):
    """cost[i][j] is the difference of the points' positions along the one corridor.  "spread": up to 8000 levels.  "first50": all
    points within the first 50 cells, so every search ends early — thousands of levels before a level adds nothing"""
    size = (130, 129, 2)
    lab, cells = _serpentine(size[0], size[1], 2)
    assert len(cells) > 8000
    if where == "spread":
        at = np.array([0, 1, 127, 128, 129, 700, 2047, 2048, 4100, 4100, 6001, len(cells) - 2, len(cells) - 1])
    else:
        at = np.array([0, 3, 7, 7, 20, 49, 31, 1])
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        want, ok = _check(m, g, pvt, _xy(pvt, cells[at]), forms=2)
        assert ok.all() and np.array_equal(want, np.abs(at[:, None] - at[None, :]))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. point counts
def test_point_counts_up_to_the_limit_and_one_beyond():
    import torch
    m, size, pvt, g = _chain_mapper()
    try:
        rng = np.random.default_rng(4)
        cells = np.stack([rng.integers(-2, size[0] + 2, 257), rng.integers(-2, size[1] + 2, 257)], 1)
        xy = _xy(pvt, cells)
        for n in (0, 1, 2, 64, 65, 256):
            want, ok = _check(m, g, pvt, xy[:n], 1 if n == 64 else 0)
            if n >= 64:
                assert 0.5 * n < ok.sum() < n and (want[np.ix_(ok, ok)] == -1).any() and (want > 20).any()
        # 257 points: refused, nothing written
        cost = np.full(257 * 257, POISON, np.int32)
        valid = np.full(257, 0x5a, np.uint8)
        dbuf = torch.full((257 * 257,), POISON, dtype=torch.int32, device="cuda:0")
        p = m.ground_nf1_param(0)
        assert m._f["ground_costmat_compute"](m._h, _ptr(xy), 257, C.byref(p), _ptr(cost), _ptr(valid)) == INVALID
        assert m._f["ground_costmat_compute_dev"](m._h, C.c_void_p(dbuf.data_ptr()), 257, C.byref(p), C.c_void_p(dbuf.data_ptr()), C.c_void_p(dbuf.data_ptr())) == INVALID
        m.sync()
        assert (cost == POISON).all() and (valid == 0x5a).all() and bool((dbuf == POISON).all())
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. points
def test_points_ties_outside_not_finite_in_obstacles_and_on_one_cell():
    m, size, pvt, g = _chain_mapper()
    try:
        rng = np.random.default_rng(5)
        cells = np.stack([rng.integers(-3, size[0] + 3, 40), rng.integers(-3, size[1] + 3, 40)], 1)
        odd = np.array([[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [1e30, 0.0], [0.0, -3e9], [3e9, 3e9]], np.float32)
        walls = np.argwhere(g["type"] == R.OCCUPIED)[::37][:6, ::-1]
        twins = np.array([(24, 20), (24, 20), (10, 30), (24, 20)])
        sets = {"centres": _xy(pvt, cells), "ties": _xy(pvt, cells, 0.5), "outside": _xy(pvt, [(-1, 0), (size[0], 3), (5, -1), (5, size[1])]),
                "odd": odd, "walls": _xy(pvt, walls), "twins": _xy(pvt, twins), "never seen": _xy(pvt, [(12, 25), (35, 30), (45, 9)])}
        sets["all"] = np.concatenate(list(sets.values()))
        sets["invalid"] = np.concatenate([sets["outside"], odd, sets["walls"]])
        out = {}
        for name, xy in sets.items():
            for csq, ut in ((0, False), (4, False), (0, True), (9, True)) if name == "all" else ((0, False),):
                out[name, csq, ut] = _check(m, g, pvt, xy, csq, ut, forms=4 if name in ("all", "invalid") else 2)
        assert out["centres", 0, False][1].sum() > 20 and out["ties", 0, False][1].sum() > 20
        assert N.cells_of(sets["centres"], pvt, W, g["type"].shape) != N.cells_of(sets["ties"], pvt, W, g["type"].shape)      # (a tie rounds up: another cell)
        cost, ok = out["invalid", 0, False]
        assert len(ok) == 16 and not ok.any() and (cost == -1).all()
        cost, ok = out["twins", 0, False]
        assert ok.all() and cost[0, 1] == cost[0, 3] == 0 and np.array_equal(cost[0], cost[1]) and np.array_equal(cost[1], cost[3]) and cost[0, 2] == 24
        a, b = out["all", 0, False], out["all", 0, True]
        assert b[1].sum() > a[1].sum() and a[1].sum() > out["all", 4, False][1].sum() > 10       # the never-seen cells open; clearance closes
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. the definition, NF1 survives
def test_a_column_is_ground_nf1_of_that_goal_and_the_current_field_survives():
    m, size, pvt, g = _chain_mapper()
    try:
        rng = np.random.default_rng(6)
        cells = np.stack([rng.integers(-1, size[0] + 1, 48), rng.integers(-1, size[1] + 1, 48)], 1)
        cells[7] = (45, 9)                                      # the never-seen cell in the closed room
        cells[8], cells[9], cells[10] = (44, 9), (48, 11), (42, 7)     # and free cells of that room
        xy = _xy(pvt, cells)
        xy[11] = np.nan
        for csq, ut in ((0, False), (2, True)):
            cost, valid = m.ground_costmat(xy, csq, ut)
            cols = [int(np.flatnonzero(valid)[0]), 8, 11, int(np.flatnonzero(~valid)[-1])]
            assert valid[8] and not valid[11] and valid[7] == ut
            for j in cols:
                n_src = m.ground_nf1_compute(xy[j:j + 1], csq, ut)
                assert n_src == int(valid[j])
                steps = m.ground_nf1_query(xy)
                assert np.array_equal(steps, cost[:, j]), (csq, ut, j)
            assert (cost[:, 8] > 0).sum() >= 2 and (cost[valid, 8] == -1).sum() > 10     # the room is closed
        # a field computed before the matrix reads back unchanged and is still valid after it; so are the frontier clusters
        m.ground_nf1_compute(_xy(pvt, [(24, 20)]), 1)
        before = m.read_ground_nf1()
        m.ground_frontier_compute(1, 2, 8, 12)
        rec = m.read_ground_frontier_clusters()[0].tobytes()
        for csq, ut in ((0, False), (4, True), (1, False)):
            _check(m, g, pvt, xy, csq, ut, forms=3)
        assert np.array_equal(m.read_ground_nf1(), before) and (before >= 0).sum() > 1000
        assert np.array_equal(m.ground_nf1_query(xy[:5]), F.gather(before, xy[:5], pvt, W))
        assert m.read_ground_frontier_clusters()[0].tobytes() == rec and len(rec) >= 4 * 64
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. both storage forms
@pytest.mark.parametrize("size,in_lds", [((512, 768, 1), True), ((512, 769, 1), False)])
def test_a_maze_in_each_storage_form(size, in_lds):
    """three bit planes of 8 * ceil(X / 64) * Y bytes: exactly the LDS budget, and one row more — there every source has a pair of
    planes of its own in global memory, and eight searches that shared one would not give eight different rows"""
    assert (3 * 8 * ((size[0] + 63) // 64) * size[1] <= LDS_BUDGET) == in_lds
    lab, cells = _serpentine(size[0], size[1], 24)
    lab[727:740, 5] = 1                                         # a pocket between two rows of the corridor without a way into it, and a point in it
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        at = np.array([0, 509, 510, 5000, 5000, 12345, len(cells) - 1])
        pts = np.concatenate([cells[at], [(5, 730), (0, 0)]])
        want, ok = _check(m, g, pvt, _xy(pvt, pts), forms=2)
        assert ok[:8].all() and not ok[8] and len(cells) > 16000
        assert np.array_equal(want[:7, :7], np.abs(at[:, None] - at[None, :])) and (want[7, :7] == -1).all() and want[7, 7] == 0
        _check(m, g, pvt, _xy(pvt, pts[[7, 0]]), forms=2)       # fewer points than the planes were sized for
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. the frontier chain
def test_the_frontier_chain_with_one_sync():
    import torch
    m, size, pvt, g = _chain_mapper()
    try:
        cap, csq = 12, 1
        fr = F.clusters(g, csq, 8, 2, cap, pvt, W)
        have = fr["n_clusters"]
        assert 4 <= have < cap
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        n = cap + 1
        for robot, blocked in (((24, 18), False), ((40, 8), True), ((3, 3), False)):       # free space; inside a wall; free space
            robot_xy = _xy(pvt, [robot])
            pts = np.concatenate([robot_xy, fr["goals"]])
            want, ok = M.matrix(g, pts, pvt, W, csq)
            steps_want = F.route_steps(g, robot_xy, fr["goals"], pvt, W, csq)
            assert ok[0] != blocked and ok[1:1 + have].all() and not ok[1 + have:].any()
            with torch.cuda.stream(st):
                d_pts = torch.full((2 * n,), 7.0, dtype=torch.float32, device=dev)
                d_pts[:2] = torch.from_numpy(robot_xy[0]).to(dev)
                d_cost = torch.full((n * n,), POISON, dtype=torch.int32, device=dev)
                d_valid = torch.full((n,), 0x5a, dtype=torch.uint8, device=dev)
                d_steps = torch.full((cap,), POISON, dtype=torch.int32, device=dev)
                m.ground_frontier_compute_dev(csq, 2, 8, cap)
                m.read_ground_frontier_clusters_dev(0, d_pts.data_ptr() + 8, 0)            # the goal array directly behind the robot
                m.ground_costmat_dev(d_pts.data_ptr(), n, d_cost.data_ptr(), d_valid.data_ptr(), csq)
                m.ground_nf1_compute_dev(d_pts.data_ptr(), 1, csq)                        # ground_exploration_goals' two calls
                m.ground_nf1_query_dev(d_pts.data_ptr() + 8, cap, d_steps.data_ptr())
            m.sync()                                            # the only wait
            cost = d_cost.cpu().numpy().reshape(n, n)
            assert np.array_equal(d_pts.cpu().numpy().reshape(-1, 2), pts, equal_nan=True)
            assert np.array_equal(cost, want) and d_valid.cpu().numpy().tolist() == ok.astype(np.uint8).tolist()
            assert (cost[1 + have:] == -1).all() and (cost[:, 1 + have:] == -1).all()     # the NaN tail
            steps = d_steps.cpu().numpy()
            assert np.array_equal(steps, steps_want) and np.array_equal(cost[0, 1:], steps) and np.array_equal(cost[1:, 0], steps)
            assert (steps == -1).all() if blocked else (steps[:have] >= 0).sum() == have - 1
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 9. the update does not notice
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

    seen = []
    prng = np.random.default_rng(9)

    def calls(a, k, phase, pos):
        pvt = scenes.local_pivot(pos, W, size)
        pts = _xy(pvt, np.stack([prng.integers(0, size[0], 20), prng.integers(0, size[1], 20)], 1))
        if phase == "fuse":                                      # between fuse and merge
            a.ground_compute(pvt[2] + 2, pvt[2] + 9, 2, k % 2 == 1)
            cost, valid = a.ground_costmat(pts, k % 3, k % 2 == 0)
            seen.append(int((cost > 0).sum()))
        elif phase == "merge":                                   # after the update
            a.ground_compute(pvt[2] + 1, pvt[2] + 14)
            cost, valid = a.ground_costmat(pts, 4)
            seen.append(int((cost > 0).sum()))
    stage_calls_change_nothing(size, (frame(k) for k in range(6)), _mapper, calls, n_probe=2000)
    assert len(seen) == 12 and sum(n > 0 for n in seen) >= 6


# ---------------------------------------------------------------------------------------------------------- 10. refusals, profile
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 3)
    m, fresh, t = _mapper(size), _mapper(size), _mapper(size)
    try:
        lab = _framed(size[0], size[1])
        pvt = _settle(m, _plane(size, lab))
        f = m._f
        xy = _xy(pvt, [(3, 3), (9, 9)])
        cost = np.full(16, POISON, np.int32)
        valid = np.full(8, 0x5a, np.uint8)
        dbuf = torch.full((64,), POISON, dtype=torch.int32, device="cuda:0")
        dp = C.c_void_p(dbuf.data_ptr())

        def P(**kw):
            p = _capi.GroundNf1Param()
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert (cost == POISON).all() and (valid == 0x5a).all() and bool((dbuf == POISON).all())

        def both(h, who, p="default", n=2, hx=True, hc=True):
            p = P() if p == "default" else p
            pp = C.byref(p) if p is not None else None
            assert f["ground_costmat_compute"](h, _ptr(xy) if hx else None, n, pp, _ptr(cost) if hc else None, _ptr(valid)) == INVALID, who
            assert f["ground_costmat_compute_dev"](h, dp if hx else None, n, pp, dp if hc else None, dp) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "before a ground field exists"), (fresh._h, "fresh")):
            both(h, who)
        t.set_tile((8, 0, 0), (64, 24, 3))                      # a tiled mapper
        both(t._h, "tiled")
        unwritten()
        m.ground_compute(pvt[2] + 1, pvt[2] + 1)
        bad = [P(clearance_sq=-1), P(clearance_sq=-2 ** 31), P(flags=2), P(flags=3), P(flags=4), P(flags=-2 ** 31)] + [P(reserved=i) for i in range(6)]
        for p in bad:
            both(m._h, (p.clearance_sq, p.flags, list(p.reserved)), p)
        both(m._h, "null parameters", None)
        both(m._h, "n < 0", n=-1)
        both(m._h, "n beyond the limit", n=257)
        both(m._h, "no points", hx=False)
        both(m._h, "no matrix", hc=False)
        unwritten()
        # n == 0 writes nothing whatever the pointers are; the same calls with good arguments work
        assert f["ground_costmat_compute"](m._h, None, 0, C.byref(P()), None, None) == 0
        assert f["ground_costmat_compute_dev"](m._h, None, 0, C.byref(P()), None, None) == 0
        assert f["ground_costmat_compute"](m._h, _ptr(xy), 0, C.byref(P()), _ptr(cost), _ptr(valid)) == 0
        assert f["ground_costmat_compute_dev"](m._h, dp, 0, C.byref(P()), dp, dp) == 0
        unwritten()
        assert f["ground_costmat_compute"](m._h, _ptr(xy), 2, C.byref(P(flags=1)), _ptr(cost), _ptr(valid)) == 0
        assert cost[:4].tolist() == [0, 12, 12, 0] and (cost[4:] == POISON).all() and valid[:2].tolist() == [1, 1] and (valid[2:] == 0x5a).all()
    finally:
        for x in (m, fresh, t):
            x.close()


def test_profile_counts_under_ground_nf1_and_adds_no_name():
    m, size, pvt, g = _chain_mapper()
    try:
        xy = _xy(pvt, [(24, 20), (3, 3), (50, 30)])
        m.profile_enable(True)
        before = m.profile_read()
        m.ground_costmat(xy)
        _dev(m, xy, 0, False, True)
        m.ground_costmat(np.zeros((0, 2), np.float32))          # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert list(prof) == list(before) and not any("costmat" in k and "ground" in k for k in prof)
        assert prof["ground_nf1"][1] == 2 and prof["ground_nf1"][0] > 0
        assert all(prof[k][1] == 0 for k in prof if k != "ground_nf1")
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 11. at size
def test_at_size_512x512x24_with_64_points_twice():
    size = (512, 512, 24)
    rng = np.random.default_rng(512)
    boxes = [(lo, lo + s) for lo, s in zip(np.stack([rng.integers(-250, 250, 300), rng.integers(-250, 250, 300), rng.integers(-14, 10, 300)], 1),
                                           rng.integers(2, 12, (300, 3)))]
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, W, size)
        lab = box_labels(pvt, size, 0, boxes, unknown_slab=6)
        assert tuple(_settle(m, lab, pos)) == tuple(pvt)
        m.ground_compute(pvt[2] + 4, pvt[2] + 15, 3)
        g = m.read_ground()
        free = np.argwhere((g["type"] == R.FREE) & (g["dist_sq"] >= 9))
        cells = np.concatenate([free[rng.choice(len(free), 56, replace=False)][:, ::-1], np.stack([rng.integers(0, 512, 8), rng.integers(0, 512, 8)], 1)])
        xy = _xy(pvt, cells)
        want, ok = _check(m, g, pvt, xy, 9, forms=2)
        assert len(xy) == 64 and ok.sum() >= 56 and want.max() > 400 and (want[np.ix_(ok, ok)] >= 0).mean() > 0.3
        again = m.ground_costmat(xy, 9)
        assert again[0].tobytes() == want.tobytes()             # bit-identical from run to run
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 12. host layer
def test_host_layer_ground_exploration_costs_matches_the_mapper(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = build_host_probe(tmp_path, "ground_tour_probe", ["-DGIE_HOST_WITH_HIP", "-I" + os.path.join(rocm, "include"), "-Wno-unused-result",
                                                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    size, w, cutoff, gmin, gmax, min_known, radius, cap, min_size = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15, 24, 2
    frames, fpath = lidar_frames(tmp_path)
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        g = m.read_ground()
        pvt = m.pivot()
        csq = int(np.ceil(np.float32(radius) / np.float32(w))) ** 2
        assert csq == 4
        n_kept, n_cells = m.ground_frontier_compute(csq, min_size, 8, cap)
        _, goals, _ = m.read_ground_frontier_clusters()
        fr = F.clusters(g, csq, 8, min_size, cap, pvt, w)
        assert np.array_equal(goals, fr["goals"], equal_nan=True) and n_kept == fr["n_clusters"] >= 2
        robot = np.array([frames[-1][0][:2]], np.float32)
        pts = np.concatenate([robot, goals])
        want, ok = _check(m, g, pvt, pts, csq, forms=2)
        assert ok[0] and (want[0, 1:] >= 0).any() and np.array_equal(want[0, 1:], F.route_steps(g, robot, goals, pvt, w, csq))
    finally:
        m.close()
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), repr(radius), str(cap), str(min_size)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 cost %d goals %d" % ((cap + 1) ** 2, 2 * (cap + 1)) in res.stdout, (res.stdout, res.stderr)
    assert np.array_equal(np.fromfile(out + ".goals", np.float32).reshape(-1, 2), pts, equal_nan=True)
    assert np.fromfile(out + ".cost", np.int32).tobytes() == want.tobytes()
    assert np.fromfile(out + ".info", np.int32).tolist() == [n_kept, n_cells, csq]
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", repr(radius), str(cap), str(min_size)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 cost 3 goals 2" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".cost", np.uint8).tobytes() == P5A * 12 and np.fromfile(out + ".goals", np.float32).tolist() == [-7.0, -7.0]
    assert np.fromfile(out + ".info", np.int32).tolist() == [0, 0, csq]

"""tests/ground_rollout_ref.py (the numpy statement of include/gie.h "ground rollouts") against a second statement that shares nothing
with it but ground_los_ref.line — its own mapping of a pose to a cell, its own blocked rule, one cell at a time with running values —
on hand-made 9 x 9 and 70 x 9 planes, and the section's declarations in the header, the binding and the host layer.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

import gie
import ground_los_ref as L
import ground_ref as R
import ground_rollout_ref as Q
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
U, F, O, T_ = R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT
PVT = (-7, 40, 0)
INFLATE = (0, 1, 9, 1 << 22)


def _plane(shape=(9, 9), walls=(), unknown=(), fnt=()):
    """{"type", "dist_sq"} [Y][X]: dist_sq = the exact squared distance to the nearest wall cell, -1 everywhere without one"""
    Y, X = shape
    t = np.full((Y, X), F, np.int8)
    for (x, y) in unknown:
        t[y, x] = U
    for (x, y) in fnt:
        t[y, x] = T_
    for (x, y) in walls:
        t[y, x] = O
    d = np.full((Y, X), -1, np.int32)
    if len(walls):
        w = np.asarray(walls)
        xs, ys = np.arange(X)[None, :, None], np.arange(Y)[:, None, None]
        d = ((xs - w[:, 0]) ** 2 + (ys - w[:, 1]) ** 2).min(axis=2).astype(np.int32)
    return {"type": t, "dist_sq": d}


def _xy(cells, shift=0.0):
    """world points (float32 metres) of local cells: (cell + pvt + shift) * w, the product in float32"""
    c = np.asarray(cells, np.float64) + np.array(PVT[:2])
    return ((c.astype(np.float32) + np.float32(shift)) * np.float32(W)).astype(np.float32)


def _cell(p, shape):
    """the second statement's own mapping: floorf(p / w + 0.5f) - pvt per axis; None without a cell"""
    out = []
    for k in range(2):
        v = np.float32(p[k])
        if np.isnan(v) or np.isinf(v):
            return None
        u = float(np.floor(v / np.float32(W) + np.float32(0.5)))
        if not -1.0e9 <= u <= 1.0e9:
            return None
        out.append(int(u) - PVT[k])
    return (out[0], out[1]) if 0 <= out[0] < shape[1] and 0 <= out[1] < shape[0] else None


def _second(f, xy, clearance_sq, inflate_sq, flags, nf):
    """the second statement: per trajectory a loop over the poses, per pose a loop over its leg's cells; a leg counts when all of it is clear"""
    t, d = f["type"], f["dist_sq"]
    out = np.zeros(len(xy), Q.ROLLOUT_DTYPE)
    for i, tr in enumerate(xy):
        end, m, hit, cells, lo, cost, prev = 0, 0, (0, 0), 0, None, 0, None
        n_end, n_min, n_at = -1, -1, -1
        for k in range(len(tr)):
            c = _cell(tr[k], t.shape)
            if c is None:
                end = 2
                break
            leg_cells, leg_lo, leg_cost, stop = 0, None, 0, False
            for (x, y) in ([c] if prev is None else L.line(prev, c)[1:]):
                ty, dv = int(t[y, x]), int(d[y, x])
                is_open = ty == F or ty == T_ or (ty == U and (flags & 1) != 0)
                if not (is_open and (dv == -1 or dv >= clearance_sq)):
                    end, hit, stop = 1, (x + PVT[0], y + PVT[1]), True
                    break
                leg_cells += 1
                leg_lo = dv if leg_lo is None or dv < leg_lo else leg_lo
                if dv != -1 and dv < inflate_sq:
                    leg_cost += inflate_sq - dv
            if stop:
                break
            cells, cost, m, prev = cells + leg_cells, cost + leg_cost, m + 1, c
            if leg_lo is not None:
                lo = leg_lo if lo is None or leg_lo < lo else lo
            if flags & 2:
                n_end = int(nf[c[1], c[0]])
                if n_end >= 0 and (n_min < 0 or n_end < n_min):
                    n_min, n_at = n_end, k
        if not flags & 2:
            n_end = n_min = n_at = -2
        out[i] = (end, m, hit, cells, 0 if lo is None else lo, cost, n_end, n_min, n_at, 0)
    return out


def _both(f, xy, clearance_sq=0, flags=0, nf=None):
    """the records of both statements for every inflate_sq of the issue, equal byte for byte: {inflate_sq: records}"""
    xy = np.asarray(xy, np.float32)
    res = {}
    for inf in INFLATE:
        a = Q.rollouts(f, xy, PVT, W, clearance_sq, inf, flags, nf)
        b = _second(f, xy, clearance_sq, inf, flags, nf)
        for key in a.dtype.names:
            assert np.array_equal(a[key], b[key]), (key, inf, a[key].tolist(), b[key].tolist())
        assert a.tobytes() == b.tobytes() and a.dtype == Q.ROLLOUT_DTYPE
        res[inf] = a
    for inf in INFLATE[1:]:                                    # inflate_sq changes the cost alone
        for key in a.dtype.names:
            assert key == "cost" or np.array_equal(res[inf][key], res[0][key])
    assert (res[0]["cost"] == 0).all()
    return res


def _rec(r):
    return [int(r["end"]), int(r["poses"]), r["hit"].tolist(), int(r["cells"]), int(r["min_dist_sq"]), int(r["cost"])]


def _nf_field(shape, seed=0):
    """a hand-made field: values 0 .. 5 (many ties) with a third of the cells unreachable"""
    rng = np.random.default_rng(seed)
    nf = rng.integers(0, 6, shape).astype(np.int32)
    nf[rng.random(shape) < 0.33] = -1
    return nf


def test_constants_and_dtype_are_the_mappers():
    assert (U, F, O, T_) == (gie.VOX_UNKNOWN, gie.VOX_FREE, gie.VOX_OCCUPIED, gie.VOX_FNT)
    assert Q.ROLLOUT_DTYPE == gie.GROUND_ROLLOUT_DTYPE and Q.ROLLOUT_DTYPE.itemsize == 48
    assert Q.UNKNOWN_TRAVERSABLE == gie.GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE == 1 and Q.NF1 == gie.GROUND_ROLLOUT_NF1 == 2
    assert Q.MAX_POSES == gie.GROUND_ROLLOUT_MAX_POSES == 4096


def test_a_one_cell_wall_between_two_poses_is_found():
    f = _plane(walls=[(4, y) for y in range(9)])
    xy = _xy([[(2, 4), (6, 4), (7, 4)], [(1, 1), (3, 7), (3, 8)], [(0, 0), (3, 0), (8, 3)], [(6, 2), (2, 6), (2, 7)]])
    res = _both(f, xy)
    r = res[9]
    # both poses of the leg are FREE cells with the wall between them: the leg is blocked at the wall's cell
    assert _rec(r[0]) == [1, 1, [4 + PVT[0], 4 + PVT[1]], 1, 4, 5]
    assert _rec(r[1])[:4] == [0, 3, [0, 0], len(set(L.line((1, 1), (3, 7)) + [(3, 8)]))] and r[1]["min_dist_sq"] == 1
    assert _rec(r[2])[:3] == [1, 2, [4 + PVT[0], 0 + PVT[1]]] and r[2]["cells"] == 4
    assert r[3]["end"] == 1 and r[3]["poses"] == 1 and r[3]["hit"].tolist() == [4 + PVT[0], 4 + PVT[1]]
    assert res[1 << 22][0]["cost"] == (1 << 22) - 4 and res[1][0]["cost"] == 0
    # with a clearance the prefix ends earlier: the cell beside the wall is blocked
    r = _both(f, xy, clearance_sq=4)[9]
    assert _rec(r[0]) == [1, 1, [3 + PVT[0], 4 + PVT[1]], 1, 4, 5]
    assert _rec(r[1])[:4] == [1, 1, [3 + PVT[0], 6 + PVT[1]], 1]             # (1,1) (1,2) (2,3) (2,4) (2,5) (3,6): beside the wall


def test_the_tie_rule_slips_through_a_corner_gap():
    f = _plane(walls=[(3, 4), (4, 3)])
    xy = _xy([[(2, 2), (5, 5)], [(2, 2), (5, 4)], [(5, 5), (2, 2)], [(3, 3), (4, 4)]])
    r = _both(f, xy)[9]
    assert L.line((2, 2), (5, 5)) == [(2, 2), (3, 3), (4, 4), (5, 5)]
    assert _rec(r[0]) == [0, 2, [0, 0], 4, 1, 4 + 8 + 8 + 4] and _rec(r[2]) == _rec(r[0]) and _rec(r[3])[:4] == [0, 2, [0, 0], 2]
    assert r[1]["end"] == 1 and r[1]["hit"].tolist() in ([4 + PVT[0], 3 + PVT[1]], [3 + PVT[0], 4 + PVT[1]])
    # with clearance_sq 2 the cells beside the two walls are blocked themselves
    r = _both(f, xy, clearance_sq=2)[9]
    assert _rec(r[0])[:3] == [1, 1, [3 + PVT[0], 3 + PVT[1]]]


def test_pose_0_blocked_outside_or_not_finite():
    f = _plane(walls=[(4, 4)], unknown=[(1, 1)])
    nf = _nf_field((9, 9))
    xy = _xy([[(4, 4), (5, 5), (6, 6)], [(-1, 0), (0, 0), (1, 0)], [(9, 8), (8, 8), (7, 8)], [(3, 9), (3, 8), (3, 7)], [(1, 1), (2, 1), (3, 1)],
              [(2, 2), (2, 3), (2, 4)], [(2, 2), (2, 3), (2, 4)], [(2, 2), (2, 3), (2, 4)], [(2, 2), (2, 3), (2, 4)], [(2, 2), (2, 3), (2, 4)]])
    xy[5, 0, 0] = np.nan
    xy[6, 0, 1] = np.inf
    xy[7, 0, 0] = -np.inf
    xy[8, 0, 1] = 1e30
    xy[9, 0, 0] = -1e30
    for flags in (0, Q.NF1):
        r = _both(f, xy, 0, flags, nf)[9]
        none = -1 if flags else -2
        assert _rec(r[0]) == [1, 0, [4 + PVT[0], 4 + PVT[1]], 0, 0, 0]          # pose 0 blocked: hit is c_0 itself
        assert _rec(r[4]) == [1, 0, [1 + PVT[0], 1 + PVT[1]], 0, 0, 0]          # (an UNKNOWN cell without the flag)
        for i in (1, 2, 3, 5, 6, 7, 8, 9):
            assert _rec(r[i]) == [2, 0, [0, 0], 0, 0, 0], i
        assert all([int(q["nf1_end"]), int(q["nf1_min"]), int(q["nf1_min_at"])] == [none] * 3 for q in r)
    r = _both(f, xy, 0, Q.UNKNOWN_TRAVERSABLE)[9]
    assert _rec(r[4])[:4] == [0, 3, [0, 0], 3]


def test_nan_in_the_middle_and_at_the_end_and_far_values():
    f = _plane(walls=[(8, 8)])
    base = [(1, 1), (2, 1), (3, 2), (4, 2), (5, 3)]
    xy = np.stack([_xy(base)] * 7)
    xy[0, 2, 0] = np.nan
    xy[1, 4, 1] = np.nan                                        # T - 1
    xy[2, 3] = np.inf
    xy[3, 1, 0] = -np.inf
    xy[4, 4, 0] = 1e30
    xy[5, 2:] = np.nan                                          # a NaN tail: a rollout of two poses
    r = _both(f, xy)[9]
    assert [(int(q["end"]), int(q["poses"]), int(q["cells"])) for q in r] == [(2, 2, 2), (2, 4, 4), (2, 3, 3), (2, 1, 1), (2, 4, 4), (2, 2, 2), (0, 5, 5)]
    assert (r["hit"] == 0).all()


def test_repeated_poses_and_a_polyline_that_crosses_itself():
    f = _plane(walls=[(0, 8)])
    xy = _xy([[(2, 2), (2, 2), (3, 2), (3, 2), (3, 2), (2, 2)], [(0, 3), (6, 3), (3, 3), (3, 0), (3, 6), (3, 6)]])
    res = _both(f, xy)
    r = res[1 << 22]
    assert _rec(r[0])[:4] == [0, 6, [0, 0], 3]                  # (2,2) (3,2) (2,2): equal consecutive cells add nothing
    # 7 cells to the right, 3 back over them, 3 down, 6 up over those and the crossing: 19, of 13 different cells
    assert _rec(r[1])[:4] == [0, 6, [0, 0], 19]
    cells = L.line((0, 3), (6, 3)) + L.line((6, 3), (3, 3))[1:] + L.line((3, 3), (3, 0))[1:] + L.line((3, 0), (3, 6))[1:]
    assert len(cells) == 19 and len(set(cells)) == 13
    assert r[1]["cost"] == sum((1 << 22) - int(f["dist_sq"][y, x]) for x, y in cells)
    assert r[1]["min_dist_sq"] == min(int(f["dist_sq"][y, x]) for x, y in cells)
    assert res[9][1]["cost"] == sum(max(0, 9 - int(f["dist_sq"][y, x])) for x, y in cells)


def test_one_pose():
    f = _plane(walls=[(4, 4)])
    nf = _nf_field((9, 9), 3)
    xy = _xy([[(0, 0)], [(4, 4)], [(5, 4)], [(9, 0)], [(8, 8)]])
    xy = np.concatenate([xy, np.full((1, 1, 2), np.nan, np.float32)])
    r = _both(f, xy, 0, Q.NF1, nf)[9]
    assert [(int(q["end"]), int(q["poses"]), int(q["cells"])) for q in r] == [(0, 1, 1), (1, 0, 0), (0, 1, 1), (2, 0, 0), (0, 1, 1), (2, 0, 0)]
    assert r[2]["cost"] == 8 and r[2]["min_dist_sq"] == 1 and r[0]["nf1_end"] == nf[0, 0] and r[4]["nf1_end"] == nf[8, 8]


def test_a_field_without_an_obstacle_column():
    f = _plane(unknown=[(5, 5)])
    assert (f["dist_sq"] == -1).all()
    xy = _xy([[(0, 0), (8, 8)], [(8, 0), (0, 8)], [(0, 4), (8, 4)]])
    for clearance_sq in (0, 9, 1 << 20):                        # every clearance passes
        res = _both(f, xy, clearance_sq)
        for inf in INFLATE:
            r = res[inf]
            assert (r["cost"] == 0).all() and r["min_dist_sq"].tolist() == [-1, -1, -1]
        assert _rec(res[9][0])[:3] == [1, 1, [5 + PVT[0], 5 + PVT[1]]] and _rec(res[9][2])[:4] == [0, 2, [0, 0], 9]
    assert _rec(_both(f, xy, 4, Q.UNKNOWN_TRAVERSABLE)[9][0])[:4] == [0, 2, [0, 0], 9]


def test_unknown_cells_with_and_without_the_flag():
    f = _plane(walls=[(0, 0)], unknown=[(x, 5) for x in range(9)], fnt=[(x, 4) for x in range(9)])
    xy = _xy([[(4, 2), (4, 4), (4, 8)], [(0, 5), (1, 5), (2, 5)], [(2, 3), (6, 3), (6, 4)]])
    r0, r1 = _both(f, xy)[9], _both(f, xy, 0, Q.UNKNOWN_TRAVERSABLE)[9]
    assert _rec(r0[0])[:4] == [1, 2, [4 + PVT[0], 5 + PVT[1]], 3] and _rec(r1[0])[:4] == [0, 3, [0, 0], 7]
    assert _rec(r0[1])[:3] == [1, 0, [0 + PVT[0], 5 + PVT[1]]] and _rec(r1[1])[:4] == [0, 3, [0, 0], 3]
    assert r0[2].tobytes() == r1[2].tobytes() and r0[2]["end"] == 0             # FNT cells are open either way
    # their dist_sq still decides
    r2 = _both(f, xy, 30, Q.UNKNOWN_TRAVERSABLE)[9]
    assert _rec(r2[1])[:3] == [1, 0, [0 + PVT[0], 5 + PVT[1]]] and _rec(r2[0])[:3] == [1, 0, [4 + PVT[0], 2 + PVT[1]]]


def test_nf1_values_skip_unreachable_poses_and_the_first_of_a_tie_wins():
    f = _plane(walls=[(8, 0)])
    nf = np.full((9, 9), -1, np.int32)
    nf[2, :] = [-1, 7, -1, 5, 5, -1, 5, 9, -1]
    cells = [(x, 2) for x in range(9)]
    xy = np.stack([_xy(cells), _xy(cells[::-1]), _xy(cells), _xy([(0, 2)] * 9), _xy([(x, 6) for x in range(9)])])
    xy[2, 6:] = np.nan
    r = _both(f, xy, 0, Q.NF1, nf)[9]
    assert [int(r[0][k]) for k in ("poses", "nf1_end", "nf1_min", "nf1_min_at")] == [9, -1, 5, 3]        # 5 at poses 3, 4 and 6
    assert [int(r[1][k]) for k in ("poses", "nf1_end", "nf1_min", "nf1_min_at")] == [9, -1, 5, 2]
    assert [int(r[2][k]) for k in ("end", "poses", "nf1_end", "nf1_min", "nf1_min_at")] == [2, 6, -1, 5, 3]
    assert [int(r[3][k]) for k in ("poses", "nf1_end", "nf1_min", "nf1_min_at")] == [9, -1, -1, -1]      # no value >= 0 at all
    assert [int(r[4][k]) for k in ("poses", "nf1_end", "nf1_min", "nf1_min_at")] == [9, -1, -1, -1]
    nf[2, 8] = 0
    r = _both(f, xy, 0, Q.NF1, nf)[9]
    assert [int(r[0][k]) for k in ("nf1_end", "nf1_min", "nf1_min_at")] == [0, 0, 8] and [int(r[1][k]) for k in ("nf1_end", "nf1_min", "nf1_min_at")] == [-1, 0, 0]
    # a prefix that a wall ends: the values behind it do not count
    f2 = _plane(walls=[(5, y) for y in range(9)])
    r = _both(f2, xy, 0, Q.NF1, nf)[9]
    assert [int(r[0][k]) for k in ("end", "poses", "nf1_end", "nf1_min", "nf1_min_at")] == [1, 5, 5, 5, 3]
    # without the flag: -2 in all three, everything else the same
    r2 = _both(f2, xy, 0, 0, nf)[9]
    assert (r2["nf1_end"] == -2).all() and (r2["nf1_min"] == -2).all() and (r2["nf1_min_at"] == -2).all()
    for key in ("end", "poses", "hit", "cells", "min_dist_sq", "cost"):
        assert np.array_equal(r[key], r2[key])


def test_70x9_planes_past_the_first_chunk_of_64_poses():
    walls = [(64, y) for y in range(9) if y != 7] + [(30, 0), (31, 8)]
    f = _plane((9, 70), walls=walls, unknown=[(50, y) for y in range(3)])
    nf = _nf_field((9, 70), 5)
    row = lambda y, x0, x1: [(x, y) for x in range(x0, x1)]     # noqa: E731
    trajs = [row(4, 0, 70),                                     # blocked in leg 64: lane 0 of the second chunk
             row(7, 0, 70),                                     # through the gap: complete, 70 poses
             row(4, 1, 70) + [(69, 4)],                         # blocked in leg 63: lane 63 of the first chunk
             [(x, 7) for x in range(0, 140, 2)],                # leaves the field behind x = 68
             [(20 + x // 2, 1) for x in range(70)],             # half steps: repeated cells, blocked at the UNKNOWN column
             [(35 + (k % 2) * 20, 3 + (k % 3)) for k in range(70)]]                # back and forth over its own cells
    xy = np.stack([_xy(t) for t in trajs])
    for flags in (0, Q.NF1, Q.NF1 | Q.UNKNOWN_TRAVERSABLE):
        for clearance_sq in (0, 2):
            res = _both(f, xy, clearance_sq, flags, nf)
    r = _both(f, xy, 0, Q.NF1, nf)[1 << 22]
    assert _rec(r[0])[:4] == [1, 64, [64 + PVT[0], 4 + PVT[1]], 64] and _rec(r[1])[:4] == [0, 70, [0, 0], 70]
    assert _rec(r[2])[:4] == [1, 63, [64 + PVT[0], 4 + PVT[1]], 63] and _rec(r[3])[:4] == [2, 35, [0, 0], 69]
    assert _rec(r[4])[:4] == [1, 60, [50 + PVT[0], 1 + PVT[1]], 30] and r[5]["end"] == 0 and r[5]["cells"] > 70 * 15
    assert r[1]["cost"] == sum((1 << 22) - int(f["dist_sq"][7, x]) for x in range(70)) > 2 ** 28
    assert r[1]["nf1_min"] == nf[7][nf[7] >= 0].min() and r[1]["nf1_min_at"] == int(np.flatnonzero(nf[7] == r[1]["nf1_min"])[0])
    assert _rec(_both(f, xy, 0, Q.UNKNOWN_TRAVERSABLE, nf)[9][4])[:4] == [0, 70, [0, 0], 35]


def test_random_trajectories_on_random_planes():
    rng = np.random.default_rng(25)
    ends = []
    for shape in ((9, 9), (9, 70)):
        Y, X = shape
        for rep in range(6):
            k = int(rng.integers(0, 8))
            walls = [(int(rng.integers(0, X)), int(rng.integers(0, Y))) for _ in range(k)]
            f = _plane(shape, walls=walls, unknown=[(int(rng.integers(0, X)), int(rng.integers(0, Y))) for _ in range(4)],
                       fnt=[(int(rng.integers(0, X)), int(rng.integers(0, Y))) for _ in range(4)])
            nf = _nf_field(shape, rep)
            T = int(rng.integers(1, 12)) if X == 9 else int(rng.integers(60, 80))
            start = np.stack([rng.integers(0, X, 20), rng.integers(0, Y, 20)], 1).astype(np.float64)
            step = rng.uniform(-1.5, 1.5, (20, 1, 2)) * np.array([1.0 if X == 9 else 2.0, 1.0])
            c = start[:, None, :] + np.arange(T)[None, :, None] * step + rng.uniform(-0.5, 0.5, (20, T, 2))
            xy = ((c + np.array(PVT[:2])) * W).astype(np.float32)
            xy[rng.random((20, T)) < 0.02] = np.nan
            for flags in range(4):
                ends += _both(f, xy, int(rng.integers(0, 4)), flags, nf)[9]["end"].tolist()
    assert min(ends.count(e) for e in (0, 1, 2)) * 10 >= len(ends), [ends.count(e) for e in (0, 1, 2)]      # every ending, a tenth each


def test_struct_sizes_and_offsets():
    st = _capi.GroundRolloutParam
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("clearance_sq", 0, 4), ("inflate_sq", 4, 4), ("flags", 8, 4), ("reserved", 12, 20)])
    st = _capi.GroundRollout
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (48, [("end", 0, 4), ("poses", 4, 4), ("hit", 8, 8), ("cells", 16, 4), ("min_dist_sq", 20, 4), ("cost", 24, 8), ("nf1_end", 32, 4),
              ("nf1_min", 36, 4), ("nf1_min_at", 40, 4), ("reserved", 44, 4)])
    dt = gie.GROUND_ROLLOUT_DTYPE
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_] and dt.itemsize == 48
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct gie_ground_rollout_param \{(.*?)\} gie_ground_rollout_param;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|int64_t)\s+([\w, \[\]]+);", body) == [("int32_t", "clearance_sq"), ("int32_t", "inflate_sq"), ("int32_t", "flags"), ("int32_t", "reserved[5]")]
    body = re.search(r"typedef struct gie_ground_rollout \{(.*?)\} gie_ground_rollout;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|int64_t)\s+([\w, \[\]]+);", body) == [("int32_t", "end"), ("int32_t", "poses"), ("int32_t", "hit[2]"), ("int32_t", "cells"),
                                                                       ("int32_t", "min_dist_sq"), ("int64_t", "cost"), ("int32_t", "nf1_end"),
                                                                       ("int32_t", "nf1_min"), ("int32_t", "nf1_min_at"), ("int32_t", "reserved")]


def test_binding_and_host_layer_declare_the_section():
    names = ["ground_rollouts", "ground_rollouts_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES and n not in _capi.ROUND_API, n
        assert callable(getattr(gie.Mapper, n))
    assert callable(gie.Mapper.ground_rollout_param)
    assert re.search(r"#define GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE\s+1\b", txt) and re.search(r"#define GIE_GROUND_ROLLOUT_NF1\s+2\b", txt)
    assert re.search(r"#define GIE_GROUND_ROLLOUT_MAX_POSES\s+4096\b", txt)
    assert gie.GroundRolloutParam is _capi.GroundRolloutParam and gie.GroundRollout is _capi.GroundRollout
    assert re.search(r"int gie_ground_rollouts\(gie_mapper \*h, const float \*xy, int n, int T, const gie_ground_rollout_param \*p, gie_ground_rollout \*out\);", txt)
    assert re.search(r"int gie_ground_rollouts_dev\(gie_mapper \*h, const float \*d_xy, int n, int T, const gie_ground_rollout_param \*p, gie_ground_rollout \*d_out\);", txt)
    assert txt.index("gie_ground_view_mask_dev") < txt.index("gie_ground_rollout_param") < txt.index("gie_costmat_compute")
    p = gie.Mapper.ground_rollout_param(None, 4, 16, True, True)
    assert (p.clearance_sq, p.inflate_sq, p.flags, list(p.reserved)) == (4, 16, 3, [0] * 5)
    p = gie.Mapper.ground_rollout_param(None)
    assert (p.clearance_sq, p.inflate_sq, p.flags) == (0, 0, 0)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"int ground_local_plan\(float yaw, const float \*v, const float \*omega, int n, float dt, int T, float inflate_radius, std::vector<float> &poses,\s*"
                     r"std::vector<gie_ground_rollout> &records\)", host)
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_hip.hip")).read()
    assert src.index('#include "gie_ground_view.inc.h"') < src.index('#include "gie_ground_rollout.inc.h"')

"""tests/ground_pose_nf1_ref.py (the numpy statement of include/gie.h "ground pose navigation function") against a second statement
that shares only the footprint's offsets — every state tested on its own through ground_footprint_ref.footprints with T = 1, the
field by relaxing FORWARD along the moves until nothing changes — on hand-made planes, the three fixed scenes of the section with
their numbers, and the section's declarations in the header, the binding and the host layer.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gie
import ground_footprint_ref as P
import ground_nf1_ref as N
import ground_pose_nf1_ref as Q
import ground_ref as R
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
U, F, O, T_ = R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT
PVT = (-7, 40, 0)
FP = (64, 4, 9)                                                 # the fixed cases' footprint: 8 ahead, 2 behind, 3 to either side
BIG = 1 << 20


def _field(t):
    """{"type", "dist_sq"} of a type plane [Y][X]: dist_sq = the exact squared distance to the nearest OCCUPIED cell, -1 without one"""
    t = np.asarray(t, np.int8)
    Y, X = t.shape
    ws = np.argwhere(t == O)
    d = np.full((Y, X), -1, np.int32)
    if len(ws):
        ys, xs = np.mgrid[0:Y, 0:X]
        d = np.full((Y, X), 1 << 30, np.int64)
        for wy, wx in ws:
            d = np.minimum(d, (xs - wx) ** 2 + (ys - wy) ** 2)
        d = d.astype(np.int32)
    return {"type": t, "dist_sq": d}


def _xy(cells):
    c = np.asarray(cells, np.float64).reshape(-1, 2) + np.array(PVT[:2])
    return (c.astype(np.float32) * np.float32(W)).astype(np.float32)


# ------------------------------------------------------------------------------------------------- the second statement
def cspace2(f, e, clearance_sq, flags):
    """bool [8][Y][X]: every state through footprints(T = 1): not free iff end == 1"""
    Y, X = np.asarray(f["type"]).shape
    ys, xs = np.mgrid[0:Y, 0:X]
    xy = _xy(np.stack([xs.ravel(), ys.ravel()], 1)).reshape(-1, 1, 2)
    out = np.zeros((8, Y, X), bool)
    for k, d in enumerate(Q.DIRS):
        hd = np.ascontiguousarray(np.broadcast_to(np.array(d, np.int32), (Y * X, 1, 2)))
        rec = P.footprints(f, xy, hd, PVT, W, e[0], e[1], e[2], clearance_sq, flags & P.UNKNOWN_TRAVERSABLE)
        assert set(rec["end"].tolist()) <= {0, 1}
        out[k] = (rec["end"] == 1).reshape(Y, X)
    return out


def _shift(a, dx, dy):
    """b[y][x] = a[y + dy][x + dx], BIG outside"""
    Y, X = a.shape
    b = np.full((Y, X), BIG, a.dtype)
    ys0, ys1 = max(0, -dy), min(Y, Y - dy)
    xs0, xs1 = max(0, -dx), min(X, X - dx)
    b[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return b


def relax2(cs, src, reverse):
    """int32 [8][Y][X]: v = 0 on sources, else 1 + the least v over the targets of the state's own moves, iterated to the fixed point"""
    v = np.where(src, 0, BIG).astype(np.int64)
    while True:
        new = v.copy()
        for k, (dx, dy) in enumerate(Q.DIRS):
            best = np.minimum(v[(k + 1) & 7], v[(k + 7) & 7])
            best = np.minimum(best, _shift(v[k], dx, dy))
            if reverse:
                best = np.minimum(best, _shift(v[k], -dx, -dy))
            new[k] = np.where(~cs[k], np.minimum(v[k], best + 1), BIG)
        if np.array_equal(new, v):
            break
        v = new
    return np.where(v >= BIG, -1, v).astype(np.int32)


def sources2(f, cs, goal_cells, goal_k, flags):
    src = np.zeros(cs.shape, bool)
    for i, c in enumerate(goal_cells):
        k = -1 if goal_k is None else goal_k[i]
        if c is None or not -1 <= k <= 7:
            continue
        if k == -1:
            src[:, c[1], c[0]] = True
        else:
            src[k, c[1], c[0]] = True
    if flags & Q.FROM_FRONTIERS:
        src |= (np.asarray(f["type"]) == T_)[None]
    return src & ~cs


def both(f, goal_cells, goal_k, e, clearance_sq=0, flags=0, nan_tail=0):
    """the reference's field, checked against the second statement: (pnf1, cspace bytes, counts)"""
    Y, X = np.asarray(f["type"]).shape
    xy = _xy([c for c in goal_cells]) if len(goal_cells) else np.zeros((0, 2), np.float32)
    gk = None if goal_k is None else list(goal_k)
    if nan_tail:
        xy = np.concatenate([xy, np.full((nan_tail, 2), np.nan, np.float32)])
        gk = None if gk is None else gk + [0] * nan_tail
    nf, cb, counts = Q.field(f, xy, gk, PVT, W, e[0], e[1], e[2], clearance_sq, flags)
    cs = cspace2(f, e, clearance_sq, flags)
    assert np.array_equal(cb, Q.cspace_bytes(cs)), "C-space"
    inside = [c if 0 <= c[0] < X and 0 <= c[1] < Y else None for c in goal_cells]
    src = sources2(f, cs, inside, goal_k, flags)
    want = relax2(cs, src, bool(flags & Q.REVERSE))
    assert np.array_equal(nf, want), "field"
    assert counts == [int(src.sum()), int((~cs).sum())]
    assert ((nf == 0) == src).all() and (nf[cs] == -1).all()
    return nf, cb, counts


# ------------------------------------------------------------------------------------------------- hand-made planes
def _random_plane(X, Y, seed, walls=10, unknown=True, fnt=True):
    rng = np.random.default_rng(seed)
    t = np.full((Y, X), F, np.int8)
    for _ in range(walls):
        x, y = int(rng.integers(0, X)), int(rng.integers(0, Y))
        t[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = O
    if unknown:
        t[:, :2] = U
        if fnt:
            t[:, 2][t[:, 2] == F] = T_
    return t


@pytest.mark.parametrize("X", [9, 64, 65, 70, 130])
def test_reference_equals_the_second_statement_on_random_planes(X):
    Y = 9 if X > 70 else 11
    t = _random_plane(X, Y, X)
    f = _field(t)
    goals = [(X - 2, Y // 2), (X // 2, 1), (X + 3, 2)]           # the last lies outside: ignored
    for flags in range(8):                                       # both values of each flag
        for e, c in (((4, 1, 1), 0), ((0, 0, 0), 1)):
            nf, cb, counts = both(f, goals, [-1, 2, 0], e, c, flags, nan_tail=2)
            if e == (0, 0, 0):                                   # the eight layers are equal, free iff not blocked
                blk = ~N.traversable(f, c, flags & 1)
                assert np.array_equal(cb, np.where(blk, 255, 0).astype(np.uint8))
    nf, cb, counts = both(f, goals, [-1, 2, 0], (9, 1, 1), 0, Q.REVERSE)
    assert (cb != 0).any() and (cb != 255).any() and ((cb != 0) & (cb != 255)).any()       # free, blocked and heading-dependent cells


def test_goal_headings_and_a_nan_tail():
    f = _field(np.full((7, 9), F, np.int8))                      # a field without an obstacle column: dist_sq is -1 everywhere
    assert (f["dist_sq"] == -1).all()
    g = [(4, 3)]
    for k in list(range(-1, 9)) + [None]:
        nf, cb, counts = both(f, g, None if k is None else [k], (0, 0, 0), 3, 0, nan_tail=1)
        if k is None or k == -1:
            assert counts == [8, 8 * 63] and (nf[:, 3, 4] == 0).all()
        elif k == 8:
            assert counts[0] == 0 and (nf == -1).all()           # ignored
        else:
            assert counts[0] == 1 and nf[k, 3, 4] == 0 and nf[(k + 1) & 7, 3, 4] == 1 and nf[(k + 4) & 7, 3, 4] == 4      # the turn wraps 7 <-> 0
    nf, _, counts = both(f, [], None, (0, 0, 0))                 # n == 0
    assert counts == [0, 8 * 63] and (nf == -1).all()


def test_diagonal_moves_cross_the_word_boundaries_and_nothing_wraps():
    X, Y = 130, 8
    f = _field(np.full((Y, X), F, np.int8))
    for k, goal in ((1, (66, 5)), (3, (61, 5)), (5, (61, 2)), (7, (66, 2)), (1, (130 - 1, 7)), (3, (126, 6)), (5, (125, 1)), (7, (129, 1)), (5, (0, 0)), (3, (0, 7))):
        nf, _, _ = both(f, [goal], [k], (0, 0, 0), 0, Q.UNKNOWN_TRAVERSABLE)
        dx, dy = Q.DIRS[k]
        x, y, n = goal[0], goal[1], 0
        while 0 <= x - dx < X and 0 <= y - dy < Y:               # F alone along the diagonal: one move per cell, across x = 63 | 64 and 127 | 128
            x, y, n = x - dx, y - dy, n + 1
            assert nf[k, y, x] == n, (k, goal, x, y)
        assert n >= 1
    # a goal in the last column, heading +x: the first cell of the next row is NOT one move away (nothing wraps)
    nf, _, _ = both(f, [(X - 1, 3)], [0], (0, 0, 0))
    assert nf[0, 3, X - 2] == 1 and nf[0, 4, 0] > X - 1 and nf[4, 2, X - 1] > 4
    nf, _, _ = both(f, [(0, 3)], [4], (0, 0, 0), 0, Q.REVERSE)
    assert nf[4, 3, 1] == 1 and nf[4, 2, X - 1] > X - 1


def test_front_and_back_differ_and_the_cap():
    t = np.full((9, 20), F, np.int8)
    t[:, 12] = O
    f = _field(t)
    nf, cb, _ = both(f, [(2, 4)], None, (16, 0, 0))
    assert (cb[4, 9] >> 0) & 1 and not (cb[4, 9] >> 4) & 1       # free at k = 4 and blocked at k = 0: layers k and k + 4 differ
    cap = Q.MAX_SQ
    f = _field(np.full((5, 9), F, np.int8))
    nf, cb, counts = both(f, [(4, 2)], None, (cap, 0, 0), 0, 0)  # 64 cells ahead: every state reaches outside the rectangle
    assert (cb == 255).all() and counts == [0, 0]
    nf, cb, counts = both(f, [(4, 2)], None, (cap, cap, cap), 0, Q.UNKNOWN_TRAVERSABLE)
    assert (cb == 0).all() and counts == [8, 8 * 45]
    assert P.radius(cap, cap, cap) == 90 and max(np.ptp(P.offsets(d, cap, cap, cap)[:, 0]) for d in Q.DIRS) + 1 <= 181


def test_path_and_query_one_step_at_a_time():
    t = _random_plane(40, 12, 5, walls=6, unknown=False)
    f = _field(t)
    for flags in (0, Q.REVERSE):
        nf, cb, _ = both(f, [(35, 6)], None, (4, 1, 1), 0, flags)
        rev = bool(flags)
        Y, X = t.shape
        ys, xs = np.nonzero((nf >= 0).any(0))
        cells = np.stack([xs, ys], 1)[::7]
        ks = [(-1, 0, 3, 5, 7, 8, -2)[i % 7] for i in range(len(cells))]
        xy = np.concatenate([_xy(cells), [[np.nan, 0.0]]]).astype(np.float32)
        ks = ks + [0]
        q = Q.query(nf, xy, ks, PVT, W)
        path, ln = Q.path(nf, xy, ks, PVT, W, 200, rev, fill=-9)
        short, ln2 = Q.path(nf, xy, ks, PVT, W, 3, rev, fill=-9)
        assert np.array_equal(ln, ln2) and np.array_equal(short[:, :3][ln2[:, None, None].repeat(3, 1).repeat(3, 2) > np.arange(3)[None, :, None]],
                                                          path[:, :3][ln[:, None, None].repeat(3, 1).repeat(3, 2) > np.arange(3)[None, :, None]])
        assert (ln > 3).any() and (ln == 0).any()
        for i, (c, k) in enumerate(zip(list(map(tuple, cells)) + [None], ks)):
            if c is None or not -1 <= k <= 7:
                assert q[i] == -1 and ln[i] == 0 and (path[i] == -9).all()
                continue
            col = nf[:, c[1], c[0]]
            if k == -1:
                assert q[i] == col[col >= 0].min() and path[i, 0, 2] == int(np.flatnonzero(col == q[i])[0])     # the lowest k among the least: ties
            else:
                assert q[i] == col[k]
            assert ln[i] == q[i] + 1
            if ln[i] == 0:
                assert (path[i] == -9).all()
                continue
            p = path[i, :ln[i]] - np.array([PVT[0], PVT[1], 0])
            assert (path[i, ln[i]:] == -9).all() and nf[p[-1, 2], p[-1, 1], p[-1, 0]] == 0
            for a, b in zip(p[:-1], p[1:]):                      # consecutive states differ by one admissible move, the FIRST that descends
                mv = Q.moves(int(a[0]), int(a[1]), int(a[2]), rev)
                down = [s for s in mv if 0 <= s[0] < X and 0 <= s[1] < Y and nf[s[2], s[1], s[0]] == nf[a[2], a[1], a[0]] - 1]
                assert tuple(b) == down[0]
        assert np.array_equal(Q.query(nf, xy, None, PVT, W), Q.query(nf, xy, [-1] * len(xy), PVT, W))          # k == NULL: -1 for all
        assert np.array_equal(Q.path(nf, xy, None, PVT, W, 5, rev)[1], Q.path(nf, xy, [-1] * len(xy), PVT, W, 5, rev)[1])


def test_heading_index():
    assert [Q.heading_index(a) for a in (0.0, 0.39, 0.4, np.pi / 2, np.pi, -np.pi, -np.pi / 4, -0.39, 2 * np.pi, 7 * np.pi / 4 + 0.1, -3 * np.pi)] == \
        [0, 0, 1, 2, 4, 4, 7, 0, 0, 7, 4]


# ------------------------------------------------------------------------------------------------- the fixed cases
def door():
    t = np.full((40, 70), F, np.int8)
    t[0] = t[-1] = O
    t[:, 0] = t[:, -1] = O
    t[:, 34:36] = O
    t[16:25, 34:36] = F
    return t


def pocket():
    t = np.full((30, 64), F, np.int8)
    t[0] = t[-1] = O
    t[:, 0] = t[:, -1] = O
    t[1:11, 1:40] = O
    t[18:29, 1:40] = O
    return t


def l_turn():
    t = np.full((48, 64), O, np.int8)
    t[4:24, 4:28] = F
    t[30:44, 40:60] = F
    t[10:17, 28:50] = F
    t[10:30, 43:50] = F
    return t


def test_fixed_door():
    f = _field(door())
    nf, _, _ = both(f, [(55, 20)], None, FP)
    assert nf[:, 20, 12].tolist() == [43, 44, 45, 46, 47, 46, 45, 44]
    nf, _, _ = both(f, [(55, 20)], None, FP, 0, Q.REVERSE)
    assert nf[:, 20, 12].tolist() == [43, 44, 45, 44, 43, 44, 45, 44]
    assert N.field(f, _xy([(55, 20)]), PVT, W, 73)[0][20, 12] == -1          # the circumscribed disc does not pass the door
    assert N.field(f, _xy([(55, 20)]), PVT, W, 9)[0][20, 12] == 43


def test_fixed_pocket():
    f = _field(pocket())
    nf, cb, _ = both(f, [(55, 14)], None, FP)
    assert not (cb[14, 20] >> 4) & 1 and nf[4, 14, 20] == -1 and nf[0, 14, 20] == 38 and (cb[14, 20] >> 2) & 1 and nf[2, 14, 20] == -1
    nf, cb, _ = both(f, [(55, 14)], None, FP, 0, Q.REVERSE)
    assert nf[4, 14, 20] == 35 and nf[0, 14, 20] == 38 and nf[2, 14, 20] == -1


def test_fixed_l_turn():
    f = _field(l_turn())
    for flags in (0, Q.REVERSE):
        nf, cb, _ = both(f, [(50, 37)], None, FP, 0, flags)
        assert nf[:, 12, 12].tolist() == [-1] * 8 and cb[12, 12] != 255
    assert N.field(f, _xy([(50, 37)]), PVT, W, 9)[0][12, 12] == 63            # the inscribed disc is sent round the corner


# ------------------------------------------------------------------------------------------------- declarations
def test_struct_size_offsets_flags_and_constants():
    st = _capi.GroundPoseNf1Param
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("front_sq", 0, 4), ("back_sq", 4, 4), ("side_sq", 8, 4), ("clearance_sq", 12, 4), ("flags", 16, 4), ("reserved", 20, 12)])
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct gie_ground_pose_nf1_param \{(.*?)\} gie_ground_pose_nf1_param;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|int64_t)\s+([\w, \[\]]+);", body) == [("int32_t", "front_sq"), ("int32_t", "back_sq"), ("int32_t", "side_sq"), ("int32_t", "clearance_sq"),
                                                                       ("int32_t", "flags"), ("int32_t", "reserved[3]")]
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, val in (("NF1_UNKNOWN_TRAVERSABLE", "1"), ("NF1_FROM_FRONTIERS", "2"), ("NF1_REVERSE", "4"), ("HEADINGS", "8"), ("MAX_SQ", r"\(1 << 12\)")):
        assert re.search(r"#define GIE_GROUND_POSE_%s\s+%s\s*$" % (name, val), txt, re.M), name
    assert (gie.GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE, gie.GROUND_POSE_NF1_FROM_FRONTIERS, gie.GROUND_POSE_NF1_REVERSE, gie.GROUND_POSE_HEADINGS, gie.GROUND_POSE_MAX_SQ) == \
        (Q.UNKNOWN_TRAVERSABLE, Q.FROM_FRONTIERS, Q.REVERSE, Q.HEADINGS, Q.MAX_SQ) == (1, 2, 4, 8, 4096)
    assert gie.GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE == gie.GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE
    assert gie.GroundPoseNf1Param is _capi.GroundPoseNf1Param


def test_header_binding_and_host_layer_declare_the_section():
    names = ["ground_pose_nf1_compute", "ground_pose_nf1_compute_dev", "read_ground_pose_nf1", "read_ground_pose_nf1_dev", "ground_pose_nf1_query",
             "ground_pose_nf1_query_dev", "ground_pose_nf1_path", "ground_pose_nf1_path_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES and n not in _capi.ROUND_API, n
        assert callable(getattr(gie.Mapper, n))
    assert re.search(r"int gie_ground_pose_nf1_compute\(gie_mapper \*h, const float \*goal_xy, const int32_t \*goal_k, int n, const gie_ground_pose_nf1_param \*p, "
                     r"int32_t \*counts\);", txt)
    assert re.search(r"int gie_read_ground_pose_nf1_dev\(gie_mapper \*h, int32_t \*d_pnf1, uint8_t \*d_cspace\);", txt)
    assert re.search(r"int gie_ground_pose_nf1_query\(gie_mapper \*h, const float \*xy, const int32_t \*k, int n, int32_t \*steps\);", txt)
    assert re.search(r"int gie_ground_pose_nf1_path_dev\(gie_mapper \*h, const float \*d_start_xy, const int32_t \*d_start_k, int n, int max_len, int32_t \*d_path_xyk, "
                     r"int32_t \*d_len\);", txt)
    assert txt.index("gie_ground_footprint_mask_dev") < txt.index("gie_ground_pose_nf1_param") < txt.index("gie_costmat_compute")
    p = gie.Mapper.ground_pose_nf1_param(None, 100, 36, 25, 4, True, True, True)
    assert (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags, list(p.reserved)) == (100, 36, 25, 4, 7, [0] * 3)
    p = gie.Mapper.ground_pose_nf1_param(None, 1, 2, 3, reverse=True)
    assert (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags) == (1, 2, 3, 0, 4)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"static int ground_heading_index\(double yaw\)", host)
    assert re.search(r"bool ground_plan_footprint\(float yaw, const float \*goal_xy, const float \*goal_yaw, int n, bool from_frontiers, bool reverse, int max_len,\s*"
                     r"std::vector<std::array<int32_t, 3>> &path\)", host)
    assert "ground_pose_plan_len" in host and "ground_pose_plan_sources" in host
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_hip.hip")).read()
    assert src.index('#include "gie_ground_footprint.inc.h"') < src.index('#include "gie_ground_pose_nf1.inc.h"')

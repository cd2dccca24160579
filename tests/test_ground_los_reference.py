"""tests/ground_los_ref.py (the numpy statement of include/gie.h "ground line of sight"): its 2-D cell line against the merged 3-D
voxel line and against an exact-rational statement of the definition, the shortcut on hand-made scenes, and the binding's view of
the section.  No GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np

import gie
import ground_los_ref as L
import ground_ref as R
import los_ref
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
GRID = [(x, y) for y in range(9) for x in range(9)]


def rational_line(a, b):
    """the cells whose square shares a piece of POSITIVE length with the segment between the centres of a and b, in the order of
    those pieces: the segment a + t (b - a), t in [0, 1], is cut at every t where it meets a grid line x = i + 1/2 or y = j + 1/2;
    between two consecutive cuts it lies strictly inside ONE square, the one that holds the piece's midpoint.  Fractions only."""
    ax, ay, bx, by = (Fraction(int(v)) for v in (*a, *b))
    dx, dy = bx - ax, by - ay
    if dx == 0 and dy == 0:
        return [(int(ax), int(ay))]
    cuts = {Fraction(0), Fraction(1)}
    for o, d in ((ax, dx), (ay, dy)):
        if d != 0:
            lo, hi = min(o, o + d), max(o, o + d)
            g = Fraction(2 * int(lo) + 1, 2)                    # (the centres are integers: the first grid line beyond lo)
            while g < hi:
                cuts.add((g - o) / d)
                g += 1
    ts = sorted(cuts)
    out = []
    for t0, t1 in zip(ts, ts[1:]):
        tm = (t0 + t1) / 2
        x, y = ax + tm * dx, ay + tm * dy
        cell = (int((x + Fraction(1, 2)) // 1), int((y + Fraction(1, 2)) // 1))     # the square [i - 1/2, i + 1/2) that holds it
        assert (x + Fraction(1, 2)) % 1 != 0 or dx == 0, "a midpoint on a grid line"
        assert (y + Fraction(1, 2)) % 1 != 0 or dy == 0
        if not out or out[-1] != cell:
            out.append(cell)
    return out


def test_line_equals_the_3d_voxel_line_on_a_9x9_grid():
    for a in GRID:
        for b in GRID:
            assert [(x, y, 0) for x, y in L.line(a, b)] == los_ref.line((a[0], a[1], 0), (b[0], b[1], 0)), (a, b)


def test_line_equals_the_exact_rational_definition():
    rng = np.random.default_rng(21)
    far = [((int(p[0]), int(p[1])), (int(p[2]), int(p[3]))) for p in rng.integers(-40, 41, size=(150, 4))]
    far += [((0, 0), (1023, 1021)), ((1023, 0), (0, 1023)), ((5, 700), (5, -3)), ((0, 0), (1023, 1))]
    for a, b in [(a, b) for a in GRID[::3] for b in GRID] + far:
        ln = L.line(a, b)
        assert ln == rational_line(a, b), (a, b)
        assert ln == L.line(b, a)[::-1], (a, b)                 # reversal
        assert len(set(ln)) == len(ln)                          # no cell repeats
        nx, ny = abs(b[0] - a[0]), abs(b[1] - a[1])
        assert 1 + max(nx, ny) <= len(ln) <= 1 + nx + ny and ln[0] == tuple(a) and ln[-1] == tuple(b)
    assert L.line((3, 4), (3, 4)) == [(3, 4)]
    assert L.line((0, 0), (3, 3)) == [(0, 0), (1, 1), (2, 2), (3, 3)]               # ties: diagonal moves, the corner cells left out
    assert len(L.line((0, 0), (3, 2))) == 1 + 3 + 2                                 # no tie: every crossing is a cell of its own


def test_struct_sizes_and_field_offsets():
    def layout(s):
        return C.sizeof(s), [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]
    assert layout(_capi.GroundLosParam) == (16, [("clearance_sq", 0, 4), ("flags", 4, 4), ("reserved", 8, 8)])
    assert layout(_capi.GroundHit) == (24, [("first", 0, 4), ("len", 4, 4), ("hit", 8, 8), ("min_dist_sq", 16, 4), ("reserved", 20, 4)])
    assert layout(_capi.GroundShortcutParam) == (32, [("lookahead", 0, 4), ("max_wp", 4, 4), ("clearance_sq", 8, 4), ("flags", 12, 4), ("reserved", 16, 16)])
    assert layout(_capi.GroundWaypoint) == (24, [("xy", 0, 8), ("index", 8, 4), ("min_dist_sq", 12, 4), ("forced", 16, 4), ("reserved", 20, 4)])
    for dt, st in ((gie.GROUND_HIT_DTYPE, _capi.GroundHit), (gie.GROUND_WAYPOINT_DTYPE, _capi.GroundWaypoint), (L.HIT_DTYPE, _capi.GroundHit),
                   (L.WAYPOINT_DTYPE, _capi.GroundWaypoint), (L.INFO_DTYPE, _capi.ShortcutInfo)):
        assert dt.itemsize == C.sizeof(st)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    assert gie.GROUND_HIT_DTYPE == L.HIT_DTYPE and gie.GROUND_WAYPOINT_DTYPE == L.WAYPOINT_DTYPE
    # the header's structs, field by field (every member is an int32 or an array of them)
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    for name, st in (("gie_ground_los_param", _capi.GroundLosParam), ("gie_ground_hit", _capi.GroundHit),
                     ("gie_ground_shortcut_param", _capi.GroundShortcutParam), ("gie_ground_waypoint", _capi.GroundWaypoint)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"int32_t\s+(\w+)(?:\[(\d+)\])?;", body)
        assert [(n, 4 * int(k or 1)) for n, k in members] == [(n, getattr(st, n).size) for n, _ in st._fields_], name


def test_binding_and_host_layer_declare_the_section():
    names = ["ground_segments", "ground_segments_dev", "ground_shortcut", "ground_shortcut_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES, n
        assert callable(getattr(gie.Mapper, n))
    assert "GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE 1" in txt
    assert gie.GROUND_LOS_UNKNOWN_TRAVERSABLE == _capi.GROUND_LOS_UNKNOWN_TRAVERSABLE == L.UNKNOWN_TRAVERSABLE == 1
    for n in ("GroundLosParam", "GroundHit", "GroundShortcutParam", "GroundWaypoint"):
        assert getattr(gie, n) is getattr(_capi, n)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"bool ground_waypoints\(const float \*goal_xy, int n, bool from_frontiers, int max_len, int lookahead, std::vector<gie_ground_waypoint> &wp\)", host)
    assert "ground_waypoints_info" in host
    assert re.search(r"bool ground_plan\(const float \*goal_xy, int n, bool from_frontiers, int max_len, std::vector<std::array<int32_t, 2>> &path\)", host)


# ---------------------------------------------------------------------------------------------------------- scenes made by hand
def _field(lab2d, flags=0):
    """ground_ref.field of a one-layer volume at pivot PVT"""
    return R.field(np.asarray(lab2d, np.int8)[None], PVT, 0, 0, 1, flags)


PVT = (-7, 40, 0)


def _glob(cells):
    return (np.asarray(cells, np.int64).reshape(-1, 2) + np.array(PVT[:2])).astype(np.int32)


def _pillar_scene():
    """a free 30 x 20 plane with a 2 x 2 pillar; a path that runs along y = 2, x = 2 .. 27, and then up along x = 27: seen from
    (2, 8) the stretch behind the pillar is hidden, the points beyond its shadow are visible again"""
    lab = np.ones((20, 30), np.int8)
    lab[6:8, 12:14] = 2
    return _field(lab)


def test_segments_reference_by_hand():
    f = _pillar_scene()
    xy = lambda c: ((np.asarray(c, np.float64).reshape(-1, 2) + np.array(PVT[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)   # noqa: E731
    a = xy([(2, 6), (2, 6), (2, 2), (5, 5), (-1, 0), (0, 0), (29, 19)])
    b = xy([(25, 6), (25, 6), (25, 2), (5, 5), (3, 3), (30, 0), (0, 0)])
    b[1, 0] = np.nan
    h = L.segments(f, a, b, PVT, W)
    assert h["first"].tolist() == [10, -2, -1, -1, -2, -2, -1] and h["len"].tolist() == [24, 0, 24, 1, 0, 0, 48]      # (29, 19): one tie, at the middle
    assert (h["hit"][0] - np.array(PVT[:2])).tolist() == [12, 6] and h["min_dist_sq"][0] == 0
    assert (h["hit"][2] - np.array(PVT[:2])).tolist() == [25, 2] and h["min_dist_sq"][2] == 16      # four rows below the pillar
    assert h["hit"][1].tolist() == [0, 0] and h["min_dist_sq"][1] == 0
    h4 = L.segments(f, a, b, PVT, W, 4)                         # a disc of radius 2: the cell beside the pillar (dist_sq 1) is blocked, the one before it (4) is not
    assert h4["first"][0] == 9 and h4["min_dist_sq"][0] == 1 and h4["first"][2] == -1
    assert L.segments(f, a, b, PVT, W, 17)["first"][2] == 10    # the line four cells below the pillar: dist_sq 16 < 17 at x = 12 first
    free = _field(np.ones((20, 30), np.int8))
    hf = L.segments(free, a, b, PVT, W, 10 ** 6)                # no obstacle column: -1 passes every clearance
    assert hf["first"].tolist() == [-1, -2, -1, -1, -2, -2, -1] and hf["min_dist_sq"].tolist() == [-1, 0, -1, -1, 0, 0, -1]
    unk = np.ones((20, 30), np.int8)
    unk[:, 10] = 0
    fu = _field(unk)
    assert L.segments(fu, a, b, PVT, W)["first"][2] == 8 and L.segments(fu, a, b, PVT, W, 0, 1)["first"][2] == -1
    fb = _field(unk, R.UNKNOWN_BLOCKS)                          # an UNKNOWN column at distance 0: the flag opens it at clearance 0 only
    assert L.segments(fb, a, b, PVT, W, 0, 1)["first"][2] == -1 and L.segments(fb, a, b, PVT, W, 1, 1)["first"][2] == 8


def test_shortcut_reference_pillar_shadow_is_not_monotone():
    f = _pillar_scene()
    cells = [(2, 8)] + [(x, 2) for x in range(2, 28)] + [(27, y) for y in range(3, 15)]
    path = _glob(cells)[None]
    blk = L.blocked(f)
    vis = [L.clear(blk, cells[0], c) for c in cells[1:]]
    first_hidden = vis.index(False)
    assert any(vis[first_hidden:]) and not all(vis[first_hidden:])                  # hidden, then visible again
    last = len(vis) - 1 - vis[::-1].index(True) + 1
    wp, info = L.shortcut(f, path, [len(cells)], PVT, 4096, 8)
    assert info["forced"][0] == 0 and wp["index"][0, 1] == last > first_hidden + 1  # max J, not the last before the first blocked one
    n = int(info["count"][0])
    assert wp["index"][0, 0] == 0 and wp["index"][0, n - 1] == len(cells) - 1 and (np.diff(wp["index"][0, :n]) > 0).all()
    assert (wp["xy"][0, :n] == path[0, wp["index"][0, :n]]).all() and not wp["reserved"].any() and info["reserved"][0] == 0
    want = np.float32(0)
    for t in range(1, n):
        d = (path[0, wp["index"][0, t]].astype(np.int64) - path[0, wp["index"][0, t - 1]]) ** 2
        want = np.float32(want + np.sqrt(np.float32(d.sum())))
        ln = L.line(cells[wp["index"][0, t - 1]], cells[wp["index"][0, t]])
        assert wp["min_dist_sq"][0, t] == min(f["dist_sq"][y, x] for x, y in ln) > 0
    assert info["length"][0] == want and wp["min_dist_sq"][0, 0] == f["dist_sq"][8, 2]
    # a short look-ahead: no leg reaches further than K points
    wp3, info3 = L.shortcut(f, path, [len(cells)], PVT, 3, 64)
    n3 = int(info3["count"][0])
    assert (np.diff(wp3["index"][0, :n3]) <= 3).all() and n3 > n and info3["length"][0] >= info["length"][0]


def test_shortcut_reference_short_paths_outside_blocked_and_capacity():
    f = _pillar_scene()
    poison = np.zeros((1, 4), L.WAYPOINT_DTYPE)
    poison.view(np.uint8)[:] = 0x5a
    # m = 0 (also from len < 0), 1 and 2; len > max_len is cut to max_len
    pts = _glob([(3, 3), (9, 5), (11, 9)])[None]
    for ln, m in ((0, 0), (-5, 0), (1, 1), (2, 2), (3, 3), (77, 3)):
        wp, info = L.shortcut(f, pts, [ln], PVT, 8, 4, wp_init=poison)
        # every point sees every other: one leg from v_0 to v_{m-1}, sqrt(36 + 4) or sqrt(64 + 36) long
        length = {0: 0.0, 1: 0.0, 2: float(np.sqrt(np.float32(40))), 3: 10.0}[m]
        assert info[0].tolist() == (min(m, 2), 0, length, 0), (ln, info)
        assert wp.tobytes()[24 * min(m, 2):] == poison.tobytes()[24 * min(m, 2):]       # the tail is untouched
        if m:
            r = wp[0, 0]
            assert (r["xy"].tolist(), r["index"], r["min_dist_sq"], r["forced"], r["reserved"]) == (pts[0, 0].tolist(), 0, int(f["dist_sq"][3, 3]), 0, 0)
        if m > 1:
            assert wp["index"][0, 1] == m - 1 and wp["forced"][0, 1] == 0
    # a point outside the rectangle: the legs into it and out of it are forced, whatever int32 it is
    out = np.array([[_glob([(3, 3)])[0], _glob([(4, 3)])[0], [2 ** 31 - 1, -2 ** 31], _glob([(6, 3)])[0], _glob([(20, 3)])[0]]], np.int32)
    wp, info = L.shortcut(f, out, [5], PVT, 1, 8)
    assert info[0].tolist() == (5, 2, 1.0 + 14.0, 0)
    assert wp["forced"][0, :5].tolist() == [0, 0, 1, 1, 0] and wp["min_dist_sq"][0, 2:4].tolist() == [L.NO_VALUE, L.NO_VALUE]
    wp, info = L.shortcut(f, out, [5], PVT, 4, 8)               # with a longer look-ahead the outside point is jumped over
    assert info[0].tolist() == (2, 0, 17.0, 0) and wp["index"][0, :2].tolist() == [0, 4]
    first_out = out[:, ::-1].copy()
    first_out[0, 0] = [-2 ** 31, 0]
    wp, info = L.shortcut(f, first_out, [3], PVT, 4, 8)         # v_0 outside: min_dist_sq -2 at t = 0, a forced first leg
    assert wp["min_dist_sq"][0, 0] == L.NO_VALUE and wp["forced"][0, :3].tolist() == [0, 1, 1] and info["forced"][0] == 2
    # a blocked start (inside the pillar; with a clearance, beside it): forced without a walk, then clear legs
    start_in = _glob([(12, 6), (11, 6), (10, 6), (3, 6)])[None]
    wp, info = L.shortcut(f, start_in, [4], PVT, 8, 8)
    assert info[0].tolist() == (3, 1, 8.0, 0) and wp["index"][0, :3].tolist() == [0, 1, 3] and wp["min_dist_sq"][0, 0] == 0
    wp, info = L.shortcut(f, start_in, [4], PVT, 8, 8, 4)
    assert info[0].tolist() == (4, 2, 7.0, 0) and wp["forced"][0, :4].tolist() == [0, 1, 1, 0] and wp["min_dist_sq"][0, 3] == 4
    # capacity: max_wp 0 and max_wp smaller than count; info is complete, the tails are untouched
    cells = [(2, 8)] + [(x, 2) for x in range(2, 28)] + [(27, y) for y in range(3, 15)]
    path = _glob(cells)[None]
    full, info_full = L.shortcut(f, path, [len(cells)], PVT, 3, 64)
    cnt = int(info_full["count"][0])
    assert cnt > 4
    wp0, info0 = L.shortcut(f, path, [len(cells)], PVT, 3, 0)
    assert wp0.shape == (1, 0) and info0.tobytes() == info_full.tobytes()
    wp4, info4 = L.shortcut(f, path, [len(cells)], PVT, 3, 4, wp_init=poison)
    assert info4.tobytes() == info_full.tobytes() and wp4.tobytes() == full[:, :4].tobytes()
    big = np.zeros((1, cnt + 3), L.WAYPOINT_DTYPE)
    big.view(np.uint8)[:] = 0x5a
    wpb, _ = L.shortcut(f, path, [len(cells)], PVT, 3, cnt + 3, wp_init=big)
    assert wpb[:, :cnt].tobytes() == full[:, :cnt].tobytes() and wpb[:, cnt:].tobytes() == big[:, cnt:].tobytes()

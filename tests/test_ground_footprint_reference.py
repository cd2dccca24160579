"""tests/ground_footprint_ref.py (the numpy statement of include/gie.h "ground footprints"): the properties of the footprint itself —
axis-aligned counts, the quarter turn, the scaling of the heading, the bounding disc, one interval per row, the single cell — the
record on hand-made planes (a wall through the footprint, outside cells, tails), and the section's declarations in the header, the
binding and the host layer.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

import gie
import ground_footprint_ref as P
import ground_ref as R
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
U, F, O, T_ = R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT
PVT = (-7, 40, 0)
HEADINGS = [(1, 0), (0, 1), (-1, 0), (0, -5), (1, 1), (-3, 3), (2, -1), (3, 4), (-7, 2), (32767, 1), (1, -32767), (-32767, -32767), (8, -8), (5, 12)]
EXTENTS = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (9, 4, 1), (25, 0, 9), (100, 36, 36), (7, 5, 3), (1600, 4, 9), (50, 50, 50)]


def _plane(shape=(9, 9), walls=(), unknown=()):
    """{"type", "dist_sq"} [Y][X]: dist_sq = the exact squared distance to the nearest wall cell, -1 everywhere without one"""
    Y, X = shape
    t = np.full((Y, X), F, np.int8)
    for (x, y) in unknown:
        t[y, x] = U
    for (x, y) in walls:
        t[y, x] = O
    d = np.full((Y, X), -1, np.int32)
    if len(walls):
        w = np.asarray(walls)
        xs, ys = np.arange(X)[None, :, None], np.arange(Y)[:, None, None]
        d = ((xs - w[:, 0]) ** 2 + (ys - w[:, 1]) ** 2).min(axis=2).astype(np.int32)
    return {"type": t, "dist_sq": d}


def _xy(cells):
    """world points (float32 metres) of local cells: (cell + pvt) * w, the product in float32"""
    c = np.asarray(cells, np.float64) + np.array(PVT[:2])
    return (c.astype(np.float32) * np.float32(W)).astype(np.float32)


def _set(h, e):
    return set(map(tuple, P.offsets(h, *e).tolist()))


def _one(f, cells, heads, e, clearance_sq=0, flags=0):
    """the record of ONE trajectory through `cells` with `heads`"""
    xy = _xy(cells)[None]
    return P.footprints(f, xy, np.asarray(heads, np.int32)[None], PVT, W, e[0], e[1], e[2], clearance_sq, flags)[0]


def _rec(r):
    return [int(r["end"]), int(r["poses"]), r["hit"].tolist(), int(r["hit_cells"]), int(r["min_dist_sq"]), int(r["min_at"])]


# ---------------------------------------------------------------------------------------------------------- the footprint
def test_axis_aligned_headings_give_the_rectangle():
    for f, b, s in ((0, 0, 0), (3, 1, 2), (5, 5, 0), (0, 4, 7), (40, 2, 3)):
        e = (f * f, b * b, s * s)
        assert _set((1, 0), e) == {(x, y) for x in range(-b, f + 1) for y in range(-s, s + 1)}
        assert _set((0, -5), e) == {(x, y) for y in range(-f, b + 1) for x in range(-s, s + 1)}      # ahead is -y
        assert len(P.offsets((1, 0), *e)) == len(P.offsets((0, -5), *e)) == (f + b + 1) * (2 * s + 1)


def test_a_quarter_turn_of_the_heading_turns_the_set():
    for h in HEADINGS:
        for e in EXTENTS:
            assert _set((-h[1], h[0]), e) == {(-y, x) for x, y in _set(h, e)}, (h, e)


def test_scaling_the_heading_changes_nothing():
    for h in [h for h in HEADINGS if max(abs(h[0]), abs(h[1])) * 4000 <= 32767]:
        for e in EXTENTS:
            assert np.array_equal(P.offsets(h, *e), P.offsets((4000 * h[0], 4000 * h[1]), *e)), (h, e)
    assert np.array_equal(P.offsets((1, 1), 100, 36, 36), P.offsets((32767, 32767), 100, 36, 36))


def test_bounding_disc_centre_rows_and_order():
    for h in HEADINGS:
        for e in EXTENTS + [(P.MAX_SQ, 0, 1), (3, P.MAX_SQ, 2)]:
            o = P.offsets(h, *e)
            d2 = (o ** 2).sum(1)
            assert d2.max() <= max(e[0], e[1]) + e[2] and np.abs(o).max() <= P.radius(*e)
            assert (0, 0) in set(map(tuple, o.tolist()))
            # (y, x) order, and every row one interval of x
            key = o[:, 1] * 100000 + o[:, 0]
            assert (np.diff(key) > 0).all()
            for y in np.unique(o[:, 1]):
                xs = o[o[:, 1] == y, 0]
                assert np.array_equal(xs, np.arange(xs[0], xs[-1] + 1)), (h, e, y)
    for h in HEADINGS:
        assert P.offsets(h, 0, 0, 0).tolist() == [[0, 0]]       # zero extents: c alone


def test_the_cap_stays_below_int64():
    o = P.offsets((32767, -32767), P.MAX_SQ, P.MAX_SQ, P.MAX_SQ)
    assert P.radius(P.MAX_SQ, P.MAX_SQ, P.MAX_SQ) == 362 and np.abs(o).max() == 362 and (2 * 362 * 32767) ** 2 < 2 ** 63
    # a square of half side 256 turned by 45 degrees: its area within a cell's rim
    assert abs(len(o) - 512 * 512) < 4 * 512


# ---------------------------------------------------------------------------------------------------------- the record
def test_a_wall_through_the_footprint_ends_the_prefix():
    f = _plane((21, 30), walls=[(14, y) for y in range(21)])     # a wall one cell thick at x = 14
    e = (16, 4, 4)                                               # 4 ahead, 2 behind, 2 to either side
    cells = [(5 + k, 10) for k in range(8)]                      # along +x: the nose (x + 4) meets the wall at pose 5
    r = _one(f, cells, [(1, 0)] * 8, e, 0, P.MARGIN)
    assert _rec(r) == [1, 5, [14 + PVT[0], 8 + PVT[1]], 5, 1, 4]          # the 5 wall cells of rows 8 .. 12; pose 4's nose is one cell from it
    # the disc that holds the rectangle would stop earlier, the one inside it later
    r = _one(f, cells, [(0, 1)] * 8, e, 0, P.MARGIN)             # sideways: 2 cells towards the wall
    assert _rec(r) == [1, 7, [14 + PVT[0], 8 + PVT[1]], 7, 1, 6]
    # the wall in the MIDDLE of the footprint: the centre cell is free on either side of it
    r = _one(f, [(13, 10)], [(1, 0)], e)
    assert _rec(r) == [1, 0, [14 + PVT[0], 8 + PVT[1]], 5, -2, -2]
    # clearance_sq pads the rectangle by a disc: with 2 the cells beside the wall (dist_sq 1) block, one pose earlier
    assert _rec(_one(f, cells, [(1, 0)] * 8, e, 1, P.MARGIN)) == [1, 5, [14 + PVT[0], 8 + PVT[1]], 5, 1, 4]
    r = _one(f, cells, [(1, 0)] * 8, e, 2, P.MARGIN)
    assert _rec(r) == [1, 4, [13 + PVT[0], 8 + PVT[1]], 5, 4, 3]
    # a diagonal heading: hit is the least blocked cell in (y, x)
    r = _one(f, [(11, 10)], [(1, 1)], e)
    o = P.offsets((1, 1), *e) + np.array([11, 10])
    on = o[o[:, 0] == 14]
    assert len(on) and _rec(r) == [1, 0, [14 + PVT[0], int(on[:, 1].min()) + PVT[1]], len(on), -2, -2]


def test_outside_cells_block_unless_unknown_is_traversable():
    f = _plane((9, 12))
    e = (9, 0, 1)
    r = _one(f, [(8, 4), (9, 4)], [(1, 0)] * 2, e, 0, P.MARGIN)
    assert _rec(r) == [1, 1, [12 + PVT[0], 3 + PVT[1]], 3, -1, 0]                   # pose 1: x = 12 of rows 3, 4, 5 lies outside
    r = _one(f, [(8, 4), (9, 4)], [(1, 0)] * 2, e, 0, P.MARGIN | P.UNKNOWN_TRAVERSABLE)
    assert _rec(r) == [0, 2, [0, 0], 0, -1, 0]
    r = _one(f, [(2, 0)], [(-1, 0)], e)                          # rows -1 and columns -1: the least is (y, x) = (-1, -1)
    assert _rec(r) == [1, 0, [-1 + PVT[0], -1 + PVT[1]], 4 + 2, -2, -2]
    # an UNKNOWN cell inside blocks the same way
    f = _plane((9, 12), unknown=[(6, 4)])
    assert _rec(_one(f, [(3, 4)], [(1, 0)], e)) == [1, 0, [6 + PVT[0], 4 + PVT[1]], 1, -2, -2]
    assert _rec(_one(f, [(3, 4)], [(1, 0)], e, 0, P.UNKNOWN_TRAVERSABLE))[:2] == [0, 1]


def test_tails_and_headings_without_a_placement():
    f = _plane((9, 12), walls=[(0, 0)])
    cells = np.array([(3, 4), (4, 4), (5, 4), (6, 4)], np.float64)
    heads = [(2, 0)] * 4
    e = (1, 1, 1)
    assert _rec(_one(f, cells, heads, e, 0, P.MARGIN)) == [0, 4, [0, 0], 0, 2 * 2 + 3 * 3, 0]
    xy = _xy(cells)[None].copy()
    xy[0, 2:] = np.nan                                          # a NaN tail
    r = P.footprints(f, xy, np.asarray(heads, np.int32)[None], PVT, W, *e, 0, P.MARGIN)[0]
    assert _rec(r) == [2, 2, [0, 0], 0, 13, 0]
    for bad in ((0, 0), (40000, 0), (0, -32768), (32768, 32768)):
        r = _one(f, cells, [(2, 0), bad, (2, 0), (2, 0)], e, 0, P.MARGIN)
        assert _rec(r) == [2, 1, [0, 0], 0, 13, 0], bad
        assert _rec(_one(f, cells, [bad] * 4, e, 0, P.MARGIN)) == [2, 0, [0, 0], 0, 0, -1]
    assert _rec(_one(f, [(12, 4)], [(1, 0)], e)) == [2, 0, [0, 0], 0, -2, -2]      # outside the rectangle
    assert _rec(_one(f, cells, [(32767, -32767)] * 4, e))[:2] == [0, 4]


def test_margin_takes_the_first_pose_with_the_least_value():
    f = _plane((15, 40), walls=[(20, 0)])
    cells = [(10 + k, 7) for k in range(21)]                     # under the wall cell and on: the least at x = 20, then equal values never replace it
    r = _one(f, cells, [(1, 0)] * 21, (4, 4, 4), 0, P.MARGIN)
    assert _rec(r) == [0, 21, [0, 0], 0, 25, 8]                  # pose 8: its nose (x = 20, y = 5) is 5 rows from the wall; poses 9 .. 12 tie
    assert _rec(_one(_plane((15, 40)), cells, [(1, 0)] * 21, (4, 4, 4), 0, P.MARGIN))[4:] == [-1, 0]


def test_mask_marks_the_inside_cells_and_keeps_the_record():
    f = _plane((9, 12), walls=[(7, 4)])
    m, rec = P.mask(f, _xy([(9, 4)]), (1, 0), PVT, W, 9, 4, 1)
    want = np.zeros((9, 12), np.uint8)
    want[3:6, 7:12] = 1
    want[4, 7] = 2
    assert np.array_equal(m, want) and _rec(rec) == [1, 0, [12 + PVT[0], 3 + PVT[1]], 3 + 1, -2, -2]
    m, rec = P.mask(f, _xy([(9, 4)]), (0, 0), PVT, W, 9, 4, 1)
    assert not m.any() and rec["end"] == 2


# ---------------------------------------------------------------------------------------------------------- declarations
def test_struct_sizes_and_offsets():
    st = _capi.GroundFootprintParam
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("front_sq", 0, 4), ("back_sq", 4, 4), ("side_sq", 8, 4), ("clearance_sq", 12, 4), ("flags", 16, 4), ("reserved", 20, 12)])
    st = _capi.GroundFootprint
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("end", 0, 4), ("poses", 4, 4), ("hit", 8, 8), ("hit_cells", 16, 4), ("min_dist_sq", 20, 4), ("min_at", 24, 4), ("reserved", 28, 4)])
    for dt in (gie.GROUND_FOOTPRINT_DTYPE, P.FOOTPRINT_DTYPE):
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_] and dt.itemsize == 32
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct gie_ground_footprint_param \{(.*?)\} gie_ground_footprint_param;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|int64_t)\s+([\w, \[\]]+);", body) == [("int32_t", "front_sq"), ("int32_t", "back_sq"), ("int32_t", "side_sq"), ("int32_t", "clearance_sq"),
                                                                       ("int32_t", "flags"), ("int32_t", "reserved[3]")]
    body = re.search(r"typedef struct gie_ground_footprint \{(.*?)\} gie_ground_footprint;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|int64_t)\s+([\w, \[\]]+);", body) == [("int32_t", "end"), ("int32_t", "poses"), ("int32_t", "hit[2]"), ("int32_t", "hit_cells"),
                                                                       ("int32_t", "min_dist_sq"), ("int32_t", "min_at"), ("int32_t", "reserved")]


def test_header_binding_and_host_layer_declare_the_section():
    names = ["ground_footprints", "ground_footprints_dev", "ground_footprint_mask", "ground_footprint_mask_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES and n not in _capi.ROUND_API, n
        assert callable(getattr(gie.Mapper, n))
    assert re.search(r"#define GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE\s+1\b", txt) and re.search(r"#define GIE_GROUND_FOOTPRINT_MARGIN\s+2\b", txt)
    assert re.search(r"#define GIE_GROUND_FOOTPRINT_MAX_SQ\s+\(1 << 16\)", txt)
    assert (gie.GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE, gie.GROUND_FOOTPRINT_MARGIN, gie.GROUND_FOOTPRINT_MAX_SQ) == (P.UNKNOWN_TRAVERSABLE, P.MARGIN, P.MAX_SQ) == (1, 2, 65536)
    assert gie.GroundFootprintParam is _capi.GroundFootprintParam and gie.GroundFootprint is _capi.GroundFootprint
    assert re.search(r"int gie_ground_footprints\(gie_mapper \*h, const float \*xy, const int32_t \*heading, int n, int T, const gie_ground_footprint_param \*p, "
                     r"gie_ground_footprint \*out\);", txt)
    assert re.search(r"int gie_ground_footprints_dev\(gie_mapper \*h, const float \*d_xy, const int32_t \*d_heading, int n, int T, const gie_ground_footprint_param \*p, "
                     r"gie_ground_footprint \*d_out\);", txt)
    assert re.search(r"int gie_ground_footprint_mask\(gie_mapper \*h, const float \*xy, const int32_t \*heading, const gie_ground_footprint_param \*p, uint8_t \*mask, "
                     r"gie_ground_footprint \*rec\);", txt)
    assert re.search(r"int gie_ground_footprint_mask_dev\(gie_mapper \*h, const float \*d_xy, const int32_t \*d_heading, const gie_ground_footprint_param \*p, "
                     r"uint8_t \*d_mask, gie_ground_footprint \*d_rec\);", txt)
    assert txt.index("gie_ground_rollouts_dev") < txt.index("gie_ground_footprint_param") < txt.index("gie_costmat_compute")
    p = gie.Mapper.ground_footprint_param(None, 100, 36, 25, 4, True, True)
    assert (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags, list(p.reserved)) == (100, 36, 25, 4, 3, [0] * 3)
    p = gie.Mapper.ground_footprint_param(None, 1, 2, 3)
    assert (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags) == (1, 2, 3, 0, 0)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"int ground_local_plan_footprint\(float yaw, const float \*v, const float \*omega, int n, float dt, int T, float inflate_radius, "
                     r"std::vector<float> &poses,\s*std::vector<int32_t> &headings, std::vector<gie_ground_rollout> &records, "
                     r"std::vector<gie_ground_footprint> &footprints\)", host)
    assert '"ground/footprint"' in host and "ground_footprint_sq() const" in host
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_hip.hip")).read()
    assert src.index('#include "gie_ground_rollout.inc.h"') < src.index('#include "gie_ground_footprint.inc.h"')

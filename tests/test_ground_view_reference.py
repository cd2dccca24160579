"""tests/ground_view_ref.py (the numpy statement of include/gie.h "ground view gain"): its vectorised walk against a plain loop over
ground_los_ref.line on hand-made 9 x 9 planes, and the section's declarations in the header, the binding and the host layer.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

import gie
import ground_los_ref as L
import ground_ref as R
import ground_view_ref as V
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
U, F, O, T = R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT


def _plane(walls=(), unknown=(), fnt=()):
    t = np.full((9, 9), F, np.int8)
    for (x, y) in unknown:
        t[y, x] = U
    for (x, y) in fnt:
        t[y, x] = T
    for (x, y) in walls:
        t[y, x] = O
    return {"type": t}


def _same(f, p, r_min, r_max, normals=None, flags=0):
    m, s = V.view(f, p, r_min, r_max, W, normals, flags)
    m2, s2 = V.view_by_lines(f, p, r_min, r_max, W, normals, flags)
    assert np.array_equal(m, m2) and s.tobytes() == s2.tobytes(), (p, r_min, r_max, normals, flags)
    assert m[p[1], p[0]] == 0 and s["candidates"] == (m > 0).sum()
    t = f["type"]
    assert [s["unknown"], s["frontier"], s["occupied"]] == [((m == 2) & (t == k)).sum() for k in (U, T, O)]
    return m, s


def test_the_type_codes_are_the_mappers():
    assert (U, F, O, T) == (gie.VOX_UNKNOWN, gie.VOX_FREE, gie.VOX_OCCUPIED, gie.VOX_FNT)
    assert V.SCORE_DTYPE == gie.VIEW_SCORE_DTYPE and V.UNKNOWN_OPAQUE == gie.GROUND_VIEW_UNKNOWN_OPAQUE == 1 and V.UNION == gie.GROUND_VIEW_UNION == 2


def test_a_wall_hides_what_lies_behind_it():
    f = _plane(walls=[(x, 4) for x in range(9)], unknown=[(x, 7) for x in range(9)], fnt=[(x, 1) for x in range(9)])
    m, s = _same(f, (4, 2), 0.0, 2.0)
    # the wall is seen where the line's last step is not along the wall (|dx| <= |dy|), nothing beyond it
    assert (m[:4] == 2).sum() == 9 * 4 - 1 and m[4].tolist() == [1, 1, 2, 2, 2, 2, 2, 1, 1] and (m[5:] == 1).all()
    assert s.tolist() == (0, 9, 5, 80)
    for p in [(x, y) for x in range(9) for y in (0, 3, 5, 8)]:
        _same(f, p, 0.0, 2.0)


def test_the_tie_rule_sees_through_a_corner_gap():
    f = _plane(walls=[(3, 4), (4, 3)])                          # two cells that touch at the corner between (3, 3) and (4, 4)
    m, _ = _same(f, (2, 2), 0.0, 2.0)
    assert L.line((2, 2), (5, 5)) == [(2, 2), (3, 3), (4, 4), (5, 5)]
    assert m[4, 4] == 2 and m[5, 5] == 2 and m[8, 8] == 2       # the diagonal passes between them
    assert m[4, 3] == 2 and m[3, 4] == 2 and m[6, 4] == 1 and m[4, 6] == 1      # the two cells are seen, their shadows are not
    for p in [(x, y) for x in range(9) for y in range(9)]:
        _same(f, p, 0.0, 2.0)


def test_a_view_inside_an_obstacle_on_an_edge_and_in_a_corner():
    f = _plane(walls=[(4, 4), (5, 4), (4, 5), (5, 5), (0, 0), (8, 3)], unknown=[(1, 7), (2, 7), (7, 1)], fnt=[(6, 6), (0, 8)])
    m, s = _same(f, (4, 4), 0.0, 2.0)                           # p's own opacity is ignored, its neighbours' is not
    assert m[4, 5] == 2 and m[4, 6] == 1 and m[3, 3] == 2 and m[6, 6] == 1
    for p in ((0, 0), (8, 8), (0, 8), (8, 0), (0, 4), (4, 0), (8, 3), (4, 8)):
        m, s = _same(f, p, 0.0, 2.0)
        assert s["candidates"] == 80


def test_radii():
    f = _plane(walls=[(6, 4), (2, 2)], unknown=[(4, 7), (4, 8)])
    for p in ((4, 4), (0, 0), (8, 4)):
        m, s = _same(f, p, 0.3, 0.3)                            # r_min == r_max: the cells at distance 3 exactly (0.3 / 0.1 rounds above 3)
        rmin2, rmax2 = V.radii_sq(0.3, 0.3, W)
        assert rmin2 == rmax2 and s["candidates"] == sum(1 for y in range(9) for x in range(9) if np.float32((x - p[0]) ** 2 + (y - p[1]) ** 2) == rmin2)
        m, s = _same(f, p, 0.0, 0.0)                            # r_max == 0: v != p leaves nothing
        assert s.tolist() == (0, 0, 0, 0) and not m.any()
        m, s = _same(f, p, 0.2, 0.35)                           # a shell
        d2 = (np.arange(9)[None] - p[0]) ** 2 + (np.arange(9)[:, None] - p[1]) ** 2
        assert ((m > 0) == ((d2 >= 4) & (d2 <= 12))).all()
        m, s = _same(f, p, 0.0, 3e38)                           # any finite r_max: the quotient overflows to inf, every other cell is a candidate
        assert s["candidates"] == 80
    assert V.radii_sq(0.15, 0.15, W)[1] < np.float32(2.25) or V.radii_sq(0.15, 0.15, W)[1] >= np.float32(2.25)    # (whatever the rounding: the products decide)
    m, s = _same(f, (4, 4), 0.0, 0.15)
    assert s["candidates"] == 8


def test_planes_union_and_a_zero_normal():
    f = _plane(walls=[(6, 4), (2, 2), (4, 6)], unknown=[(4, 7), (4, 8), (0, 3)], fnt=[(7, 7)])
    p = (4, 4)
    full = _same(f, p, 0.0, 2.0)[1]["candidates"]
    assert full == 80
    m, s = _same(f, p, 0.0, 2.0, [(1, 0)])                      # x >= p_x: the column of p is inside
    assert ((m > 0) == ((np.arange(9)[None] >= 4) & ~((np.arange(9)[None] == 4) & (np.arange(9)[:, None] == 4)))).all()
    m, s = _same(f, p, 0.0, 2.0, [(1, 0), (0, 1)])              # a quadrant
    assert s["candidates"] == 24
    m, s = _same(f, p, 0.0, 2.0, [(1, 0), (0, 1)], V.UNION)     # three quadrants
    assert s["candidates"] == 80 - 16
    m, s = _same(f, p, 0.0, 2.0, [(2, 1), (2, -1)])             # a wedge of oblique normals
    assert 0 < s["candidates"] < 40
    m, s = _same(f, p, 0.0, 2.0, [(-32767, 32767), (32767, 3)], V.UNION)
    assert 40 < s["candidates"] < 80
    assert _same(f, p, 0.0, 2.0, [(0, 0)])[1]["candidates"] == 80                               # a zero normal holds for every d
    assert _same(f, p, 0.0, 2.0, [(0, 0), (1, 0)])[1]["candidates"] == 44
    assert _same(f, p, 0.0, 2.0, [(0, 0), (1, 0)], V.UNION)[1]["candidates"] == 80
    for q in ((0, 0), (8, 2), (3, 8)):
        for nr, fl in (([(1, 1)], 0), ([(-3, 1), (1, 5)], 0), ([(-3, 1), (1, 5)], V.UNION), ([(0, -1)], V.UNKNOWN_OPAQUE)):
            _same(f, q, 0.1, 0.6, nr, fl)
    # what the _dev forms score -1: no cell, a normal component beyond +-32767
    for m, s in (V.view(f, None, 0.0, 2.0, W), V.view(f, p, 0.0, 2.0, W, [(32768, 0)]), V.view(f, p, 0.0, 2.0, W, [(0, 1), (0, -32768)])):
        assert s.tolist() == (-1, -1, -1, -1) and not m.any()


def test_unknown_opaque_and_not():
    f = _plane(unknown=[(x, 5) for x in range(9)] + [(4, 7)], walls=[(1, 1)], fnt=[(x, 8) for x in range(9)])
    m0, s0 = _same(f, (4, 2), 0.0, 2.0)
    m1, s1 = _same(f, (4, 2), 0.0, 2.0, None, V.UNKNOWN_OPAQUE)
    assert (m0[5:] == 2).all() and s0["unknown"] == 10 and s0["frontier"] == 9
    assert m1[5].tolist() == [1, 2, 2, 2, 2, 2, 2, 2, 1] and (m1[6:] == 1).all() and s1["unknown"] == 7 and s1["frontier"] == 0
    assert s0["candidates"] == s1["candidates"] == 80
    assert V.opaque(f).sum() == 1 and V.opaque(f, V.UNKNOWN_OPAQUE).sum() == 11 and V.opaque(f, V.UNION).sum() == 1


def test_gain_maps_points_as_the_ground_queries_do():
    f = _plane(walls=[(6, 4)], unknown=[(0, 0)])
    pvt = (-7, 40, 0)
    xy = ((np.array([(4, 4), (0, 0), (8, 8), (9, 4), (-1, 0), (3, 3)], np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    xy[5, 0] = np.nan
    out, masks = V.gain(f, xy, pvt, 0.0, 2.0, W, masks=True)
    assert out["candidates"].tolist() == [80, 80, 80, -1, -1, -1] and out["unknown"][3:].tolist() == [-1] * 3
    assert out[0].tobytes() == V.view(f, (4, 4), 0.0, 2.0, W)[1].tobytes() and not masks[3].any()
    nr = np.array([[(1, 0)]] * 6)
    assert V.gain(f, xy, pvt, 0.0, 2.0, W, nr, 1)["candidates"].tolist() == [44, 80, 8, -1, -1, -1]


def test_struct_size_and_offsets():
    st = _capi.GroundViewParam
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("r_min", 0, 4), ("r_max", 4, 4), ("n_planes", 8, 4), ("flags", 12, 4), ("reserved", 16, 16)])
    assert C.sizeof(_capi.ViewScore) == 16 == V.SCORE_DTYPE.itemsize
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct gie_ground_view_param \{(.*?)\} gie_ground_view_param;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(float|int32_t)\s+([\w, \[\]]+);", body) == [("float", "r_min, r_max"), ("int32_t", "n_planes"), ("int32_t", "flags"), ("int32_t", "reserved[4]")]


def test_binding_and_host_layer_declare_the_section():
    names = ["ground_view_gain", "ground_view_gain_dev", "ground_view_mask", "ground_view_mask_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES and n not in _capi.ROUND_API, n
        assert callable(getattr(gie.Mapper, n))
    assert callable(gie.Mapper.ground_view_param)
    assert re.search(r"#define GIE_GROUND_VIEW_UNKNOWN_OPAQUE\s+1\b", txt) and re.search(r"#define GIE_GROUND_VIEW_UNION\s+2\b", txt)
    assert gie.GroundViewParam is _capi.GroundViewParam
    assert re.search(r"int gie_ground_view_gain_dev\(gie_mapper \*h, const float \*d_xy, const int32_t \*d_normals, int n, const gie_ground_view_param \*p, "
                     r"gie_view_score \*d_out\);", txt)
    assert re.search(r"int gie_ground_view_mask\(gie_mapper \*h, const float \*xy, const int32_t \*normals, const gie_ground_view_param \*p, uint8_t \*mask, "
                     r"gie_view_score \*score\);", txt)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"bool ground_exploration_gains\(int max_clusters, int min_size, float r_min, float r_max, std::vector<gie_ground_frontier_cluster> &clusters,\s*"
                     r"std::vector<int32_t> &steps, std::vector<gie_view_score> &scores\)", host)
    assert re.search(r"bool ground_exploration_goals\(int max_clusters, int min_size, std::vector<gie_ground_frontier_cluster> &clusters, std::vector<int32_t> &steps\)", host)

"""The numpy statement of the line-of-sight queries (tests/los_ref.py) against slower, plainer statements of the same definitions:
the voxel line against an exact rational brute force of "the cube shares a piece of positive length with the segment", the view
gain against a triple loop and against the exhaustive statement of tests/los_exact.py (no candidate radius), with the properties
of the tie radii the device tests rely on.  And the presence of the feature in the header, both libraries and the binding."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np

import gie
import los_exact as lx
import los_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gie_los_prepare", "gie_los_prepare_dev", "gie_read_los_opaque", "gie_read_los_opaque_dev", "gie_los_segments",
         "gie_los_segments_dev", "gie_view_gain", "gie_view_gain_dev"]
STRUCTS = ["gie_los_param", "gie_los_hit", "gie_view", "gie_view_param", "gie_view_score"]


def _brute(a, b):
    """the voxels whose closed cube meets the segment between the centres of a and b in a piece of positive length, ordered by
    that piece; exact (Fraction).  A float prefilter drops the voxels whose centre is a voxel or more from the line (a cube the
    line passes through has its centre within sqrt(3) / 2 of it)."""
    a, b = np.array(a, np.int64), np.array(b, np.int64)
    d = b - a
    if not d.any():
        return [tuple(int(v) for v in a)]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    g = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    t = np.clip(((g - a) @ d) / float(d @ d), 0.0, 1.0)
    near = np.linalg.norm(g - (a + t[:, None] * d), axis=1) < 1.0
    out = []
    half = Fraction(1, 2)
    for u in g[near]:
        t0, t1 = Fraction(0), Fraction(1)
        for k in range(3):
            if d[k] == 0:
                if u[k] != a[k]:
                    t1 = Fraction(-1)
                continue
            e0, e1 = (u[k] - half - a[k]) / Fraction(int(d[k])), (u[k] + half - a[k]) / Fraction(int(d[k]))
            t0, t1 = max(t0, min(e0, e1)), min(t1, max(e0, e1))
        if t1 > t0:
            out.append((t0, tuple(int(v) for v in u)))
    out.sort()
    assert len({t for t, _ in out}) == len(out)
    return [v for _, v in out]


def _check_line(a, b):
    got = lr.line(a, b)
    assert got == _brute(a, b), (a, b)
    assert got[0] == tuple(a) and got[-1] == tuple(b) and len(set(got)) == len(got)
    assert lr.line(b, a) == got[::-1]
    n = [abs(int(b[k]) - int(a[k])) for k in range(3)]
    assert 1 + max(n) <= len(got) <= 1 + sum(n)
    return got


def test_line_against_the_rational_brute_force():
    rng = np.random.default_rng(11)
    ties = 0
    for i in range(400):
        a = rng.integers(-6, 7, 3)
        if i % 4 == 0:                                         # lengths with common factors: crossings that tie
            b = a + rng.integers(-3, 4, 3) * rng.integers(1, 4)
        elif i % 4 == 1:                                       # an axis or two that do not move
            b = a + rng.integers(-9, 10, 3) * (rng.random(3) < 0.5)
        else:
            b = a + rng.integers(-9, 10, 3)
        got = _check_line(tuple(int(v) for v in a), tuple(int(v) for v in b))
        ties += len(got) < 1 + int(np.abs(b - a).sum())
    assert ties >= 100


def test_line_special_cases():
    assert lr.line((3, 4, 5), (3, 4, 5)) == [(3, 4, 5)]
    assert _check_line((0, 0, 0), (5, 0, 0)) == [(x, 0, 0) for x in range(6)]
    assert _check_line((2, 7, 1), (2, 3, 1)) == [(2, y, 1) for y in range(7, 2, -1)]
    assert _check_line((0, 0, 0), (4, 4, 0)) == [(k, k, 0) for k in range(5)]           # through the edges: diagonal moves
    assert _check_line((1, 1, 1), (4, -2, 4)) == [(1 + k, 1 - k, 1 + k) for k in range(4)]   # through the corners
    assert _check_line((0, 0, 0), (2, 1, 0)) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)]  # crossings at 1/4, 1/2, 3/4
    assert _check_line((0, 0, 0), (3, 1, 0)) == [(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 1, 0)]  # x and y tie at 1/2
    assert _check_line((0, 0, 0), (2, 2, 1)) == [(0, 0, 0), (1, 1, 0), (1, 1, 1), (2, 2, 1)]  # an x-y tie, then z alone


def test_long_line():
    a, b = (0, 15, 0), (1023, 0, 11)
    got = _check_line(a, b)
    assert 1024 <= len(got) <= 1 + 1023 + 15 + 11
    w = lr.Walk([a], [b])
    assert max(int(w.T.max()), 2047 * 1023 * 15) < 2 ** 31 * 2 ** 20       # (the device's 64-bit keys have room to spare)


def test_walk_is_line():
    """the vectorised walk of los_ref (the one segments and view_gain use) gives line()'s voxels, for all pairs at once"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 12, (300, 3))
    b = np.where(rng.random((300, 3)) < 0.2, a, rng.integers(0, 12, (300, 3)))
    b[::7] = a[::7] + rng.integers(-3, 4, (len(a[::7]), 1))                # exact diagonals
    w = lr.Walk(a, b)
    got = [[tuple(int(x) for x in v)] for v in a]
    done = np.zeros(len(a), bool)
    for _ in range(40):
        moved, last = w.step()
        assert not (moved & done).any()
        for i in np.flatnonzero(moved):
            got[i].append(tuple(int(x) for x in w.v[i]))
        done |= last | ~moved
    for i in range(len(a)):
        assert got[i] == lr.line(a[i], b[i]), i


def _gain_loops(vtype, opq, p, rmin, rmax, tan2, normals):
    """one view at local voxel p, ranges in voxels: the definition as a triple loop"""
    Z, Y, X = opq.shape
    rmin, rmax, tan2 = np.float32(rmin), np.float32(rmax), np.float32(tan2)
    cnt = {lr.UNKNOWN: 0, lr.FNT: 0, lr.OCCUPIED: 0, lr.FREE: 0}
    cand = 0
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                d = (x - p[0], y - p[1], z - p[2])
                d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if d2 == 0 or not (np.float32(d2) >= rmin * rmin and np.float32(d2) <= rmax * rmax):
                    continue
                if tan2 >= 0 and not np.float32(d[2] * d[2]) <= tan2 * np.float32(d[0] * d[0] + d[1] * d[1]):
                    continue
                if any(int(n[0]) * d[0] + int(n[1]) * d[1] + int(n[2]) * d[2] < 0 for n in normals):
                    continue
                cand += 1
                if not any(opq[v[2], v[1], v[0]] for v in lr.line(p, (x, y, z))[1:-1]):
                    cnt[int(vtype[z, y, x])] += 1
    return (cnt[lr.UNKNOWN], cnt[lr.FNT], cnt[lr.OCCUPIED], cand)


def _room():
    """9 x 9 x 7: free but for a wall across x = 4 with a one-voxel gap, never-seen voxels and frontier voxels behind it"""
    t = np.full((7, 9, 9), lr.FREE, np.int8)
    t[:, :, 4] = lr.OCCUPIED
    t[3, 4, 4] = lr.FREE                                      # the gap, straight ahead of (1, 4, 3)
    t[:, :, 7:] = lr.UNKNOWN
    t[:, :, 6] = lr.FNT
    t[0, :, :3] = lr.UNKNOWN
    return t


def _views(ps, normals=()):
    v = np.zeros(len(ps), lr.VIEW_DTYPE)
    v["pos"] = np.asarray(ps, np.float32)
    v["n_planes"] = len(normals)
    for i, n in enumerate(normals):
        v["normal"][:, i] = n
    return v


def test_view_gain_against_the_loops():
    t = _room()
    opq = lr.opaque(t, None, 0.0, 0)
    frustum = gie.view_frustum(0.1, -0.05, 1.2, 0.9)
    assert frustum.shape == (4, 3) and frustum.dtype == np.int32 and np.abs(frustum).max() <= 16384
    assert all(abs(float(np.linalg.norm(n)) - 16384.0) < 2.0 for n in frustum)
    cases = [((1, 4, 3), 0.0, 20.0, -1.0, ()), ((1, 4, 3), 2.5, 6.0, -1.0, ()), ((1, 4, 3), 0.0, 20.0, 0.25, ()),
             ((1, 4, 3), 0.0, 20.0, -1.0, [(1, 0, 0)]), ((1, 4, 3), 0.0, 9.0, -1.0, list(frustum)),
             ((0, 0, 0), 0.0, 7.0, -1.0, ()), ((8, 4, 6), 0.0, 5.0, 1.0, [(-1, 0, 0)]), ((4, 2, 3), 0.0, 8.0, -1.0, ()),
             ((5, 5, 3), 1.0, 1.0, -1.0, ())]
    for p, rmin, rmax, tan2, normals in cases:
        got = lr.view_gain(t, opq, _views([p], normals), rmin, rmax, tan2, 1.0, (0, 0, 0))[0]
        assert tuple(got) == _gain_loops(t, opq, p, rmin, rmax, tan2, normals), (p, rmin, rmax, tan2)
    # with a pivot and a voxel width: the same voxel, the same counts
    a = lr.view_gain(t, opq, _views([(1, 4, 3)]), 0.0, 20.0, -1.0, 1.0, (0, 0, 0))
    b = lr.view_gain(t, opq, _views([((1 + 10) * 0.25, (4 - 3) * 0.25, (3 + 2) * 0.25)]), 0.0, 5.0, -1.0, 0.25, (10, -3, 2))
    assert a.tobytes() == b.tobytes()
    out = lr.view_gain(t, opq, _views([(-1, 4, 3), (np.nan, 0, 0), (9, 0, 0)]), 0.0, 5.0, -1.0, 1.0, (0, 0, 0))
    assert (out.view(np.int32) == -1).all()


def test_view_gain_occlusion_by_hand():
    t = _room()
    opq = lr.opaque(t, None, 0.0, 0)
    one = lambda p, **kw: lr.view_gain(t, opq, _views([p]), kw.get("rmin", 0.0), kw.get("rmax", 30.0), -1.0, 1.0, (0, 0, 0))[0]   # noqa: E731
    # from in front of the gap: only what the gap shows; the voxel straight behind it is seen, its neighbours behind the wall are not
    seen = one((1, 4, 3))
    assert 0 < seen["unknown"] < int((t[:, :, 7:] == lr.UNKNOWN).sum()) and 0 < seen["frontier"] < 63
    line = lr.line((1, 4, 3), (8, 4, 3))
    assert (4, 4, 3) in line and not any(opq[v[2], v[1], v[0]] for v in line[1:-1])
    # the wall's own voxels are visible candidates (v may be anything) unless another voxel of the wall stands before them
    assert 9 <= seen["occupied"] < 62
    # the tie rule at a corner gap: (3, 3) -> (5, 5) in the plane passes BETWEEN the opaque (4, 3) and (3, 4) ... through (4, 4)
    c = np.full((1, 7, 7), lr.FREE, np.int8)
    c[0, 3, 4] = c[0, 4, 3] = lr.OCCUPIED
    c[0, 5, 5] = lr.UNKNOWN
    oc = lr.opaque(c, None, 0.0, 0)
    g = lr.view_gain(c, oc, _views([(3, 3, 0)]), 0.0, 3.0, -1.0, 1.0, (0, 0, 0))[0]
    assert g["unknown"] == 1 and g["occupied"] == 2
    c[0, 4, 4] = lr.OCCUPIED                                    # the diagonal voxel itself closes it
    g = lr.view_gain(c, lr.opaque(c, None, 0.0, 0), _views([(3, 3, 0)]), 0.0, 3.0, -1.0, 1.0, (0, 0, 0))[0]
    assert g["unknown"] == 0 and g["occupied"] == 3
    # a view inside an obstacle sees out: p's own opacity is ignored
    inside = one((4, 0, 3), rmax=1.0)
    assert inside["candidates"] == 5 and inside["occupied"] == 3
    # r_min cuts the shell below it
    assert one((1, 4, 3), rmin=2.0, rmax=3.0)["candidates"] == one((1, 4, 3), rmax=3.0)["candidates"] - one((1, 4, 3), rmax=1.9)["candidates"]


def _tie_scene(size):
    """types of a scene for the tie radii: the solid scene's labels taken as committed types (free next to never-seen is not
    turned into FNT here: the two statements are compared on whatever plane they are given)"""
    import planner_scenes as ps
    t = ps.solid_labels(size, 3)
    return t, lr.opaque(t, None, 0.0, 0)


def test_exhaustive_statement_against_the_radius_bounded_one():
    """tests/los_exact.py asks every voxel of the volume; los_ref.view_gain bounds its candidates by a radius derived from r_max.
    Equal on the room cases, and at every tie radius of the device test (r_max / w one float32 step either side of k)."""
    t = _room()
    opq = lr.opaque(t, None, 0.0, 0)
    frustum = gie.view_frustum(0.1, -0.05, 1.2, 0.9)
    cases = [((1, 4, 3), 0.0, 20.0, -1.0, ()), ((1, 4, 3), 2.5, 6.0, -1.0, ()), ((1, 4, 3), 0.0, 20.0, 0.25, ()),
             ((1, 4, 3), 0.0, 20.0, -1.0, [(1, 0, 0)]), ((1, 4, 3), 0.0, 9.0, -1.0, list(frustum)),
             ((0, 0, 0), 0.0, 7.0, -1.0, ()), ((8, 4, 6), 0.0, 5.0, 1.0, [(-1, 0, 0)]), ((4, 2, 3), 0.0, 8.0, -1.0, ()),
             ((5, 5, 3), 1.0, 1.0, -1.0, ()), ((4, 4, 3), 0.0, 0.0, -1.0, ()), ((4, 4, 3), 0.0, 1e18, 0.09, ())]
    for p, rmin, rmax, tan2, normals in cases:
        got = lx.view_gain(t, opq, _views([p], normals), rmin, rmax, tan2, 1.0, (0, 0, 0))[0]
        assert tuple(got) == _gain_loops(t, opq, p, rmin, rmax, tan2, normals), (p, rmin, rmax, tan2)
        assert got.tobytes() == lr.view_gain(t, opq, _views([p], normals), rmin, rmax, tan2, 1.0, (0, 0, 0))[0].tobytes()
    out = lx.view_gain(t, opq, _views([(-1, 4, 3), (np.nan, 0, 0), (9, 0, 0)]), 0.0, 5.0, -1.0, 1.0, (0, 0, 0))
    assert (out.view(np.int32) == -1).all()
    for size in lx.TIE_SIZES:
        t, opq = _tie_scene(size)
        cache = {}
        pvt = (7, -3, 2)
        for w in lx.TIE_WIDTHS:
            for k in lx.TIE_KS:
                vox = lx.tie_views(size, k)[:3 if k > 3 else 10]           # (the bounded statement walks every call anew)
                views = _views((vox + np.array(pvt)) * np.float32(w))
                for r in lx.tie_radii(k, w)[:: 1 if k in (5, 13) else 3]:
                    a = lx.view_gain(t, opq, views, 0.0, r, -1.0, w, pvt, cache=cache)
                    b = lr.view_gain(t, opq, views, 0.0, r, -1.0, w, pvt)
                    assert a.tobytes() == b.tobytes() and (a["candidates"] > 0).all(), (size, w, k, float(r))


def test_tie_radii_are_populated_and_tell_one_step_from_the_next():
    """for every tie radius k of the device test and every view used there: at least 6 voxels of the volume lie at distance exactly
    k (k = 1 and 2 have only the six axis neighbours: a view on a face, an edge or a corner keeps five, four or three of them,
    and three are asked there), the radii hold quotients r_max / w below k, at k and above k, and the candidate count differs between the two float32
    neighbours of k * w — so a candidate radius one too small cannot go unnoticed at these radii"""
    for size in lx.TIE_SIZES:
        for w in lx.TIE_WIDTHS:
            for k in lx.TIE_KS:
                radii = lx.tie_radii(k, w)
                q = [r / np.float32(w) for r in radii]
                assert len(radii) >= 3 and all(r.dtype == np.float32 for r in radii) and len({float(r) for r in radii}) == len(radii)
                # (no float32 r_max need give the quotient k itself: around 13 * 0.1 the quotients step over 13)
                lo, hi = max(r for r, v in zip(radii, q) if v < k), min(r for r, v in zip(radii, q) if v >= k)
                assert np.nextafter(lo, np.float32(np.inf)) == hi and any(v > k for v in q), (w, k, q)
                for p in lx.tie_views(size, k):
                    shell = lx.shell_count(size, p, k)
                    inner = all(0 < c < s - 1 for c, s in zip(p, size))
                    assert shell >= (6 if k >= 3 or (inner and k == 1) else lx.tie_need(k)), (size, k, p)
                    n = [int(lx.candidate_mask(size, p, *lx.thresholds(0.0, r, -1.0, w)).sum()) for r in radii[:3]]
                    assert n[2] - n[1] == shell, (size, w, k, p, n)         # the two neighbours of k * w: without and with the shell
                    assert n[0] in (n[1], n[2])


def test_elevation_ties_are_populated():
    """tan2_elev 1 and 0.25 have exact ties d_z^2 == tan2 * (d_x^2 + d_y^2): at least 20 candidates per view of the device test"""
    for size in lx.TIE_SIZES:
        for p in lx.tie_views(size, 9):
            dx, dy, dz = lx.offsets(size, p)
            for tan2, num, den in ((1.0, 1, 1), (0.25, 1, 4)):
                cand = lx.candidate_mask(size, p, *lx.thresholds(0.0, 3e38, tan2, 0.1))
                tie = (den * dz * dz == num * (dx * dx + dy * dy)) & (dz != 0)
                assert int((tie & cand).sum()) == int(tie.sum()) >= 20, (size, p, tan2, int(tie.sum()))
            flat = lx.candidate_mask(size, p, *lx.thresholds(0.0, 3e38, 0.0, 0.1))
            assert np.array_equal(flat, (dz == 0) & ((dx != 0) | (dy != 0)) & np.ones(size[::-1], bool))


def test_opaque_and_segments():
    t = _room()
    e = np.full(t.shape, 5.0, np.float32)
    e[:, :, 3:6] = 1.0
    e[:, :, 4] = 0.0
    assert lr.opaque(t, e, 0.0, 0).sum() == 62
    assert lr.opaque(t, e, 0.0, lr.UNKNOWN_OPAQUE).sum() == 62 + int((t == lr.UNKNOWN).sum())
    assert lr.opaque(t, e, 1.0, 0).sum() == 63 and lr.opaque(t, e, 1.5, 0).sum() == 3 * 63
    opq = lr.opaque(t, e, 0.0, 0)
    a = np.array([(1, 4, 3), (1, 4, 3), (8, 0, 0), (1, 1, 1), (1, 1, 1), (-1, 0, 0), (4, 0, 0), (0, 0, 0)], np.float32)
    b = np.array([(8, 4, 3), (8, 6, 3), (0, 0, 0), (1, 1, 1), (np.nan, 1, 1), (1, 1, 1), (8, 0, 0), (4, 8, 6)], np.float32)
    r = lr.segments(e, opq, a + 100, b + 100, 1.0, (100, 100, 100))
    through = lr.line((1, 4, 3), (8, 6, 3))                  # (8, 5, 3) would pass the gap's corner in a diagonal move: clear
    assert lr.segments(e, opq, [(1, 4, 3)], [(8, 5, 3)], 1.0, (0, 0, 0))[0]["first"] == -1 and through[4] == (4, 5, 3)
    assert r["first"].tolist() == [-1, 4, 4, -1, -2, -2, 0, [v[0] for v in lr.line((0, 0, 0), (4, 8, 6))].index(4)]
    assert r["len"].tolist() == [8, len(through), 9, 1, 0, 0, 5, len(lr.line((0, 0, 0), (4, 8, 6)))]
    assert r["hit"][0].tolist() == [108, 104, 103] and r["hit"][2].tolist() == [104, 100, 100] and r["hit"][4].tolist() == [0, 0, 0]
    assert r["min_edt"].tolist() == [0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 0.0]
    r2 = lr.segments(e, opq, [(0, 0, 0)], [(2, 8, 6)], 1.0, (0, 0, 0))[0]
    assert r2["first"] == -1 and r2["min_edt"] == 5.0


def _exports(path):
    import subprocess
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-nm") else "nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_the_feature_is_there():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    assert set(NAMES) <= declared
    for s in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % s, txt), s
    assert "GIE_LOS_UNKNOWN_OPAQUE" in txt
    import __graft_entry__
    if not os.path.exists(gie.LIB_PATH):
        __graft_entry__.build_hip()
    assert set(NAMES) <= _exports(gie.LIB_PATH)
    assert set(NAMES) <= _exports(__graft_entry__.build_hip_test_hooks())
    assert (C.sizeof(gie.LosHit), C.sizeof(gie.View), C.sizeof(gie.ViewScore)) == (24, 64, 16)
    assert (gie.LOS_HIT_DTYPE.itemsize, gie.VIEW_DTYPE.itemsize, gie.VIEW_SCORE_DTYPE.itemsize) == (24, 64, 16)
    assert gie.LOS_HIT_DTYPE == lr.HIT_DTYPE and gie.VIEW_DTYPE == lr.VIEW_DTYPE and gie.VIEW_SCORE_DTYPE == lr.SCORE_DTYPE
    for name in ("los_prepare", "los_prepare_dev", "read_los_opaque", "read_los_opaque_dev", "los_segments", "los_segments_dev",
                 "view_gain", "view_gain_dev"):
        assert callable(getattr(gie.Mapper, name)), name
    v = gie.make_views([(0, 0, 0), (1, 2, 3)], gie.view_frustum(0.0, 0.0, 1.0, 1.0))
    assert v.dtype == lr.VIEW_DTYPE and v["n_planes"].tolist() == [4, 4] and v["normal"][1].tolist() == gie.view_frustum(0.0, 0.0, 1.0, 1.0).tolist()

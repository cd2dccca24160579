"""tests/ground_ref.py (the numpy statement of include/gie.h "ground costmap") against a literal triple loop and an O(cells²)
brute-force distance on small grids, and the binding's view of the section.  No GPU."""
import os
import re

import numpy as np
import pytest

import ground_ref as R
from gie import _capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loops(vtype, pvt_z, z_lo, z_hi, min_known, flags):
    """the header's sentences, one voxel and one pair of cells at a time"""
    Z, Y, X = vtype.shape
    lo, hi = max(z_lo, pvt_z), min(z_hi, pvt_z + Z - 1)
    ctype = np.zeros((Y, X), np.int8)
    top = np.full((Y, X), R.NO_TOP, np.int32)
    counts = np.zeros(4, np.int32)
    for y in range(Y):
        for x in range(X):
            occ = fnt = False
            known = 0
            for gz in range(lo, hi + 1):
                t = vtype[gz - pvt_z, y, x]
                if t == R.OCCUPIED:
                    occ = True
                    top[y, x] = gz
                if t == R.FNT:
                    fnt = True
                if t in (R.FREE, R.FNT, R.OCCUPIED):
                    known += 1
            ctype[y, x] = R.OCCUPIED if occ else R.UNKNOWN if known < min_known else R.FNT if fnt else R.FREE
            counts[ctype[y, x]] += 1
    obs = [(x, y) for y in range(Y) for x in range(X)
           if ctype[y, x] == R.OCCUPIED or (flags & R.UNKNOWN_BLOCKS and ctype[y, x] == R.UNKNOWN)]
    d = np.full((Y, X), -1, np.int32)
    for y in range(Y):
        for x in range(X):
            if obs:
                d[y, x] = min((x - ox) ** 2 + (y - oy) ** 2 for ox, oy in obs)
    return ctype, top, counts, d


def volume(size, seed, p=(0.3, 0.5, 0.08, 0.12)):
    X, Y, Z = size
    return np.random.default_rng(seed).choice(4, size=(Z, Y, X), p=p).astype(np.int8)


def compare(vtype, pvt, z_lo, z_hi, min_known, flags):
    f = R.field(vtype, pvt, z_lo, z_hi, min_known, flags)
    ctype, top, counts, d = loops(vtype, pvt[2], z_lo, z_hi, min_known, flags)
    assert np.array_equal(f["type"], ctype) and np.array_equal(f["top"], top) and np.array_equal(f["counts"], counts)
    assert np.array_equal(f["dist_sq"], d)
    return f


def test_7x5x4_whole_height():
    v = volume((7, 5, 4), 1)
    f = compare(v, (-3, 2, -1), -1, 2, 1, 0)
    assert f["obs"].any() and not f["obs"].all() and f["dist_sq"].max() > 0


@pytest.mark.parametrize("flags", [0, R.UNKNOWN_BLOCKS])
@pytest.mark.parametrize("min_known", [1, 3])
@pytest.mark.parametrize("z_lo,z_hi", [(10, 12), (8, 10), (12, 40), (11, 11), (-5, 9), (13, 20)])
def test_70x9x3_bands(z_lo, z_hi, min_known, flags):
    """pivot z = 10, Z = 3: the whole height, clipped below, clipped above, one layer and two empty bands"""
    v = volume((70, 9, 3), 2, p=(0.45, 0.45, 0.02, 0.08))
    f = compare(v, (5, -4, 10), z_lo, z_hi, min_known, flags)
    if z_hi < 10 or z_lo > 12:
        assert (f["type"] == R.UNKNOWN).all() and (f["top"] == R.NO_TOP).all()
        assert (f["dist_sq"] == (0 if flags else -1)).all()
    if (z_lo, z_hi) == (10, 12) and min_known == 3 and not flags:
        assert len(np.unique(f["type"])) == 4                    # every column type occurs


def test_without_an_obstacle_and_of_obstacles_only():
    v = volume((9, 6, 3), 3, p=(0.3, 0.6, 0.0, 0.1))
    f = compare(v, (0, 0, 0), 0, 2, 1, 0)
    assert (f["dist_sq"] == -1).all() and not f["obs"].any()
    R.check_witness(np.full((6, 9, 2), R.EMPTY), f, (0, 0, 0))
    v[1] = R.OCCUPIED
    f = compare(v, (0, 0, 0), 0, 2, 1, 0)
    assert (f["dist_sq"] == 0).all() and (f["top"] == 1).all() and f["counts"].tolist() == [0, 0, 54, 0]


def test_witness_check_accepts_the_brute_force_argmin_and_refuses_a_wrong_one():
    v = volume((12, 7, 2), 4)
    pvt = (-20, 30, 0)
    f = R.field(v, pvt, 0, 1)
    oy, ox = np.nonzero(f["obs"])
    coc = np.zeros((7, 12, 2), np.int32)
    for y in range(7):
        for x in range(12):
            k = np.argmin((ox - x) ** 2 + (oy - y) ** 2)
            coc[y, x] = (ox[k] + pvt[0], oy[k] + pvt[1])
    R.check_witness(coc, f, pvt)
    far = np.argwhere(f["dist_sq"] > 0)[0]
    coc[far[0], far[1]] = (far[1] + pvt[0], far[0] + pvt[1])      # itself: in range, but no obstacle column
    with pytest.raises(AssertionError):
        R.check_witness(coc, f, pvt)


def test_costmap_and_query_follow_pos2coord():
    size, pvt, w = (7, 5, 4), (-3, 2, -1), 0.1
    f = R.field(volume(size, 1), pvt, 0, 1)
    pay, hdr = R.costmap(f, size, pvt, w, 0)
    assert pay.dtype.itemsize == 8 and pay.shape == (5, 7) and not pay["s"].any() and not pay["pad"].any()
    assert np.array_equal(np.rint(pay["d"].astype(np.float64) ** 2).astype(np.int32), f["dist_sq"]) and f["dist_sq"].max() > 1
    assert np.array_equal(pay["o"] != 0, f["type"] != R.UNKNOWN)
    assert hdr["z_size"] == 1 and hdr["z_origin"] == np.float32(0) and hdr["x_origin"] == np.float32(-3) * np.float32(w)
    none = R.field(np.ones((4, 5, 7), np.int8), pvt, 0, 1)
    assert (R.costmap(none, size, pvt, w, 0)[0]["d"] == np.float32(49 + 25 + 16)).all()
    coc = np.zeros((5, 7, 2), np.int32)
    # cell centres, the ties of pos2coord (a border belongs to the cell above it), outside, not finite
    xy = np.array([[-0.3, 0.2], [0.3, 0.6], [-0.35, 0.2], [0.35, 0.2], [0.0, 0.15], [0.0, 0.65], [np.nan, 0.2], [0.0, np.inf], [1e30, 0.2]], np.float32)
    q = R.query(f, coc, pvt, w, xy)
    cells = [(scenes.pos2coord(p[0], w) - pvt[0], scenes.pos2coord(p[1], w) - pvt[1]) for p in xy[:6]]
    assert q["inside"].tolist() == [int(0 <= x < 7 and 0 <= y < 5) for x, y in cells] + [0, 0, 0]
    assert q["inside"][:2].tolist() == [1, 1] and cells[0] == (0, 0) and cells[1] == (6, 4)
    for r, (x, y) in zip(q[:6], cells):
        if r["inside"]:
            assert r["dist_sq"] == f["dist_sq"][y, x] and r["type"] == f["type"][y, x]
    out = q[q["inside"] == 0]
    assert len(out) >= 3 and (out["dist_sq"] == -1).all() and (out["coc"] == R.EMPTY).all() and (out["type"] == R.UNKNOWN).all()


def test_binding_declares_the_section():
    """struct sizes 32 and 16, the eight symbols in include/gie.h and in the binding's table"""
    import ctypes as C
    assert C.sizeof(_capi.GroundParam) == 32 and C.sizeof(_capi.GroundCell) == 16
    assert R.CELL.itemsize == 16 and _capi.GROUND_UNKNOWN_BLOCKS == R.UNKNOWN_BLOCKS == 1
    names = ["ground_compute", "ground_compute_dev", "read_ground", "read_ground_dev", "read_costmap_ground", "read_costmap_ground_dev",
             "ground_query", "ground_query_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY, n
    assert "GIE_GROUND_UNKNOWN_BLOCKS 1" in txt

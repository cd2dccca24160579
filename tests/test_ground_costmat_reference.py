"""tests/ground_costmat_ref.py (the numpy statement of include/gie.h "ground cost matrix") against a plain queue BFS written one cell
at a time, its defining properties, and the binding's view of the section.  No GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import ground_costmat_ref as M
import ground_nf1_ref as N
import ground_ref as R
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
CLEARANCES = (0, 1, 4, 9)


def queue_matrix(ctype, dist, cells, clearance_sq, flags):
    """the header's sentences, one cell at a time: (cost, valid); cells are local (x, y), possibly outside, or None"""
    Y, X = ctype.shape

    def trav(x, y):
        t = ctype[y, x]
        if not (t == R.FREE or t == R.FNT or (t == R.UNKNOWN and flags & N.UNKNOWN_TRAVERSABLE)):
            return False
        return dist[y, x] == -1 or dist[y, x] >= clearance_sq

    n = len(cells)
    valid = [c is not None and 0 <= c[0] < X and 0 <= c[1] < Y and trav(c[0], c[1]) for c in cells]
    cost = np.full((n, n), -1, np.int32)
    for j in range(n):
        if not valid[j]:
            continue
        steps = {tuple(cells[j]): 0}
        q = collections.deque([tuple(cells[j])])
        while q:
            x, y = q.popleft()
            for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if 0 <= nx < X and 0 <= ny < Y and (nx, ny) not in steps and trav(nx, ny):
                    steps[(nx, ny)] = steps[(x, y)] + 1
                    q.append((nx, ny))
        for i in range(n):
            if valid[i]:
                cost[i, j] = steps.get(tuple(cells[i]), -1)
    return cost, np.array(valid, bool).reshape(n)


def world(cells, pvt):
    """float32 world points of local cells; None becomes NaN"""
    out = np.full((len(cells), 2), np.nan, np.float32)
    for i, c in enumerate(cells):
        if c is not None:
            out[i] = ((np.array(c) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    return out


def properties(cost, valid):
    assert cost.dtype == np.int32 and cost.shape == (len(valid), len(valid))
    assert np.array_equal(cost, cost.T)
    assert (cost[~valid] == -1).all() and (cost[:, ~valid] == -1).all()
    assert (np.diag(cost)[valid] == 0).all()
    assert (cost >= -1).all()


@pytest.mark.parametrize("ground_flags", [0, R.UNKNOWN_BLOCKS])
@pytest.mark.parametrize("size,seed", [((7, 5, 3), 1), ((70, 9, 2), 2)])
def test_reference_equals_queue_bfs(size, seed, ground_flags):
    pvt = (-3, 12, 0)
    X, Y, Z = size
    v = np.random.default_rng(seed).choice(4, size=(Z, Y, X), p=(0.2, 0.66, 0.04, 0.10)).astype(np.int8)
    f = R.field(v, pvt, 0, Z - 1, 1, ground_flags)
    rng = np.random.default_rng(seed + 10)
    seen_valid = seen_far = seen_cut = False
    for flags in (0, N.UNKNOWN_TRAVERSABLE):
        for csq in CLEARANCES:
            cells = [(int(x), int(y)) for x, y in zip(rng.integers(-2, X + 2, 14), rng.integers(-2, Y + 2, 14))]
            cells[1] = cells[0]                                 # two points on one cell
            cells += [(-1, 0), (X, Y - 1), (0, Y), None]       # outside, and one that is not finite
            xy = world(cells, pvt)
            got, valid = M.matrix(f, xy, pvt, W, csq, flags)
            want, ok = queue_matrix(f["type"], f["dist_sq"], cells, csq, flags)
            assert np.array_equal(valid, ok) and np.array_equal(got, want), (flags, csq)
            properties(got, valid)
            assert not valid[-4:].any() and valid[0] == valid[1] and np.array_equal(got[0], got[1])
            seen_valid |= valid.sum() >= 2
            seen_far |= bool((got > 2).any())
            off = ~np.eye(len(cells), dtype=bool)
            seen_cut |= bool((got[np.ix_(valid, valid)] == -1).any()) and bool((got[off] >= 0).any())
    assert seen_valid and seen_far
    if size[0] == 70 and not ground_flags:
        assert seen_cut                                         # valid points without a path between them, beside some with one


def test_two_regions_duplicates_and_points_that_are_not_valid():
    pvt = (4, -9, 0)
    lab = np.ones((1, 9, 70), np.int8)
    lab[0, :, 33] = 2                                           # a wall from edge to edge: two regions
    lab[0, 4, 10] = 2                                           # and an obstacle cell a point stands on
    f = R.field(lab, pvt, 0, 0)
    cells = [(2, 2), (30, 7), (2, 2), (40, 1), (69, 8), (33, 4), (10, 4), (-1, 3), (70, 3), (5, 9), None, (32, 0), (34, 0)]
    xy = world(cells, pvt)
    xy[10] = [np.inf, 0.0]
    xy = np.concatenate([xy, np.array([[1e30, 0.0], [0.0, -3e9], [np.nan, np.nan]], np.float32)])
    cost, valid = M.matrix(f, xy, pvt, W)
    properties(cost, valid)
    assert valid.tolist() == [True, True, True, True, True, False, False, False, False, False, False, True, True, False, False, False]
    left, right = [0, 1, 2, 11], [3, 4, 12]
    assert (cost[np.ix_(left, right)] == -1).all() and (cost[np.ix_(left, left)] >= 0).all() and (cost[np.ix_(right, right)] >= 0).all()
    assert cost[0, 2] == 0 and np.array_equal(cost[0], cost[2]) and np.array_equal(cost[:, 0], cost[:, 2])
    assert cost[0, 1] == 28 + 5 and cost[3, 4] == 29 + 7 and cost[11, 12] == -1      # L1 where nothing is in the way; neighbours of the wall
    want, ok = queue_matrix(f["type"], f["dist_sq"], cells + [None] * 3, 0, 0)
    assert np.array_equal(cost, want) and np.array_equal(valid, ok)
    # at clearance_sq 4 the cells within two of the wall or of the obstacle cell are not traversable
    cost4, valid4 = M.matrix(f, xy, pvt, W, 4)
    assert not valid4[11] and not valid4[12] and valid4[0] and cost4[0, 1] == 33
    assert np.array_equal(cost4, queue_matrix(f["type"], f["dist_sq"], cells + [None] * 3, 4, 0)[0])
    # no point, one point, all points invalid
    c0, v0 = M.matrix(f, np.zeros((0, 2), np.float32), pvt, W)
    assert c0.shape == (0, 0) and v0.shape == (0,)
    c1, v1 = M.matrix(f, xy[:1], pvt, W)
    assert c1.tolist() == [[0]] and v1.tolist() == [True]
    cb, vb = M.matrix(f, xy[5:11], pvt, W)
    assert (cb == -1).all() and not vb.any()


def test_a_field_without_an_obstacle_column_gives_l1():
    pvt = (5, -4, 0)
    f = R.field(np.ones((1, 5, 7), np.int8), pvt, 0, 0)
    assert (f["dist_sq"] == -1).all()                           # -1 passes every clearance
    cells = [(x, y) for y in range(5) for x in range(7)]
    c = np.array(cells)
    l1 = np.abs(c[:, None, :] - c[None, :, :]).sum(axis=2)
    for csq in CLEARANCES:
        cost, valid = M.matrix(f, world(cells, pvt), pvt, W, csq)
        assert valid.all() and np.array_equal(cost, l1)
    with pytest.raises(AssertionError):
        M.matrix(f, world(cells, pvt), pvt, W, 0, N.FROM_FRONTIERS)
    unk = R.field(np.zeros((1, 5, 7), np.int8), pvt, 0, 0)    # never seen: traversable with the flag only
    assert not M.matrix(unk, world(cells, pvt), pvt, W, 0, 0)[1].any()
    cost, valid = M.matrix(unk, world(cells, pvt), pvt, W, 0, N.UNKNOWN_TRAVERSABLE)
    assert valid.all() and np.array_equal(cost, l1)


def test_binding_declares_the_section():
    """the two symbols in include/gie.h and in the binding's device-only table only, on ground NF1's parameters; 256 points"""
    names = ["ground_costmat_compute", "ground_costmat_compute_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    assert re.search(r"#define\s+GIE_GROUND_COSTMAT_MAX_POINTS\s+256\b", txt) and M.MAX_POINTS == 256
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES, n
        res, args = _capi.DEVICE_ONLY[n]
        assert res is C.c_int and len(args) == 6 and args[3] == C.POINTER(_capi.GroundNf1Param)
    import gie
    assert hasattr(gie.Mapper, "ground_costmat") and hasattr(gie.Mapper, "ground_costmat_dev")
    assert txt.index("gie_ground_nf1_query_dev") < txt.index("gie_ground_costmat_compute") < txt.index("GIE_COSTMAT_MAX_POINTS")

"""tests/ground_nf1_ref.py (the numpy statement of include/gie.h "ground navigation function") against a plain queue BFS written
one cell at a time, the path and CostMap statements against the header's sentences, and the binding's view of the section.  No GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import ground_nf1_ref as N
import ground_ref as R
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
CLEARANCES = (0, 1, 2, 4, 5, 9)


def bfs(ctype, dist, goal_cells, clearance_sq, flags):
    """the header's sentences, one cell at a time: (nf1, number of sources)"""
    Y, X = ctype.shape

    def trav(x, y):
        t = ctype[y, x]
        if not (t == R.FREE or t == R.FNT or (t == R.UNKNOWN and flags & N.UNKNOWN_TRAVERSABLE)):
            return False
        return dist[y, x] == -1 or dist[y, x] >= clearance_sq

    nf = np.full((Y, X), -1, np.int32)
    q = collections.deque()
    cand = [c for c in goal_cells if 0 <= c[0] < X and 0 <= c[1] < Y]
    if flags & N.FROM_FRONTIERS:
        cand += [(x, y) for y in range(Y) for x in range(X) if ctype[y, x] == R.FNT]
    for x, y in cand:
        if trav(x, y) and nf[y, x] < 0:
            nf[y, x] = 0
            q.append((x, y))
    n_src = len(q)
    while q:
        x, y = q.popleft()
        for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= nx < X and 0 <= ny < Y and nf[ny, nx] < 0 and trav(nx, ny):
                nf[ny, nx] = nf[y, x] + 1
                q.append((nx, ny))
    return nf, n_src


def volume(size, seed, p):
    X, Y, Z = size
    return np.random.default_rng(seed).choice(4, size=(Z, Y, X), p=p).astype(np.int8)


def goals_of(rng, size, pvt, n):
    """n goal cells, some of them outside the rectangle: (cells local, world points float32)"""
    cells = np.stack([rng.integers(-2, size[0] + 2, n), rng.integers(-2, size[1] + 2, n)], 1)
    xy = ((cells + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    return [tuple(c) for c in cells], xy


def compare(f, size, pvt, seed, n_goals=3):
    rng = np.random.default_rng(seed)
    seen = set()
    for flags in (0, 1, 2, 3):
        for csq in CLEARANCES:
            cells, xy = goals_of(rng, size, pvt, n_goals)
            got, n_got = N.field(f, xy, pvt, W, csq, flags)
            want, n_want = bfs(f["type"], f["dist_sq"], cells, csq, flags)
            assert np.array_equal(got, want), (flags, csq)
            assert n_got == n_want == int((got == 0).sum()), (flags, csq)
            seen.add((n_got > 0, int(got.max()) > 2))
    return seen


@pytest.mark.parametrize("ground_flags", [0, R.UNKNOWN_BLOCKS])
@pytest.mark.parametrize("size,seed", [((7, 5, 3), 1), ((70, 9, 2), 2)])
def test_dilation_equals_queue_bfs(size, seed, ground_flags):
    pvt = (-3, 12, 0)
    v = volume(size, seed, (0.2, 0.66, 0.04, 0.10))
    f = R.field(v, pvt, 0, size[2] - 1, 1, ground_flags)
    seen = compare(f, size, pvt, seed)
    assert (True, True) in seen                                 # some case has sources and a field more than two steps deep
    if size[0] == 70:
        assert {R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT} <= set(np.unique(f["type"]))


def test_no_source_all_blocked_and_no_obstacle():
    size, pvt = (70, 9, 1), (5, -4, 0)
    free = R.field(np.ones((1, 9, 70), np.int8), pvt, 0, 0)
    assert (free["dist_sq"] == -1).all()                        # no obstacle column: -1 passes every clearance
    centre = np.array([[(5 + 40) * W, (-4 + 4) * W]], np.float32)
    for csq in CLEARANCES:
        nf, n = N.field(free, centre, pvt, W, csq)
        assert n == 1 and nf[4, 40] == 0 and nf.min() == 0 and nf.max() == 40 + 4
        assert np.array_equal(nf, bfs(free["type"], free["dist_sq"], [(40, 4)], csq, 0)[0])
    nf, n = N.field(free, np.zeros((0, 2), np.float32), pvt, W)                    # no source
    assert n == 0 and (nf == -1).all()
    nf, n = N.field(free, np.array([[np.nan, 0.0], [1e30, 0.0], [0.0, -np.inf], [(5 - 1) * W, 0.0]], np.float32), pvt, W)
    assert n == 0 and (nf == -1).all()                          # goals that are not finite, or outside
    full = R.field(np.full((1, 9, 70), 2, np.int8), pvt, 0, 0)                     # all blocked
    nf, n = N.field(full, centre, pvt, W, 0, 3)
    assert n == 0 and (nf == -1).all()
    unk = R.field(np.zeros((1, 9, 70), np.int8), pvt, 0, 0, 1, R.UNKNOWN_BLOCKS)   # UNKNOWN columns block: distance 0 everywhere
    assert N.field(unk, centre, pvt, W, 0, N.UNKNOWN_TRAVERSABLE)[1] == 1 and N.field(unk, centre, pvt, W, 1, N.UNKNOWN_TRAVERSABLE)[1] == 0
    assert N.field(unk, centre, pvt, W, 0, 0)[1] == 0


def test_path_rule_ties_truncation_and_starts_without_a_path():
    pvt = (-3, 7, 0)
    nf = N.propagate(np.ones((5, 7), bool), np.array([[x == 0 and y == 4 for x in range(7)] for y in range(5)]))      # source (0, 4)
    assert nf[0, 6] == 10
    starts = np.array([[(-3 + 3) * W, (7 + 2) * W], [(-3 + 9) * W, 7 * W], [np.nan, 0.0]], np.float32)
    p, ln = N.path(nf, starts, pvt, W, 16, fill=-7)
    assert ln.tolist() == [6, 0, 0] and (p[1:] == -7).all() and (p[0, 6:] == -7).all()
    # from (3, 2), value 5: -x and +y both hold 4, -x comes first in the order -x +x -y +y; at x = 0 only +y is left
    assert (p[0, :6] - np.array(pvt[:2])).tolist() == [[3, 2], [2, 2], [1, 2], [0, 2], [0, 3], [0, 4]]
    p3, ln3 = N.path(nf, starts, pvt, W, 3, fill=-7)
    assert ln3.tolist() == [6, 0, 0] and np.array_equal(p3[0], p[0, :3])          # truncated: len says how long it would have been
    wall = np.ones((5, 7), bool)
    wall[:, 3] = False
    nf2 = N.propagate(wall, np.array([[x == 0 and y == 0 for x in range(7)] for y in range(5)]))
    assert (nf2[:, 3:] == -1).all()
    assert N.path(nf2, np.array([[(-3 + 5) * W, (7 + 1) * W]], np.float32), pvt, W, 4)[1].tolist() == [0]     # unreachable


def test_costmap_bytes():
    size, pvt = (7, 5, 3), (-3, 2, -1)
    f = R.field(volume(size, 1, (0.3, 0.6, 0.02, 0.08)), pvt, -1, 1)
    nf, _ = N.field(f, np.zeros((0, 2), np.float32), pvt, W, 0, N.FROM_FRONTIERS)
    pay, hdr = N.costmap(nf, f, size, pvt, W, -1)
    assert pay.dtype.itemsize == 8 and pay.shape == (5, 7) and not pay["s"].any() and not pay["pad"].any()
    assert np.array_equal(pay["d"], np.where(nf < 0, np.float32(-1), nf.astype(np.float32))) and (nf == -1).any() and nf.max() > 0
    assert np.array_equal(pay["o"] != 0, f["type"] != R.UNKNOWN)
    assert hdr["type"] == 2 and hdr["z_size"] == 1 and hdr["z_origin"] == np.float32(-1) * np.float32(W) and hdr["x_size"] == 7
    assert hdr["x_origin"] == np.float32(-3) * np.float32(W)


def test_binding_declares_the_section():
    """the struct's 32 bytes, the flag values, the eight symbols in include/gie.h and in the binding's device-only table"""
    assert C.sizeof(_capi.GroundNf1Param) == 32
    assert _capi.GROUND_NF1_UNKNOWN_TRAVERSABLE == N.UNKNOWN_TRAVERSABLE == 1 and _capi.GROUND_NF1_FROM_FRONTIERS == N.FROM_FRONTIERS == 2
    names = ["ground_nf1_compute", "ground_nf1_compute_dev", "read_ground_nf1", "read_ground_nf1_dev", "ground_nf1_path", "ground_nf1_path_dev",
             "read_costmap_ground_nf1", "read_costmap_ground_nf1_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    for n in names:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES, n
    assert "GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE 1" in txt and "GIE_GROUND_NF1_FROM_FRONTIERS 2" in txt

"""The numpy statement of the cost matrix (tests/costmat_ref.py) against scipy's shortest paths on the 6-connected grid graph, its
defining properties, and the section's presence in the header, the binding and the library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gie
from gie import _capi

import costmat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy_matrix(trav, vox):
    """all-pairs steps among the voxels over the grid graph of the traversable voxels: -1 where there is no path"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path
    Z, Y, X = trav.shape
    idx = np.arange(Z * Y * X).reshape(Z, Y, X)
    rows, cols = [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        both = trav[tuple(lo)] & trav[tuple(hi)]
        rows.append(idx[tuple(lo)][both])
        cols.append(idx[tuple(hi)][both])
    r, c = np.concatenate(rows), np.concatenate(cols)
    g = coo_matrix((np.ones(len(r)), (r, c)), shape=(idx.size, idx.size)).tocsr()
    src = (vox[:, 2] * Y + vox[:, 1]) * X + vox[:, 0]
    d = shortest_path(g, method="D", directed=False, unweighted=True, indices=src)[:, src]
    ok = trav[vox[:, 2], vox[:, 1], vox[:, 0]]
    out = np.where(np.isfinite(d), d, -1).astype(np.int32)
    out[~ok, :] = -1
    out[:, ~ok] = -1
    return out, ok


@pytest.mark.parametrize("size", [(13, 9, 7), (70, 5, 1), (9, 9, 9)])
@pytest.mark.parametrize("fill", [0.0, 0.55, 0.75, 1.0])
def test_reference_equals_scipy_shortest_paths(size, fill):
    X, Y, Z = size
    rng = np.random.default_rng(X * 7 + int(fill * 100))
    trav = rng.random((Z, Y, X)) < fill                         # fill 0: no traversable voxel; fill 1: all of them
    vox = rng.integers(0, np.array(size), size=(20, 3))
    vox[1] = vox[0]                                             # two points on one voxel
    got, valid = R.matrix_of_voxels(trav, vox, np.ones(len(vox), bool))
    want, ok = _scipy_matrix(trav, vox)
    assert np.array_equal(valid, ok) and np.array_equal(got, want)
    if fill == 0.0:
        assert (got == -1).all() and not valid.any()
    if fill == 1.0:
        l1 = np.abs(vox[:, None, :] - vox[None, :, :]).sum(axis=2)
        assert valid.all() and np.array_equal(got, l1)


def test_symmetry_coincident_points_and_invalid_rows():
    size, w, pvt = (21, 17, 6), np.float32(0.2), (-5, 3, 40)
    X, Y, Z = size
    rng = np.random.default_rng(2)
    vtype = rng.choice(np.array([0, 1, 1, 1, 2, 3], np.int8), size=(Z, Y, X))
    edt = rng.uniform(0.0, 3.0, (Z, Y, X)).astype(np.float32)
    vox = rng.integers(0, np.array(size), size=(30, 3))
    pts = ((vox + np.array(pvt)).astype(np.float32) * w).astype(np.float32)
    pts[3] = pts[2]                                             # the same voxel
    pts[4] = [np.nan, 0, 0]
    pts[5] = ((np.array([X, 0, 0]) + np.array(pvt)).astype(np.float32) * w)      # one voxel beyond the volume
    pts[6, 2] = np.inf
    seen_finite = False
    for cl, flags in ((0.0, 0), (1.0, 0), (0.0, 1), (1.5, 1)):
        cost, valid = R.matrix(vtype, edt, pts, cl, flags, w, pvt)
        assert cost.dtype == np.int32 and cost.shape == (30, 30)
        assert np.array_equal(cost, cost.T)
        assert not valid[4] and not valid[5] and not valid[6]
        assert (cost[~valid] == -1).all() and (cost[:, ~valid] == -1).all()
        assert (np.diag(cost)[valid] == 0).all()
        assert valid[2] == valid[3] and np.array_equal(cost[2], cost[3])
        if valid[2]:
            assert cost[2, 3] == 0
        trav = R.nf1_ref.traversable(vtype, edt, cl, flags)
        v, inside = R.nf1_ref.point_voxels(pts, w, pvt, size)
        for i in np.flatnonzero(valid):
            assert inside[i] and trav[v[i, 2], v[i, 1], v[i, 0]]
        seen_finite |= bool((cost[~np.eye(30, dtype=bool)] > 0).any())
    assert seen_finite
    with pytest.raises(AssertionError):
        R.matrix(vtype, edt, pts, 0.0, R.nf1_ref.FROM_FRONTIERS, w, pvt)


def test_header_binding_and_library_have_the_section():
    """both symbols are declared in include/gie.h with GIE_COSTMAT_MAX_POINTS = 64, have their signatures in gie._capi, and the
    library built without a GPU exports them"""
    names = ["costmat_compute", "costmat_compute_dev"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    assert re.search(r"#define\s+GIE_COSTMAT_MAX_POINTS\s+64\b", txt) and R.MAX_POINTS == 64
    for n in names:
        assert "gie_" + n in declared, n
        assert n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES, n
        res, args = _capi.DEVICE_ONLY[n]
        assert res is C.c_int and len(args) == 6 and args[3] == C.POINTER(_capi.Nf1Param)
    if not os.path.exists(gie.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    lib = C.CDLL(gie.LIB_PATH)
    for n in names:
        assert hasattr(lib, "gie_" + n), n
    assert hasattr(gie.Mapper, "costmat") and hasattr(gie.Mapper, "costmat_dev")

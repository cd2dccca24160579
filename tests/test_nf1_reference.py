"""The numpy statement of the NF1 navigation function (tests/nf1_ref.py) against scipy's graph shortest paths on small random
masks, and its local certificate: it accepts the BFS field and rejects perturbed ones.  CPU only."""
import numpy as np
import pytest

import nf1_ref

sp = pytest.importorskip("scipy.sparse")
csgraph = pytest.importorskip("scipy.sparse.csgraph")


def _graph_field(trav, src):
    """the field by multi-source unweighted shortest paths over the 6-connected graph of the traversable voxels"""
    idx = np.arange(trav.size).reshape(trav.shape)
    rows, cols = [], []
    for ax in range(3):
        if trav.shape[ax] < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        both = trav[tuple(lo)] & trav[tuple(hi)]
        rows.append(idx[tuple(lo)][both])
        cols.append(idx[tuple(hi)][both])
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    c = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    n = trav.size + 1                                          # node n - 1: a super source joined to every source
    s = idx[src & trav]
    r = np.concatenate([r, np.full(len(s), n - 1)])
    c = np.concatenate([c, s])
    g = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    d = csgraph.shortest_path(g, directed=False, unweighted=True, indices=n - 1)[:-1]
    return np.where(np.isfinite(d), d - 1, -1).astype(np.int32).reshape(trav.shape)


def _case(rng, shape, p_trav, n_src, faces=False):
    trav = rng.random(shape) < p_trav
    src = np.zeros(shape, bool)
    for _ in range(n_src):
        v = [int(rng.integers(0, s)) for s in shape]
        if faces:
            ax = int(rng.integers(0, 3))
            v[ax] = 0 if rng.random() < 0.5 else shape[ax] - 1
        src[tuple(v)] = True
    return trav, src


@pytest.mark.parametrize("shape,p_trav,n_src,faces", [
    ((9, 11, 13), 0.7, 3, False),
    ((7, 6, 17), 0.6, 1, False),
    ((1, 23, 31), 0.65, 2, False),              # Z = 1
    ((5, 9, 8), 0.75, 4, True),                 # sources on faces
    ((6, 7, 5), 0.7, 0, False),                 # no source
    ((8, 9, 10), 1.0, 2, False),                # all traversable
    ((13, 3, 1), 0.8, 1, False),
    ((11, 12, 10), 0.45, 5, False),             # many components
    ((19, 23, 1), 0.75, 2, True),               # array shapes [Z][Y][X]: X = 1 ...
    ((17, 1, 29), 0.8, 2, False),               # ... and Y = 1, the flat volumes of the device test's shape table
])
def test_bfs_equals_graph_shortest_paths(shape, p_trav, n_src, faces):
    rng = np.random.default_rng(sum(shape) * 7 + n_src)
    for _ in range(3):
        trav, src = _case(rng, shape, p_trav, n_src, faces)
        f = nf1_ref.bfs(trav, src)
        assert np.array_equal(f, _graph_field(trav, src))
        assert nf1_ref.certificate(f, trav, src) == ""
        if n_src == 0:
            assert (f == -1).all()
        if p_trav == 1.0:
            assert (f >= 0).all()


def test_traversable_and_sources_follow_the_statement():
    T = np.array([[[0, 1, 2, 3, 1, 3, 0]]], np.int8)
    edt = np.array([[[5.0, 1.49999, 0.0, 2.0, 1.5, 1.0, 0.5]]], np.float32)
    assert nf1_ref.traversable(T, edt, 1.5).tolist() == [[[False, False, False, True, True, False, False]]]
    assert nf1_ref.traversable(T, edt, 0.0).tolist() == [[[False, True, False, True, True, True, False]]]
    tr = nf1_ref.traversable(T, edt, 0.0, nf1_ref.UNKNOWN_TRAVERSABLE)
    assert tr.tolist() == [[[True, True, False, True, True, True, True]]]
    # goals: metres at w = 0.5, pivot x = 10: voxel floor(p / w + 0.5) - 10; outside / not finite ones ignored
    goals = np.array([[5.0, 0, 0], [6.5, 0, 0], [4.0, 0, 0], [np.nan, 0, 0], [5.1, 0.3, 0], [1e30, 0, 0]], np.float32)
    src = nf1_ref.sources(T, tr, goals, 0.5, (10, 0, 0), 0)
    assert src.tolist() == [[[True, False, False, True, False, False, False]]]
    src = nf1_ref.sources(T, tr, (), 0.5, (10, 0, 0), nf1_ref.FROM_FRONTIERS)
    assert src.tolist() == [[[False, False, False, True, False, True, False]]]
    f = nf1_ref.bfs(nf1_ref.traversable(T, edt, 0.0), src)
    assert f.tolist() == [[[-1, -1, -1, 0, 1, 0, -1]]]


def test_descent_rule_and_truncation():
    trav = np.ones((3, 4, 5), bool)
    src = np.zeros_like(trav)
    src[0, 0, 0] = True
    f = nf1_ref.bfs(trav, src)
    p = nf1_ref.descend(f, (4, 3, 2))
    assert len(p) == f[2, 3, 4] + 1 == 10
    assert p[0] == (4, 3, 2) and p[-1] == (0, 0, 0)
    assert p[1] == (3, 3, 2)                                   # -x first
    for a, b in zip(p, p[1:]):
        assert sum(abs(i - j) for i, j in zip(a, b)) == 1
        assert f[b[2], b[1], b[0]] == f[a[2], a[1], a[0]] - 1
    starts = np.array([[4, 3, 2], [0, 0, 0], [9, 0, 0]], np.float32)     # w = 1, pivot (1, 2, 3): global = local + pivot
    out, lens = nf1_ref.paths(f, starts + np.array([1, 2, 3], np.float32), 1.0, (1, 2, 3), 4)
    assert lens.tolist() == [10, 1, 0]
    assert out[0].shape == (4, 3) and out[0][0].tolist() == [5, 5, 5]
    assert out[1].tolist() == [[1, 2, 3]] and out[2].shape == (0, 3)


def test_certificate_accepts_the_bfs_and_rejects_perturbations():
    rng = np.random.default_rng(11)
    trav, src = _case(rng, (24, 40, 48), 0.72, 4)
    f = nf1_ref.bfs(trav, src)
    assert nf1_ref.certificate(f, trav, src) == ""
    reached = np.argwhere(f > 0)
    unreached = np.argwhere(trav & (f < 0))
    assert len(reached) > 1000 and len(unreached) > 0
    for k in range(20):
        g = f.copy()
        v = tuple(reached[rng.integers(len(reached))])
        g[v] += 1 if k % 2 else -1                             # a value off by one
        assert nf1_ref.certificate(g, trav, src) != ""
    g = f.copy()
    g[tuple(reached[0])] = -1                                  # a hole
    assert nf1_ref.certificate(g, trav, src) != ""
    g = f.copy()
    g[tuple(unreached[0])] = 7                                 # a value where no path leads
    assert nf1_ref.certificate(g, trav, src) != ""
    g = f.copy()
    g[tuple(np.argwhere(src)[0])] = 1                          # a source lost
    assert nf1_ref.certificate(g, trav, src) != ""
    g = f.copy()
    g[tuple(np.argwhere(~trav)[0])] = 3                        # a value in an obstacle
    assert nf1_ref.certificate(g, trav, src) != ""
    g = np.where(f > 0, f + 1, f)                              # every non-source value shifted
    assert nf1_ref.certificate(g, trav, src) != ""

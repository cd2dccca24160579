"""The goal-to-goal cost matrix on the device (include/gie.h gie_costmat_compute*) against the numpy statement of
tests/costmat_ref.py, computed from read_local's type and edt at the same point of the mapper's stream.  Every comparison is
bit for bit."""
import ctypes as C

import numpy as np
import pytest

import costmat_ref
import nf1_ref
from gie import scenes
from stage_common import W, box_labels, mapper as _mapper, serpentine_labels, stage_calls_change_nothing, update as _update, world as _world

pytestmark = pytest.mark.gpu


def _reference(m, loc, pts, clearance=0.0, unknown=False):
    cv = np.float32(clearance) / np.float32(m.cfg.voxel_width)
    return costmat_ref.matrix(loc["type"], loc["edt"], pts, cv, nf1_ref.UNKNOWN_TRAVERSABLE if unknown else 0, m.cfg.voxel_width, m.pivot())


def _check(m, loc, pts, clearance=0.0, unknown=False, ref=None):
    """costmat (clearance in metres) against the reference on read_local's planes: (cost, valid)"""
    cost, valid = m.costmat(pts, clearance, unknown)
    rc, rv = ref if ref is not None else _reference(m, loc, pts, clearance, unknown)
    assert cost.dtype == np.int32 and cost.shape == (len(pts), len(pts))
    assert np.array_equal(valid, rv), (valid, rv)
    assert np.array_equal(cost, rc), (int((cost != rc).sum()), cost[cost != rc][:8], rc[cost != rc][:8])
    return cost, valid


# ---- 1. random boxes -------------------------------------------------------------------------------------------------------------
SIZES = [(96, 80, 72), (97, 61, 45), (77, 53, 1)]
N_POINTS = 24
SEALED = 9                                                      # index of the point inside the closed hollow box


def _box_scene(size):
    """labels [Z][Y][X]: an unknown slab x < 5, random boxes, free corridors of half-width 3 that join the hand-placed points
    (clearance 2 voxels holds along their axes whatever the boxes do), and a closed hollow box of 9^3 (7^3 inside) away from them;
    the hand-placed local voxels"""
    X, Y, Z = size
    rng = np.random.default_rng(sum(size))
    lab = np.ones((Z, Y, X), np.int8)
    for _ in range(14):
        s = rng.integers(4, 22, size=3)
        lo = rng.integers(0, np.array(size))
        lab[lo[2]:lo[2] + s[2], lo[1]:lo[1] + s[1], lo[0]:lo[0] + s[0]] = 2
    lab[:, :, :5] = 0
    zc = Z // 2
    zs = slice(max(zc - 3, 0), zc + 4)
    lab[zs, 17:24, 6:70] = 1                                    # the spine along x at y = 20, across x = 63 / 64
    lab[zs, 3:24, 27:34] = 1                                    # a branch to y = 7 / 8, across the y tile border
    lab[zs, 17:34, 37:44] = 1                                   # a branch to y = 30
    hz = slice(max(zc - 4, 0), zc + 5)
    lab[hz, 40:49, 66:75] = 2                                   # the hollow box: shell ...
    lab[zs, 41:48, 67:74] = 1                                   # ... and inside (Z = 1: a ring, sealed by the volume's faces)
    hand = {"x63": (63, 20, zc), "x64": (64, 20, zc), "y7": (30, 7, zc), "y8": (30, 8, zc), "twin": (40, 30, zc), "sealed": (70, 44, zc)}
    return lab, hand


@pytest.fixture(scope="module", params=SIZES, ids=lambda v: "x".join(map(str, v)))
def box_scene(request):
    size = request.param
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        lab, hand = _box_scene(size)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        assert (loc["type"] == nf1_ref.FNT).any() and (loc["type"] == nf1_ref.OCCUPIED).any() and (loc["type"] == nf1_ref.UNKNOWN).any()
        rng = np.random.default_rng(5 + sum(size))
        # the free points: voxels the strictest setting (2 voxels of clearance, unknown closed) reaches from the spine, so that every
        # setting connects them
        strict = nf1_ref.traversable(loc["type"], loc["edt"], np.float32(0.2) / np.float32(W), 0)
        src = np.zeros(strict.shape, bool)
        x, y, z = hand["x63"]
        src[z, y, x] = True
        reach = np.argwhere(nf1_ref.bfs(strict, src) > 0)[:, ::-1]
        free = reach[rng.choice(len(reach), N_POINTS - 10, replace=False)]
        occ = np.argwhere(loc["type"] == nf1_ref.OCCUPIED)[:1, ::-1]
        jit = rng.uniform(-0.4, 0.4, (N_POINTS, 3))
        vox = np.array([hand["x63"], hand["x64"], hand["y7"], hand["y8"], hand["twin"], hand["twin"], (-6, 0, 0), (0, 0, 0), tuple(occ[0]),
                        hand["sealed"]] + [tuple(v) for v in free])
        pts = _world(m, vox, jit)
        pts[7, 1] = np.nan
        assert len(pts) == N_POINTS
        yield m, loc, pts
    finally:
        m.close()


@pytest.mark.parametrize("unknown", [False, True])
@pytest.mark.parametrize("clearance", [0.0, 0.2])
def test_random_boxes(box_scene, clearance, unknown):
    m, loc, pts = box_scene
    rc, rv = ref = _reference(m, loc, pts, clearance, unknown)
    # the scene's guarantees, on the REFERENCE: a matrix of all -1 cannot pass
    assert rv.tolist()[:10] == [True] * 6 + [False] * 3 + [True] and rv[10:].all()
    vi = np.flatnonzero(rv)
    sub = rc[np.ix_(vi, vi)]
    off = ~np.eye(len(vi), dtype=bool)
    assert (sub[off] >= 0).mean() >= 0.25
    assert (np.delete(rc[SEALED], SEALED) == -1).all() and rc[SEALED, SEALED] == 0
    assert rc[0, 1] == 1 and rc[2, 3] == 1 and rc[4, 5] == 0 and np.array_equal(rc[4], rc[5])
    cost, valid = _check(m, loc, pts, clearance, unknown, ref=ref)
    assert np.array_equal(cost, cost.T)


# ---- 4. against the shipped NF1 on the device -------------------------------------------------------------------------------------
def test_against_nf1_fields_on_the_device(box_scene):
    m, loc, pts = box_scene
    X, Y, Z = m.size
    cost, valid = m.costmat(pts, 0.2, True)
    vox, inside = nf1_ref.point_voxels(pts, m.cfg.voxel_width, m.pivot(), (X, Y, Z))
    assert valid.sum() >= N_POINTS - 3
    for j in range(len(pts)):
        ns = m.nf1_compute(pts[j:j + 1], 0.2, True, False)
        assert ns == int(valid[j])
        f = m.read_nf1()
        col = np.array([f[vox[i, 2], vox[i, 1], vox[i, 0]] if inside[i] else -1 for i in range(len(pts))], np.int32)
        assert np.array_equal(col, cost[:, j]), j


# ---- 2. n at its limits -----------------------------------------------------------------------------------------------------------
def _small_scene(size, seed=1):
    X, Y, Z = size
    rng = np.random.default_rng(seed)
    lab = np.ones((Z, Y, X), np.int8)
    for _ in range(6):
        s = rng.integers(2, 9, size=3)
        lo = rng.integers(0, np.array(size))
        lab[lo[2]:lo[2] + s[2], lo[1]:lo[1] + s[1], lo[0]:lo[0] + s[0]] = 2
    return lab


@pytest.fixture(scope="module")
def small():
    size = (70, 24, 10)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        for _ in range(2):
            _update(m, pos, q, _small_scene(size))
        yield m, size
    finally:
        m.close()


def _free_points(m, loc, rng, k, clearance=0.0):
    trav = nf1_ref.traversable(loc["type"], loc["edt"], np.float32(clearance) / np.float32(m.cfg.voxel_width), 0)
    cells = np.argwhere(trav)[:, ::-1]
    return _world(m, cells[rng.choice(len(cells), k, replace=False)], rng.uniform(-0.4, 0.4, (k, 3)))


def test_n_at_its_limits(small):
    m, size = small
    loc = m.read_local(dist_sq=False, coc=False)
    rng = np.random.default_rng(64)
    cost, valid = m.costmat(np.zeros((0, 3), np.float32))
    assert cost.shape == (0, 0) and valid.shape == (0,)
    p = m.nf1_param(0.0)
    assert m._f["costmat_compute"](m._h, None, 0, C.byref(p), None, None) == 0
    assert m._f["costmat_compute_dev"](m._h, None, 0, C.byref(p), None, None) == 0
    pts = _free_points(m, loc, rng, 64)
    cost, valid = _check(m, loc, pts[:1])
    assert cost.tolist() == [[0]] and valid.tolist() == [True]
    cost, valid = _check(m, loc, pts)                            # every bit of the masks in use
    assert valid.all() and (cost >= 0).all() and cost[63].max() > 0 and cost[:, 63].max() > 0
    out = np.full((65, 65), 7, np.int32)
    val = np.full(65, 7, np.uint8)
    xyz = np.concatenate([pts, pts[:1]])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
    assert m._f["costmat_compute"](m._h, ptr(xyz), 65, C.byref(p), ptr(out), ptr(val)) == 1
    assert m._f["costmat_compute_dev"](m._h, ptr(xyz), 65, C.byref(p), ptr(out), ptr(val)) == 1
    assert (out == 7).all() and (val == 7).all()                 # refused: nothing written


# ---- 3. serpentine maze -----------------------------------------------------------------------------------------------------------
def test_serpentine_maze_thousands_of_levels():
    """one corridor of more than 2000 steps across the 64-voxel words in x and the 8-voxel tiles in y and z; a pocket walled off
    beside it.  Three point sets out of ONE reference: points close together in the middle (the propagation may leave early), the
    same with both ends (a far pair: every level runs), and with the pocket (the early exit never applies)."""
    inner, size, w = (70, 20, 12), (74, 20, 12), 0.125
    m = _mapper(size, voxel=w)
    try:
        pos, q = scenes.pose(0, w, delta_vox=0, yaw_deg=0.0)
        serp, cells = serpentine_labels(inner)
        lab = np.full((size[2], size[1], size[0]), 2, np.int8)
        lab[:, :, :inner[0]] = serp
        pocket = (72, 10, 5)
        lab[pocket[2], pocket[1], pocket[0]] = 1
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        mid = len(cells) // 2
        vox = np.array([tuple(cells[mid]), tuple(cells[mid + 40]), tuple(cells[mid + 300]), tuple(cells[0]), tuple(cells[-1]), pocket])
        pts = _world(m, vox)
        rc, rv = _reference(m, loc, pts)
        assert rv.all() and rc[3, 4] == len(cells) - 1 >= 2000 and rc[0, 2] == 300 and rc[0, 1] == 40
        assert (np.delete(rc[5], 5) == -1).all()
        for k in (3, 5, 6):
            _check(m, loc, pts[:k], ref=(rc[:k, :k], rv[:k]))
        cost, valid = m.costmat(pts, 0.1875)                      # 1.5 voxels: the corridor is too narrow, nobody is valid
        assert not valid.any() and (cost == -1).all()
    finally:
        m.close()


# ---- 5. stale scratch -------------------------------------------------------------------------------------------------------------
def test_second_call_sees_nothing_of_the_first(small):
    m, size = small
    rng = np.random.default_rng(11)
    loc = m.read_local(dist_sq=False, coc=False)
    many = _free_points(m, loc, rng, 64)
    _check(m, loc, many)
    few = _free_points(m, loc, rng, 3)
    cost, valid = _check(m, loc, few)
    assert valid.all() and (cost >= 0).all()
    m2 = _mapper(size)                                           # (a mapper of its own: `small` stays at its pose for the other tests)
    try:
        pivots = []
        for k in (0, 3):
            pos, q = scenes.pose(k, W, delta_vox=3, yaw_deg=0.0)
            _update(m2, pos, q, np.roll(_small_scene(size, seed=2), k, axis=2))
            pivots.append(m2.pivot())
            loc2 = m2.read_local(dist_sq=False, coc=False)
            _check(m2, loc2, _free_points(m2, loc2, rng, 64 if k == 0 else 5))
        assert pivots[0] != pivots[1]
    finally:
        m2.close()


# ---- 6. the _dev form -------------------------------------------------------------------------------------------------------------
def test_dev_form_fed_by_the_frontier_goals():
    import torch
    size, cap = (72, 64, 24), 40
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        lab = _small_scene(size, seed=3)
        lab[:, :, :6] = 0                                        # never seen: a slab, and pockets far from each other
        for x0, y0, z0 in ((20, 10, 8), (40, 40, 10), (55, 15, 12), (30, 50, 6), (60, 50, 14)):
            lab[z0:z0 + 4, y0:y0 + 4, x0:x0 + 4] = 0
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        robot = _free_points(m, loc, np.random.default_rng(3), 1, 0.1)
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            buf = torch.zeros((cap + 1, 3), dtype=torch.float32, device=dev)
            buf[0] = torch.from_numpy(robot[0]).to(dev)
            dcost = torch.full((cap + 1, cap + 1), 7, dtype=torch.int32, device=dev)
            dval = torch.full((cap + 1,), 7, dtype=torch.uint8, device=dev)
            m.frontier_compute_dev(0.1, 2, 26, cap)
            m.read_frontier_clusters_dev(0, buf[1:].data_ptr(), 0)
            m.costmat_dev(buf.data_ptr(), cap + 1, dcost.data_ptr(), dval.data_ptr(), 0.1, False)
        m.sync()
        pts = buf.cpu().numpy()
        nan = np.isnan(pts).any(axis=1)
        assert 2 <= (~nan[1:]).sum() < cap and nan[-1] and not nan[0]     # clusters, and a NaN tail
        hc, hv = _check(m, loc, pts, 0.1, False)                  # the host form on the same points, and the reference
        assert np.array_equal(dcost.cpu().numpy(), hc) and np.array_equal(dval.cpu().numpy().astype(bool), hv)
        assert set(np.unique(dval.cpu().numpy())) <= {0, 1}
        assert hv[0] and (hv[1:] == ~nan[1:]).all() and (hc[0, 1:][hv[1:]] > 0).any()
    finally:
        m.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    size = (32, 32, 16)
    m, t = _mapper(size), _mapper(size)
    try:
        f, h = m._f, m._h
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        _update(m, pos, q, np.ones((size[2], size[1], size[0]), np.int8))
        xyz = _world(m, [[3, 3, 3], [9, 3, 3]])
        cost = np.full((2, 2), 7, np.int32)
        val = np.full(2, 7, np.uint8)
        p = m.nf1_param(0.0)
        for fn in ("costmat_compute", "costmat_compute_dev"):
            assert f[fn](h, ptr(xyz), 2, None, ptr(cost), ptr(val)) == 1
            for bad in (-1.0, float("nan"), float("inf"), -1e-4):
                b = m.nf1_param(0.0)
                b.clearance = bad
                assert f[fn](h, ptr(xyz), 2, C.byref(b), ptr(cost), ptr(val)) == 1
            for flags in (nf1_ref.FROM_FRONTIERS, nf1_ref.FROM_FRONTIERS | nf1_ref.UNKNOWN_TRAVERSABLE, 4):
                b = m.nf1_param(0.0)
                b.flags = flags
                assert f[fn](h, ptr(xyz), 2, C.byref(b), ptr(cost), ptr(val)) == 1
            assert f[fn](h, ptr(xyz), -1, C.byref(p), ptr(cost), ptr(val)) == 1
            assert f[fn](h, ptr(xyz), 2, C.byref(p), None, ptr(val)) == 1
            assert f[fn](h, None, 2, C.byref(p), ptr(cost), ptr(val)) == 1
            assert f[fn](None, ptr(xyz), 2, C.byref(p), ptr(cost), ptr(val)) == 1
        assert f["costmat_compute"](h, None, 0, None, None, None) == 1
        t.set_tile((8, 0, 0), (64, 32, 16))
        for fn in ("costmat_compute", "costmat_compute_dev"):
            assert f[fn](t._h, ptr(xyz), 2, C.byref(p), ptr(cost), ptr(val)) == 1
            assert f[fn](t._h, None, 0, C.byref(p), None, None) == 1
        assert (cost == 7).all() and (val == 7).all()            # nothing refused has written anything
        assert f["costmat_compute"](h, ptr(xyz), 2, C.byref(p), ptr(cost), None) == 0      # valid may be NULL
        assert cost.tolist() == [[0, 6], [6, 0]]
    finally:
        m.close()
        t.close()


# ---- 8. the map update is untouched -----------------------------------------------------------------------------------------------
def test_costmat_calls_change_nothing_of_the_map_update():
    size = (80, 64, 64)
    rng0 = np.random.default_rng(5)
    boxes = [(lo, lo + rng0.integers(6, 26, size=3)) for lo in rng0.integers(-60, 60, size=(24, 3))]

    def pose(k):
        return scenes.pose(k, W, delta_vox=3, yaw_deg=0.0)

    def frame(k):
        pos, q = pose(k)
        return pos, q, box_labels(scenes.local_pivot(pos, W, size), size, k, boxes, unknown_slab=4)

    def points(k):
        return (np.array([pose(k)[0]], np.float32) + np.random.default_rng(k).uniform(-3.0, 3.0, (16, 3)).astype(np.float32)).astype(np.float32)

    def calls(a, k, phase, pos):
        if phase == "labels":
            a.costmat(points(k), 0.1, k % 2 == 0)
        elif phase == "fuse":
            a.costmat(points(k)[:3], 0.0)
        elif phase == "edt":
            a.costmat(points(k), 0.0, True)

    def after(k, a, la):
        _check(a, la, points(k), 0.1, k % 2 == 1)                 # and the matrix of the finished update is exact
    stage_calls_change_nothing(size, (frame(k) for k in range(8)), _mapper, calls, after=after)

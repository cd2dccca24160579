"""Line of sight on the device (include/gie.h gie_los_prepare* / gie_read_los_opaque* / gie_los_segments* / gie_view_gain*) against
the numpy statement of tests/los_ref.py.  The reference works on read_local's type and edt taken at the same point of the mapper's
stream; every comparison is bit for bit and leaves no voxel, segment or view out."""
import ctypes as C

import numpy as np
import pytest

import gie
import los_ref as lr
from gie import scenes
from stage_common import W, BoxDrive as _BoxDrive, bits as _bits, cv as _cv, mapper as _mapper, scene as _scene
from stage_common import stage_calls_change_nothing, update as _update, world as _world

pytestmark = pytest.mark.gpu

OPAQUE_SIZES = [(96, 80, 72), (97, 61, 45), (77, 53, 1), (48, 40, 33), (65, 20, 20), (1, 40, 40)]
BOX_SIZES = OPAQUE_SIZES[:4]


# ---- the opaque plane
@pytest.mark.parametrize("size", OPAQUE_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_opaque_plane_and_count(size):
    m = _mapper(size)
    try:
        loc, _, _ = _scene(m, size)
        seen = {}
        for cl in (0.0, 0.15, 0.3):
            for fl in (0, gie.LOS_UNKNOWN_OPAQUE):
                n = m.los_prepare(cl, fl)
                got = m.read_los_opaque()
                ref = lr.opaque(loc["type"], loc["edt"], _cv(m, cl), fl)
                assert got.dtype == np.uint8 and np.array_equal(got, ref.astype(np.uint8)), (cl, fl, int((got != ref).sum()))
                assert n == int(ref.sum())
                seen[cl, fl] = n
        # the clearances give different planes, none empty or full; the flag adds the never-seen voxels that are not opaque anyway
        assert 0 < seen[0.0, 0] < seen[0.15, 0] < seen[0.3, 0] < m.n and seen[0.0, 0] < seen[0.0, 1] < m.n, seen
        assert all(seen[cl, 1] >= seen[cl, 0] for cl in (0.15, 0.3)), seen
    finally:
        m.close()


# ---- segments
def _segment_cases(rng, size, opq, n=20000):
    """local coordinates (float, voxel units) of n segments: random pairs over the volume +- 2 voxels, then the special ones"""
    S = np.array(size, np.float64)
    lo, hi = np.where(S > 1, -2.0, -0.7), np.where(S > 1, S + 1, 0.7)    # (a flat axis: a fifth outside, not three quarters)
    a = rng.uniform(lo, hi, (n, 3))
    b = rng.uniform(lo, hi, (n, 3))
    short = slice(0, n // 4)                                  # a quarter of them short: most of those are clear
    b[short] = a[short] + rng.uniform(-12, 12, (n // 4, 3)) * (S > 1)
    vox = lambda k: rng.integers(0, size, (k, 3)).astype(np.float64)      # noqa: E731
    k = n // 2
    a[k:k + 500] = b[k:k + 500] = vox(500)                    # a == b
    k += 500
    a[k:k + 1500] = vox(1500)                                 # axis-aligned, between voxel centres
    b[k:k + 1500] = a[k:k + 1500]
    ax = rng.integers(0, 3, 1500)
    b[np.arange(k, k + 1500), ax] = rng.integers(0, np.array(size)[ax])
    k += 1500
    a[k:k + 1500] = vox(1500)                                 # exact diagonals in a plane or in space, clipped by the volume
    sg = rng.integers(-1, 2, (1500, 3))
    room = np.where(sg > 0, S - 1 - a[k:k + 1500], np.where(sg < 0, a[k:k + 1500], 1e9)).min(axis=1)
    b[k:k + 1500] = a[k:k + 1500] + sg * np.minimum(room, rng.integers(1, 40, 1500))[:, None]
    k += 1500
    oz, oy, ox = np.nonzero(opq)
    pick = rng.integers(0, len(ox), 1000)
    a[k:k + 500] = np.stack([ox, oy, oz], 1)[pick[:500]]      # opaque at the first voxel ...
    k += 500
    b[k:k + 500] = np.stack([ox, oy, oz], 1)[pick[500:]]      # ... and (for the short ones among them) at the last only
    a[k:k + 500] = b[k:k + 500] + rng.integers(-3, 4, (500, 3))
    k += 500
    a[k:k + 100, rng.integers(0, 3, 100)] = np.nan            # not finite
    b[k + 100:k + 200, 0] = np.inf
    return a, b


def _check_segments(m, loc, opq, a, b, pvt=None):
    a, b = _world(m, np.float32(a), pvt=pvt), _world(m, np.float32(b), pvt=pvt)      # (fractional voxels: to float32 before the pivot is added)
    got = m.los_segments(a, b)
    ref = lr.segments(loc["edt"], opq, a, b, m.cfg.voxel_width, m.pivot() if pvt is None else pvt)
    assert got.dtype == lr.HIT_DTYPE
    for k in got.dtype.names:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (k, int((got[k] != ref[k]).sum()))
    assert got.tobytes() == ref.tobytes()
    return ref


@pytest.mark.parametrize("size", BOX_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_segments(size):
    m = _mapper(size)
    try:
        loc, _, _ = _scene(m, size)
        for cl, fl, seed in ((0.0, 0, 1), (0.15, gie.LOS_UNKNOWN_OPAQUE, 2)):
            m.los_prepare(cl, fl)
            opq = lr.opaque(loc["type"], loc["edt"], _cv(m, cl), fl)
            a, b = _segment_cases(np.random.default_rng(seed), size, opq)
            ref = _check_segments(m, loc, opq, a, b)
            f, ln = ref["first"], ref["len"]
            assert (f == -2).sum() >= 200 and (f == -1).sum() >= 1000 and (f == 0).sum() >= 500 and (f > 0).sum() >= 1000
            assert ((f == ln - 1) & (ln > 1)).sum() >= 10 and ((ln == 1) & (f != -2)).sum() >= 500
            moved = np.abs(ref["hit"][f != -2] - m.pivot()).max()
            assert moved < max(size)
        assert m.los_segments(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    finally:
        m.close()


@pytest.mark.parametrize("size", [(1024, 16, 12), (16, 1024, 12), (12, 16, 1024)], ids=lambda v: "x".join(map(str, v)))
def test_long_lines(size):
    """segments from end to end of a volume 1024 voxels long, each with one opaque voxel of its own placed at a chosen index"""
    m = _mapper(size)
    try:
        ax = int(np.argmax(size))
        o1, o2 = [k for k in range(3) if k != ax]
        rng = np.random.default_rng(ax)
        want = [0, 1, 63, 64, 65, 511, 512, 1000, -2, -1, None, None]
        a = np.zeros((len(want), 3), np.int64)
        b = np.zeros((len(want), 3), np.int64)
        b[:, ax] = size[ax] - 1
        for arr in (a, b):
            arr[:, o1] = rng.integers(0, size[o1], len(want))
            arr[:, o2] = rng.integers(0, size[o2], len(want))
        a[1::2], b[1::2] = b[1::2].copy(), a[1::2].copy()      # every other one runs backwards
        lab = np.ones(size[::-1], np.int8)
        for i, k in enumerate(want):
            if k is not None:
                x, y, z = lr.line(a[i], b[i])[k]
                lab[z, y, x] = 2
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        assert np.array_equal(loc["type"] == lr.OCCUPIED, lab == 2)
        assert m.los_prepare(0.0, 0) == int((lab == 2).sum()) >= len(want) - 4
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        ra = np.concatenate([a, rng.integers(0, size, (2000, 3))])
        rb = np.concatenate([b, rng.integers(0, size, (2000, 3))])
        ref = _check_segments(m, loc, opq, ra, rb)
        f, ln = ref["first"][:len(want)], ref["len"][:len(want)]
        assert (ln >= size[ax]).all() and f[0] == 0 and f[1] <= 1 and (f[:-2] >= 0).all()
        assert f.max() >= 1000 and (f == ln - 1).any()        # (another segment's voxel can only make a hit earlier)
        m.los_prepare(0.2, 0)                                 # two voxels of clearance: the hits come earlier, min_edt is below 2
        opq2 = lr.opaque(loc["type"], loc["edt"], _cv(m, 0.2), 0)
        ref2 = _check_segments(m, loc, opq2, ra, rb)
        assert (ref2["first"][2:len(want) - 2] < f[2:-2]).all()
    finally:
        m.close()


def _beyond_scene(size):
    """free labels and four lines along the longest axis, far apart in the cross-section (straight end to end; oblique end to end
    forwards and backwards; oblique between inner points).  The opaque voxels come from a clearance of 1.2 voxels: an occupied
    voxel one voxel BESIDE the line gives the line's voxel next to it edt 1 (opaque) and its neighbours on the line sqrt(2) (not).
    On each line: such a voxel at index i; before i an occupied voxel two voxels beside the line (edt 2: a dip above the
    clearance); beyond i a second opaque voxel of the same kind at j, and an occupied voxel ON the line at c (edt 0: lower than
    anything up to i, and opaque as well), once between i and j and once right behind i.
    Returns (labels, a [4, 3], b [4, 3], i [4], j [4], c [4]) in local voxels."""
    ax = int(np.argmax(size))
    o1, o2 = [k for k in range(3) if k != ax]
    n, s1, s2 = size[ax], size[o1], size[o2]
    if s2 >= 10:
        anchors = [(2, 2), (s1 - 3, 2), (2, s2 - 3), (s1 - 3, s2 - 3)]
    else:                                                      # a thin cross-section: four lines side by side
        anchors = [(3 + k * ((s1 - 7) // 3), s2 // 2) for k in range(4)]
    a = np.zeros((4, 3), np.int64)
    b = np.zeros((4, 3), np.int64)
    side = []
    for k, (p1, p2) in enumerate(anchors):
        d1 = (2 if p1 < s1 / 2 else -2) if k else 0            # the drift of the oblique ones, towards the middle
        d2 = (1 if p2 < s2 / 2 else -1) if k else 0
        lo, hi = (n // 8, n - 1 - n // 8) if k == 3 else (0, n - 1)
        a[k, ax], a[k, o1], a[k, o2] = lo, p1, p2
        b[k, ax], b[k, o1], b[k, o2] = hi, p1 + d1, p2 + d2
        side.append(-1 if p1 < s1 / 2 else 1)                  # beside the line: away from the middle along o1
    a[2], b[2] = b[2].copy(), a[2].copy()
    lab = np.ones(size[::-1], np.int8)
    lines = [lr.line(a[k], b[k]) for k in range(4)]
    on_a_line = {v for ln in lines for v in ln}

    def beside(ln, t, dist, sd):
        """an occupied voxel `dist` beside the line's voxel t, or the next one where the line keeps its place in the cross-section
        over five voxels (beside a side step of an oblique line stands the line itself): the index used"""
        while True:
            v = list(ln[t])
            v[o1] += sd * dist
            if tuple(v) not in on_a_line and all(ln[t + e][o1] == ln[t][o1] and ln[t + e][o2] == ln[t][o2] for e in (-2, -1, 1, 2)):
                lab[v[2], v[1], v[0]] = 2
                return t
            t += 1

    first, second, lower = [], [], []
    for k, ln in enumerate(lines):
        i = beside(ln, (63, 2 * len(ln) // 5, 511 if n > 600 else 129, len(ln) // 3)[k], 1, side[k])
        beside(ln, i // 2, 2, side[k])
        j = beside(ln, (i + 8, 4 * len(ln) // 5, len(ln) - 4, i + 70)[k], 1, side[k])
        c = (i + 4, j + (len(ln) - j) // 2, i + 1, len(ln) - 1)[k]
        lab[ln[c][2], ln[c][1], ln[c][0]] = 2
        first.append(i)
        second.append(j)
        lower.append(c)
    return lab, a, b, np.array(first), np.array(second), np.array(lower)


BEYOND_CLEARANCE = 0.12                                        # metres at w = 0.1: 1.2 voxels, between 1 and sqrt(2)


@pytest.mark.parametrize("size", [(1024, 16, 12), (16, 1024, 12), (12, 16, 1024), (300, 40, 7)], ids=lambda v: "x".join(map(str, v)))
def test_segments_beyond_the_first_hit(size):
    """after its first hit the kernel walks on without loads, for len: a second opaque voxel and a voxel of lower edt beyond the
    hit must change nothing — first and hit stay the first opaque voxel, min_edt is the minimum over indices 0 .. first only.
    (An opaque voxel has the smallest edt seen so far whatever made it opaque — occupied and never-seen voxels have edt 0, a
    clearance is a bound on edt — so the minimum up to i is at i itself; what can be asked is that it is not the line's.)"""
    m = _mapper(size)
    try:
        lab, a, b, want, second, lower = _beyond_scene(size)
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        pvt = np.array(m.pivot())
        assert np.array_equal(loc["type"] == lr.OCCUPIED, lab == 2)
        m.los_prepare(BEYOND_CLEARANCE, 0)
        opq = lr.opaque(loc["type"], loc["edt"], _cv(m, BEYOND_CLEARANCE), 0)
        ref = _check_segments(m, loc, opq, a, b)               # every field, bit for bit
        got = m.los_segments(_world(m, a), _world(m, b))
        for k in range(len(a)):
            ln = lr.line(a[k], b[k])
            e = np.array([loc["edt"][v[2], v[1], v[0]] for v in ln], np.float32)
            o = np.array([opq[v[2], v[1], v[0]] for v in ln])
            i, j, c = int(want[k]), int(second[k]), int(lower[k])
            assert not o[:i].any() and o[i] and o[j] and o[c] and i < j and i < c and o[i + 1:].sum() >= 2
            # the case proves something: a dip before i that is not the hit, and the line goes strictly lower beyond i
            assert e[i] == 1.0 and e[:i - 2].min() == 2.0 and e[i + 1:].min() == 0.0 < e[:i + 1].min(), (k, e[:i].min(), e[i], e[i + 1:].min())
            for r in (ref[k], got[k]):
                assert r["first"] == i and r["len"] == len(ln) and r["hit"].tolist() == (np.array(ln[i]) + pvt).tolist()
                assert _bits(r["min_edt"]).tobytes() == _bits(e[:i + 1].min()).tobytes()
    finally:
        m.close()


# ---- view gain
def _view_set(m, rng, size, loc, corner, pocket, reps):
    """local voxels of the views: random ones, the cluster representatives, one inside an obstacle, the closed room's corner (the
    last but two), and two outside the volume (the last two)"""
    occ = np.argwhere(loc["type"] == lr.OCCUPIED)[:, ::-1]
    v = [rng.integers(0, size, (6, 3)), np.asarray(reps).reshape(-1, 3)[:12], occ[rng.integers(0, len(occ), 1)]]
    v.append(np.array([corner if corner is not None else (0, 0, 0)]))
    v.append(np.array([(-1, 3, 0), (size[0] + 2, 0, 0)]))
    return np.concatenate(v).astype(np.float64)


@pytest.mark.parametrize("size", BOX_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_view_gain(size):
    import torch
    m = _mapper(size)
    try:
        loc, corner, pocket = _scene(m, size)
        pvt = np.array(m.pivot())
        nc, _ = m.frontier_compute(0.0, 3, 26, 12)
        rec, goal, _ = m.read_frontier_clusters()
        assert nc >= 2
        m.los_prepare(0.0, 0)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        rng = np.random.default_rng(sum(size))
        vox = _view_set(m, rng, size, loc, corner, pocket, rec["rep"] - pvt)
        assert 8 <= len(vox) <= 32
        frustum = gie.view_frustum(0.6, 0.2, 1.6, 1.1)
        ncand = nvis = 0
        for rmin, rmax, tan2, normals in ((0.0, 1.6, -1.0, None), (0.0, 2.0, 0.09, None), (0.0, 1.8, -1.0, frustum), (0.65, 1.2, -1.0, None),
                                          (0.0, 1.45, 0.5, [(0, 0, 1)])):
            views = gie.make_views(_world(m, vox), normals)
            got = m.view_gain(views, rmin, rmax, tan2)
            vis = []
            ref = lr.view_gain(loc["type"], opq, views, rmin, rmax, tan2, m.cfg.voxel_width, pvt, vis)
            assert got.dtype == lr.SCORE_DTYPE and got.tobytes() == ref.tobytes(), (rmin, rmax, tan2, got, ref)
            assert (got[-2:].view(np.int32) == -1).all() and (got[:-2]["candidates"] >= 0).all()
            ncand += int(ref["candidates"][:-2].sum())
            nvis += sum(vis)
        assert nvis >= ncand // 10 and ncand - nvis >= ncand // 10          # neither branch of the walk is idle
        # the closed room: from inside it, only its own never-seen pocket; voxels outside it score nothing
        if corner is not None:
            unk = loc["type"] == lr.UNKNOWN
            inroom = int(unk[pocket].sum())
            zz, yy, xx = np.ogrid[:size[2], :size[1], :size[0]]
            d2 = (xx - corner[0]) ** 2 + (yy - corner[1]) ** 2 + (zz - corner[2]) ** 2
            assert int((unk & (d2 <= 16 ** 2)).sum()) > inroom == unk[pocket].size
            sc = m.view_gain(gie.make_views(_world(m, [corner])), 0.0, 1.6)[0]
            assert 0 < sc["unknown"] <= inroom and sc["frontier"] > 0
        # the cluster representatives handed on as DEVICE buffers: frontier_compute -> goals -> views -> scores, no host in between
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        cap = 12
        with torch.cuda.stream(st):
            dg = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
            m.frontier_compute_dev(0.0, 3, 26, cap)
            m.read_frontier_clusters_dev(0, dg.data_ptr(), 0)
            dv = torch.zeros((cap, 16), dtype=torch.float32, device=dev)
            dv[:, :3] = dg
            ds = torch.full((cap, 4), -7, dtype=torch.int32, device=dev)
            m.view_gain_dev(dv.data_ptr(), cap, ds.data_ptr(), 0.0, 1.6)
        m.sync()
        ref = lr.view_gain(loc["type"], opq, gie.make_views(goal), 0.0, 1.6, -1.0, m.cfg.voxel_width, pvt)
        assert ds.cpu().numpy().tobytes() == ref.tobytes()
        assert (ref["candidates"][:min(nc, cap)] > 0).all() and (ref["candidates"][nc:] == -1).all()
    finally:
        m.close()


def test_view_gain_256_cubed_range_60():
    size, w = (256, 256, 256), 0.05
    m = _mapper(size, voxel=w, cutoff_dist=2.0)
    try:
        for k in range(2):
            pos, q = scenes.pose(k, w, delta_vox=8, yaw_deg=2.0)
            pvt = scenes.local_pivot(pos, w, size)
            _update(m, pos, q, scenes.hash_world_labels(pvt, size, k).astype(np.int8))
        loc = m.read_local(dist_sq=False, coc=False)
        m.los_prepare(0.0, 0)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        free = np.argwhere(loc["type"] == lr.FREE)[:, ::-1]
        vox = np.concatenate([free[np.random.default_rng(1).integers(0, len(free), 3)], [[128, 128, 128]]])
        views = gie.make_views(_world(m, vox))
        got = m.view_gain(views, 0.0, 60 * w)
        ref = lr.view_gain(loc["type"], opq, views, 0.0, 60 * w, -1.0, w, m.pivot())
        assert got.tobytes() == ref.tobytes(), (got, ref)
        assert (ref["candidates"] > 300000).all() and (ref["occupied"] > 0).all()
    finally:
        m.close()


# ---- life cycle
def _whole_feature(m, rng, size, cl, fl, loc=None, check=True):
    """prepare + the three readers on the current map; with check, against the reference.  Returns what the device gave."""
    if loc is None and check:
        loc = m.read_local(dist_sq=False, coc=False)
    pvt = m.pivot()
    n = m.los_prepare(cl, fl)
    plane = m.read_los_opaque()
    a, b = np.float32(rng.uniform(-1, np.array(size), (2000, 3))), np.float32(rng.uniform(-1, np.array(size), (2000, 3)))
    views = gie.make_views(_world(m, rng.integers(0, size, (8, 3))))
    seg = m.los_segments(_world(m, a), _world(m, b))
    sc = m.view_gain(views, 0.0, 1.2, 0.7)
    if check:
        opq = lr.opaque(loc["type"], loc["edt"], _cv(m, cl), fl)
        assert np.array_equal(plane, opq.astype(np.uint8)) and n == int(opq.sum())
        assert seg.tobytes() == lr.segments(loc["edt"], opq, _world(m, a), _world(m, b), m.cfg.voxel_width, pvt).tobytes()
        assert sc.tobytes() == lr.view_gain(loc["type"], opq, views, 0.0, 1.2, 0.7, m.cfg.voxel_width, pvt).tobytes()
    return dict(n=n, plane=plane, seg=seg, sc=sc, a=_world(m, a), b=_world(m, b), views=views)


def test_result_stays_with_its_prepare_through_a_drive():
    size = (80, 72, 64)
    d = _BoxDrive(size, seed=4)
    m = _mapper(size)
    try:
        pos, q, lab = d.frame(0)
        _update(m, pos, q, lab)
        first = _whole_feature(m, np.random.default_rng(0), size, 0.15, 0)
        pv = m.pivot()
        for k in range(1, 13):                                # the map moves and changes; the result stays
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
            if k % 4 == 0 or k == 12:
                assert np.array_equal(m.read_los_opaque(), first["plane"])
                assert m.los_segments(first["a"], first["b"]).tobytes() == first["seg"].tobytes()
                assert m.view_gain(first["views"], 0.0, 1.2, 0.7).tobytes() == first["sc"].tobytes()
        assert m.pivot() != pv
        second = _whole_feature(m, np.random.default_rng(1), size, 0.0, gie.LOS_UNKNOWN_OPAQUE)     # a second prepare replaces it
        assert second["n"] != first["n"] and not np.array_equal(second["plane"], first["plane"])
    finally:
        m.close()


def test_refusals():
    size = (32, 32, 16)
    m, t = _mapper(size), _mapper(size)
    try:
        f, h = m._f, m._h
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
        plane = np.zeros(m.n, np.uint8)
        xyz = np.zeros((4, 3), np.float32)
        hits = np.zeros(4, lr.HIT_DTYPE)
        views = gie.make_views(xyz)
        score = np.zeros(4, lr.SCORE_DTYPE)
        vp = m.view_param(0.0, 1.0)
        n = C.c_int32(0)

        def readers(hh):
            return [f["read_los_opaque"](hh, ptr(plane)), f["read_los_opaque_dev"](hh, ptr(plane)),
                    f["los_segments"](hh, ptr(xyz), ptr(xyz), 4, ptr(hits)), f["los_segments_dev"](hh, ptr(xyz), ptr(xyz), 4, ptr(hits)),
                    f["view_gain"](hh, ptr(views), 4, C.byref(vp), ptr(score)), f["view_gain_dev"](hh, ptr(views), 4, C.byref(vp), ptr(score))]
        assert readers(h) == [1] * 6                                      # before the first prepare
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        for mm in (m, t):
            _update(mm, pos, q, np.ones((size[2], size[1], size[0]), np.int8))
        good = m.los_param(0.0, 0)
        for cl, fl in ((-1.0, 0), (-1e-4, 0), (float("nan"), 0), (float("inf"), 0), (0.0, 2), (0.0, 5)):
            p = m.los_param(0.0, fl)
            p.clearance = cl
            assert f["los_prepare"](h, C.byref(p), C.byref(n)) == 1
            assert f["los_prepare_dev"](h, C.byref(p), None) == 1
        assert f["los_prepare"](h, None, None) == 1 and f["los_prepare_dev"](h, None, None) == 1
        assert f["los_prepare"](None, C.byref(good), None) == 1
        assert readers(h) == [1] * 6                                      # (nothing refused has made a plane)
        assert f["los_prepare"](h, C.byref(good), None) == 0              # the count may be NULL
        assert f["los_prepare"](h, C.byref(good), C.byref(n)) == 0 and n.value == 0
        assert f["read_los_opaque"](h, ptr(plane)) == 0 and f["los_segments"](h, ptr(xyz), ptr(xyz), 4, ptr(hits)) == 0
        assert f["view_gain"](h, ptr(views), 4, C.byref(vp), ptr(score)) == 0
        # NULL buffers, NULL param, n < 0; n == 0 is valid
        assert f["read_los_opaque"](h, None) == 1 and f["read_los_opaque_dev"](h, None) == 1
        assert f["los_segments"](h, None, ptr(xyz), 4, ptr(hits)) == 1 and f["los_segments_dev"](h, ptr(xyz), ptr(xyz), 4, None) == 1
        assert f["los_segments"](h, ptr(xyz), ptr(xyz), -1, ptr(hits)) == 1
        assert f["view_gain"](h, ptr(views), 4, None, ptr(score)) == 1 and f["view_gain_dev"](h, ptr(views), 4, None, ptr(score)) == 1
        assert f["view_gain"](h, None, 4, C.byref(vp), ptr(score)) == 1 and f["view_gain"](h, ptr(views), -1, C.byref(vp), ptr(score)) == 1
        assert f["los_segments"](h, None, None, 0, None) == 0 and f["view_gain"](h, None, 0, C.byref(vp), None) == 0
        assert f["los_segments_dev"](h, None, None, 0, None) == 0 and f["view_gain_dev"](h, None, 0, C.byref(vp), None) == 0
        # ranges and views
        for rmin, rmax, tan2 in ((1.0, 0.5, -1.0), (-0.1, 1.0, -1.0), (0.0, float("inf"), -1.0), (float("nan"), 1.0, -1.0), (0.0, 1.0, float("nan"))):
            bad = m.view_param(rmin, rmax, tan2)
            assert f["view_gain"](h, ptr(views), 4, C.byref(bad), ptr(score)) == 1
            assert f["view_gain_dev"](h, ptr(views), 4, C.byref(bad), ptr(score)) == 1
        five = views.copy()
        five["n_planes"][2] = 5
        far = gie.make_views(xyz, [(1, 0, 0), (0, 40000, 0)])
        neg = views.copy()
        neg["n_planes"][0] = -1
        for bad in (five, far, neg):
            assert f["view_gain"](h, ptr(bad), 4, C.byref(vp), ptr(score)) == 1
        ok = gie.make_views(xyz, [(32767, -32767, 0), (0, 0, 1)])
        ok["normal"][:, 2] = 40000                                        # (beyond n_planes: not looked at)
        assert f["view_gain"](h, ptr(ok), 4, C.byref(vp), ptr(score)) == 0
        # a tiled mapper
        t.set_tile((8, 0, 0), (64, 32, 16))
        th = t._h
        assert f["los_prepare"](th, C.byref(good), None) == 1 and f["los_prepare_dev"](th, C.byref(good), None) == 1
        assert readers(th) == [1] * 6
    finally:
        m.close()
        t.close()


def test_dev_forms_through_torch():
    import torch
    size = (72, 64, 48)
    m = _mapper(size)
    try:
        loc, _, _ = _scene(m, size)
        host = _whole_feature(m, np.random.default_rng(3), size, 0.15, gie.LOS_UNKNOWN_OPAQUE, loc=loc)
        bad = host["views"].copy()
        bad["n_planes"][1] = 7                                            # the _dev form cannot refuse it: the view scores -1
        m.los_prepare(0.0, 0)                                             # another plane in between
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        ns = len(host["a"])
        with torch.cuda.stream(st):
            dn = torch.full((1,), -7, dtype=torch.int32, device=dev)
            m.los_prepare_dev(0.15, gie.LOS_UNKNOWN_OPAQUE, dn.data_ptr())
            dp = torch.empty(size[::-1], dtype=torch.uint8, device=dev)
            m.read_los_opaque_dev(dp.data_ptr())
            da, db = torch.from_numpy(host["a"]).to(dev), torch.from_numpy(host["b"]).to(dev)
            dh = torch.zeros(ns * 24, dtype=torch.uint8, device=dev)
            m.los_segments_dev(da.data_ptr(), db.data_ptr(), ns, dh.data_ptr())
            dv = torch.from_numpy(np.concatenate([host["views"], bad]).view(np.uint8)).to(dev)
            ds = torch.zeros(16 * 16, dtype=torch.uint8, device=dev)
            m.view_gain_dev(dv.data_ptr(), 16, ds.data_ptr(), 0.0, 1.2, 0.7)
        m.sync()
        assert int(dn.cpu().item()) == host["n"] and np.array_equal(dp.cpu().numpy(), host["plane"])
        assert dh.cpu().numpy().tobytes() == host["seg"].tobytes()
        sc = ds.cpu().numpy().view(lr.SCORE_DTYPE)
        want = host["sc"].copy()
        assert sc[:8].tobytes() == want.tobytes()
        want[1] = (-1, -1, -1, -1)
        assert sc[8:].tobytes() == want.tobytes()
        m.profile_enable(True)
        m.los_prepare(0.0, 0)
        m.los_segments(host["a"][:10], host["b"][:10])
        m.view_gain(host["views"][:2], 0.0, 0.5)
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["los"][1] == 1 and prof["los_query"][1] == 2 and prof["los"][0] > 0 and prof["los_query"][0] > 0
    finally:
        m.close()


def test_los_calls_change_nothing_of_the_map_update():
    size = (80, 64, 64)
    d = _BoxDrive(size, seed=5)
    rngs = {}

    def calls(a, k, phase, pos):
        rng = rngs.setdefault(k, np.random.default_rng(k))       # one generator per frame, through its four phases
        if phase == "labels":
            _whole_feature(a, rng, size, 0.1, 0, check=False)
        elif phase == "fuse":
            _whole_feature(a, rng, size, 0.0, gie.LOS_UNKNOWN_OPAQUE, check=False)
        elif phase == "edt":
            a.read_los_opaque()
            a.view_gain(gie.make_views(_world(a, [(40, 32, 32)])), 0.0, 2.0)
        else:
            _whole_feature(a, rng, size, 0.2, 0, check=(k % 4 == 3))
    stage_calls_change_nothing(size, (d.frame(k) for k in range(12)), _mapper, calls)

"""The ground pose navigation function on the device (include/gie.h "ground pose navigation function") against
tests/ground_pose_nf1_ref.py on the same mapper's planes (read_ground()), byte for byte: box scenes at the word boundaries, the three
fixed scenes, both forms of the propagation at their threshold, the parent's footprint call as a second witness, the chain from the
ground frontier clusters, lifetime, refusals, the map update's invariant, the profile and the launches."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ground_nf1_ref as N
import ground_pose_nf1_ref as Q
import ground_ref as R
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, xy as _xy, ground
from stage_common import W, box_labels, mapper as _mapper, stage_calls_change_nothing, update as _update

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries of a mapper without frontier clusters: the parent's
FEET = [(0, 0, 0), (64, 4, 9), (9, 9, 1), (Q.MAX_SQ, 4, 1)]     # (front_sq, back_sq, side_sq); the last at the cap: 64 cells ahead
FP = (64, 4, 9)


def _ground(m, size):
    """the ground field of the inner layers: the volume's top and bottom layers are frontier voxels everywhere, a band that holds them
    has no FREE column"""
    skip = 2 if size[2] >= 8 else 1
    return ground(m, size, (skip, size[2] - 1 - skip))


def _labels(size, plane):
    """labels [Z][Y][X] of a cell plane [Y][X] of 0 unknown / 1 free / 2 occupied: every column the same over the whole height"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(plane, np.int8)[None], (size[2], size[1], size[0])))


def _box_plane(size, seed, n_boxes=9, unknown_slab=3):
    """random boxes, an unknown x-slab (FNT cells beside it) and a pocket: a corridor 7 cells wide, closed at its -x end"""
    X, Y, _ = size
    rng = np.random.default_rng(seed)
    t = np.ones((Y, X), np.int8)
    for _ in range(n_boxes):
        x, y = int(rng.integers(4, X - 2)), int(rng.integers(0, Y))
        t[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 5))] = 2
    y0, x0 = 2, X // 2 - 8
    t[y0:y0 + 9, x0:x0 + 18] = 1
    t[y0, x0:x0 + 18] = 2
    t[y0 + 8, x0:x0 + 18] = 2
    t[y0:y0 + 9, x0] = 2
    gx = _goal_x(X)
    t[Y - 7:Y - 3, gx - 2:gx + 3] = 1                           # room around the first goal
    t[:, :unknown_slab] = 0
    return t


def _goal_x(X):
    """the goals' column: beyond the last 64-column boundary where there is one, so that the long routes cross it"""
    return X - 5 if X - 5 >= 64 or X == 64 else 64


def _dev_forms(m, st, pvt, goals, gk, e, c, flags, want, starts, sk, max_len):
    """the host forms and the _dev forms over buffers one element longer with a poisoned tail: the reference's bytes, nothing beyond"""
    import torch
    nf, cb, counts = want
    u, fr, rv = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    assert m.ground_pose_nf1_compute(goals, gk, e[0], e[1], e[2], c, u, fr, rv) == counts, ("counts", e, c, flags)
    f, cs = m.read_ground_pose_nf1()
    assert np.array_equal(cs, cb), ("cspace", e, c, flags, np.argwhere(cs != cb)[:5].tolist())
    assert np.array_equal(f, nf), ("pnf1", e, c, flags, np.argwhere(f != nf)[:5].tolist())
    wq = Q.query(nf, starts, sk, pvt, W)
    wp, wl = Q.path(nf, starts, sk, pvt, W, max_len, rv, fill=0x5a5a5a5a)
    assert np.array_equal(m.ground_pose_nf1_query(starts, sk), wq)
    hp, hl = m.ground_pose_nf1_path(starts, sk, max_len, fill=0x5a5a5a5a)
    assert np.array_equal(hl, wl) and hp.tobytes() == wp.tobytes(), ("path", e, c, flags)
    dev = torch.device("cuda", 0)
    n, ns, cells = len(goals), len(starts), f[0].size
    with torch.cuda.stream(st):
        dg = torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
        dk = torch.from_numpy(np.asarray(gk, np.int32)).to(dev) if gk is not None else None
        dcnt = torch.full((3,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        m.ground_pose_nf1_compute_dev(dg.data_ptr() if n else 0, dk.data_ptr() if dk is not None and n else 0, n, dcnt.data_ptr(), e[0], e[1], e[2], c, u, fr, rv)
        df = torch.full((8 * cells + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        dc = torch.full((cells + 1,), 0x5a, dtype=torch.uint8, device=dev)
        m.read_ground_pose_nf1_dev(df.data_ptr(), dc.data_ptr())
        ds = torch.from_numpy(np.ascontiguousarray(starts)).to(dev)
        dsk = torch.from_numpy(np.asarray(sk, np.int32)).to(dev) if sk is not None else None
        dq = torch.full((ns + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        m.ground_pose_nf1_query_dev(ds.data_ptr(), dsk.data_ptr() if dsk is not None else 0, ns, dq.data_ptr())
        dp = torch.full((ns * max_len * 3 + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        dl = torch.full((ns + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        m.ground_pose_nf1_path_dev(ds.data_ptr(), dsk.data_ptr() if dsk is not None else 0, ns, max_len, dp.data_ptr(), dl.data_ptr())
    m.sync()
    assert dcnt.cpu().tolist() == counts + [0x5a5a5a5a]
    o = df.cpu().numpy()
    assert o[:-1].tobytes() == nf.tobytes() and o[-1] == 0x5a5a5a5a
    o = dc.cpu().numpy()
    assert o[:-1].tobytes() == cb.tobytes() and o[-1] == 0x5a
    assert dq.cpu().numpy().tolist() == wq.tolist() + [0x5a5a5a5a]
    assert dl.cpu().numpy().tolist() == wl.tolist() + [0x5a5a5a5a]
    o = dp.cpu().numpy()
    assert o[:-1].tobytes() == wp.tobytes() and o[-1] == 0x5a5a5a5a      # (wp is poisoned beyond min(len, max_len))
    return wl


def _starts(g, pvt, rng, n=40):
    Y, X = g["type"].shape
    cells = np.stack([rng.integers(-1, X + 1, n), rng.integers(-1, Y + 1, n)], 1)
    xy = np.concatenate([_xy(pvt, cells), [[np.nan, 0.0]]]).astype(np.float32)
    sk = np.array([(-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, -2)[i % 11] for i in range(n + 1)], np.int32)
    return xy, sk


# ---------------------------------------------------------------------------------------------------------- 1. box scenes
@pytest.mark.parametrize("si, size", list(enumerate([(64, 48, 8), (65, 40, 8), (70, 32, 8), (130, 24, 8)])))
def test_field_cspace_path_and_query_equal_the_reference(si, size):
    """every flag combination with every footprint and both clearances: 64 fields a scene"""
    import torch
    m = _mapper(size)
    try:
        pvt = _settle(m, _labels(size, _box_plane(size, 40 + si)))
        g = _ground(m, size)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        X, Y = size[0], size[1]
        gx = _goal_x(X)
        goals = np.concatenate([_xy(pvt, [(gx, Y - 5), (gx, Y // 2), (X + 2, 3), (X // 2, Y - 3)]), np.full((2, 2), np.nan, np.float32)]).astype(np.float32)
        gk = np.array([-1, 4, 0, 9, 0, -1], np.int32)
        starts, sk = _starts(g, pvt, np.random.default_rng(si))
        seen = {"free": False, "blocked": False, "k_not_k4": False, "reverse_only": False, "goal_src": False, "fnt_src": False, "crosses": False, "short": False}
        fields = {}
        for fl in range(8):
            for j, (e, c) in enumerate((e, c) for e in FEET for c in (0, 4)):
                use_gk = None if fl == 5 else gk                 # (NULL heading arrays in one combination each)
                want = Q.field(g, goals, use_gk, pvt, W, e[0], e[1], e[2], c, fl)
                wl = _dev_forms(m, st, pvt, goals, use_gk, e, c, fl, want, starts, None if fl == 6 else sk, 7 if j % 2 else 300)
                nf, cb, counts = want
                fields[(fl, j)] = nf
                cs = ((cb[None] >> np.arange(8, dtype=np.uint8)[:, None, None]) & 1).astype(bool)
                seen["free"] |= bool((~cs).any())
                seen["blocked"] |= bool(cs.any())
                seen["k_not_k4"] |= bool((~cs[:4] & cs[4:]).any())
                seen["short"] |= bool((wl > 7).any()) and j % 2 == 1
                if fl & 2:
                    fnt = np.asarray(g["type"]) == R.FNT
                    seen["fnt_src"] |= bool(((nf == 0) & fnt[None]).any())
                seen["goal_src"] |= bool((nf[:, Y - 5, gx] == 0).any())
                far = np.argwhere(nf == nf.max())[0]
                if nf.max() > 0:
                    p, ln = Q.path(nf, _xy(pvt, [(far[2], far[1])]), [int(far[0])], pvt, W, int(nf.max()) + 1, bool(fl & 4))
                    xs = p[0, :ln[0], 0] - pvt[0]
                    seen["crosses"] |= bool(((xs[:-1] // 64) != (xs[1:] // 64)).any())
        for fl in range(4):
            for j in range(8):
                a, b = fields[(fl, j)], fields[(fl | 4, j)]
                seen["reverse_only"] |= bool(((a < 0) & (b >= 0)).any())
        if X == 64:
            seen["crosses"] = True                              # (one word per row: there is no 64-column boundary to cross)
        ty = np.asarray(g["type"])
        assert all(seen.values()) and all((ty == v).sum() > 20 for v in (R.UNKNOWN, R.FREE, R.OCCUPIED, R.FNT)), (seen, np.unique(ty, return_counts=True))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. the fixed scenes
def _fixed(plane_fn, goal, checks, gnf1=()):
    t = plane_fn()
    plane = np.where(t == R.OCCUPIED, 2, 1).astype(np.int8)
    size = (t.shape[1], t.shape[0], 4)
    m = _mapper(size)
    try:
        pvt = _settle(m, _labels(size, plane))
        g = _ground(m, size)
        assert np.array_equal(np.asarray(g["type"]) == R.OCCUPIED, t == R.OCCUPIED) and not (np.asarray(g["type"]) == R.UNKNOWN).any()
        for rv in (False, True):
            counts = m.ground_pose_nf1_compute(_xy(pvt, [goal]), None, FP[0], FP[1], FP[2], 0, False, False, rv)
            f, cs = m.read_ground_pose_nf1()
            nf, cb, wc = Q.field(g, _xy(pvt, [goal]), None, pvt, W, FP[0], FP[1], FP[2], 0, 4 if rv else 0)
            assert counts == wc and np.array_equal(f, nf) and np.array_equal(cs, cb)
            checks(f, cs, rv)
        for clearance_sq, cell, val in gnf1:
            m.ground_nf1_compute(_xy(pvt, [goal]), clearance_sq)
            assert m.read_ground_nf1()[cell[1], cell[0]] == val
    finally:
        m.close()


def test_fixed_door():
    import test_ground_pose_nf1_reference as T

    def checks(f, cs, rv):
        assert f[:, 20, 12].tolist() == ([43, 44, 45, 44, 43, 44, 45, 44] if rv else [43, 44, 45, 46, 47, 46, 45, 44])
    _fixed(T.door, (55, 20), checks, [(73, (12, 20), -1), (9, (12, 20), 43)])


def test_fixed_pocket():
    import test_ground_pose_nf1_reference as T

    def checks(f, cs, rv):
        assert not (cs[14, 20] >> 4) & 1 and f[4, 14, 20] == (35 if rv else -1) and f[0, 14, 20] == 38 and (cs[14, 20] >> 2) & 1 and f[2, 14, 20] == -1
    _fixed(T.pocket, (55, 14), checks)


def test_fixed_l_turn():
    import test_ground_pose_nf1_reference as T

    def checks(f, cs, rv):
        assert f[:, 12, 12].tolist() == [-1] * 8
    _fixed(T.l_turn, (50, 37), checks, [(9, (12, 12), 63)])


# ---------------------------------------------------------------------------------------------------------- 3. the two forms
_FORM_CHILD = r"""
import sys
import numpy as np
from hooks_py import HooksMapper
import gie
sys.path.insert(0, %r)
import ground_pose_nf1_ref as Q
size = (192, %d, 2)
rng = np.random.default_rng(3)
t = np.ones((size[1], size[0]), np.int8)
for _ in range(30):
    x, y = int(rng.integers(0, 190)), int(rng.integers(0, size[1] - 2))
    t[y:y + int(rng.integers(2, 12)), x:x + int(rng.integers(2, 12))] = 2
t[100:140, 90:130] = 1
lab = np.ascontiguousarray(np.broadcast_to(t[None], (2, size[1], size[0])))
m = HooksMapper(gie.make_config(0.1, size, fast_mode=False, cutoff_dist=3.0))
for _ in range(2):
    m.set_pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    m.ogm_labels(lab)
    m.step()
pvt = m.pivot()
m.ground_compute(pvt[2], pvt[2] + 1)
g = m.read_ground()
goal = ((np.array([[110.0, 120.0]]) + np.array(pvt[:2])).astype(np.float32) * np.float32(0.1)).astype(np.float32)
sys.stderr.write("BEGIN\n"); sys.stderr.flush()
counts = m.ground_pose_nf1_compute(goal, None, 25, 4, 4, 0, False, False, %s)
sys.stderr.write("END\n"); sys.stderr.flush()
f, cs = m.read_ground_pose_nf1()
nf, cb, wc = Q.field(g, goal, None, pvt, 0.1, 25, 4, 4, 0, %d)
assert counts == wc and counts[0] == 8, (counts, wc)
assert np.array_equal(cs, cb) and np.array_equal(f, nf), np.argwhere(f != nf)[:5]
assert nf.max() > 100 and (nf[:, -4:, :] >= 0).any() and (nf[:, :4, :] >= 0).any()
m.close()
"""


@pytest.mark.parametrize("Y, form, rev", [(256, "k_gpose_bfs<true>", False), (257, "k_gpose_bfs<false>", True)])
def test_the_two_forms_at_the_threshold(Y, form, rev):
    """3 words a row: 192 x 256 is exactly 768 words (the LDS form), 192 x 257 is 771 (global planes); the launch is named by the
    test build's launch trace (a switch read once per process: a child process)"""
    import os
    import sys
    env = dict(os.environ, GIE_TRACE_LAUNCHES="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    src = _FORM_CHILD % (os.path.dirname(os.path.abspath(__file__)), Y, rev, 4 if rev else 0)
    res = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr[-3000:])
    call = res.stderr.split("BEGIN\n")[1].split("END")[0]
    names = [ln.split("launch ")[1].strip() for ln in call.splitlines() if "launch " in ln]
    assert names == ["k_glos_prep", "k_gpose_cspace", "k_gpose_prep", "k_gpose_goals", form], names


# ---------------------------------------------------------------------------------------------------------- 4. the parent's calls
def test_cspace_and_paths_against_ground_footprints():
    size = (70, 32, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, _labels(size, _box_plane(size, 42)))
        g = _ground(m, size)
        X, Y = size[0], size[1]
        ys, xs = np.mgrid[0:Y, 0:X]
        xy = _xy(pvt, np.stack([xs.ravel(), ys.ravel()], 1)).reshape(-1, 1, 2)
        for e, c, u in ((FP, 0, False), ((9, 9, 1), 4, True), ((Q.MAX_SQ,) * 3, 0, True)):      # the last: the cap in all three, R = 90
            m.ground_pose_nf1_compute(_xy(pvt, [(X - 5, Y - 5)]), None, e[0], e[1], e[2], c, u, False, True)
            f, cs = m.read_ground_pose_nf1()
            for k, d in enumerate(Q.DIRS):                      # bit k of every byte = end == 1 of the T = 1 pose with heading d_k
                hd = np.ascontiguousarray(np.broadcast_to(np.array(d, np.int32), (X * Y, 1, 2)))
                rec = m.ground_footprints(xy, hd, e[0], e[1], e[2], c, u)
                assert np.array_equal((rec["end"] == 1).reshape(Y, X), ((cs >> k) & 1).astype(bool)), (e, k)
            starts, sk = _starts(g, pvt, np.random.default_rng(1), 60)
            path, ln = m.ground_pose_nf1_path(starts, sk, 200)
            assert ((ln > 1).sum() > 10 or e[0] == Q.MAX_SQ) and ln.max() <= 200
            for i in np.flatnonzero(ln > 0):
                p = path[i, :ln[i]].astype(np.int64)
                pxy = ((p[:, :2].astype(np.float32)) * np.float32(W)).astype(np.float32).reshape(-1, 1, 2)
                hd = np.array([Q.DIRS[k] for k in p[:, 2]], np.int32).reshape(-1, 1, 2)
                assert (m.ground_footprints(pxy, hd, e[0], e[1], e[2], c, u)["end"] == 0).all()      # every pose is clear
                for a, b in zip(p[:-1], p[1:]):                  # one admissible move apart
                    assert tuple(b) in Q.moves(int(a[0]), int(a[1]), int(a[2]), True)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. the chain
def test_chain_from_the_frontier_clusters_with_one_sync():
    import torch
    size = (70, 32, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, _labels(size, _box_plane(size, 43)))
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        K, L = 16, 120
        start = _xy(pvt, [(60, 20), (50, 10), (40, 25), (20, 15)])
        with torch.cuda.stream(st):
            dgoal = torch.zeros((K, 2), dtype=torch.float32, device=dev)
            dcnt = torch.zeros((2,), dtype=torch.int32, device=dev)
            ds = torch.from_numpy(start).to(dev)
            dp = torch.full((4 * L * 3,), -7, dtype=torch.int32, device=dev)
            dl = torch.zeros((4,), dtype=torch.int32, device=dev)
            m.ground_compute_dev(pvt[2] + 2, pvt[2] + 5, 1, False)
            m.ground_frontier_compute_dev(0, 1, 8, K)
            m.read_ground_frontier_clusters_dev(0, dgoal.data_ptr(), 0)
            m.ground_pose_nf1_compute_dev(dgoal.data_ptr(), 0, K, dcnt.data_ptr(), 9, 9, 1, 0, True, False, True)
            m.ground_pose_nf1_path_dev(ds.data_ptr(), 0, 4, L, dp.data_ptr(), dl.data_ptr())
        m.sync()                                                # the one sync
        g = m.read_ground()
        goals = dgoal.cpu().numpy()
        assert np.isnan(goals).any() and np.isfinite(goals).any()       # the NaN tail is taken as it is
        nf, cb, counts = Q.field(g, goals, None, pvt, W, 9, 9, 1, 0, Q.REVERSE | Q.UNKNOWN_TRAVERSABLE)
        wp, wl = Q.path(nf, start, None, pvt, W, L, True, fill=-7)
        assert dcnt.cpu().tolist() == counts and counts[0] > 0
        assert dl.cpu().numpy().tolist() == wl.tolist() and dp.cpu().numpy().tobytes() == wp.tobytes() and (wl > 1).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. state
def test_lifetime_invalidation_and_neighbours_untouched():
    size = (65, 40, 8)
    m = _mapper(size)
    try:
        lab = _labels(size, _box_plane(size, 44))
        pvt = _settle(m, lab)
        g = _ground(m, size)
        goal = _xy(pvt, [(60, 30)])
        m.ground_nf1_compute(goal, 1)
        gn = m.read_ground_nf1()
        m.ground_pose_nf1_compute(goal, None, 9, 9, 1)
        first = m.read_ground_pose_nf1()
        g2 = m.read_ground()
        assert all(np.array_equal(g[k], g2[k]) for k in g) and np.array_equal(m.read_ground_nf1(), gn)      # neither the field nor ground NF1
        pos, q = scenes.pose(3, W, delta_vox=4, yaw_deg=0.0)
        _update(m, pos, q, lab)                                 # a map update changes nothing
        assert tuple(m.pivot()) != tuple(pvt)
        again = m.read_ground_pose_nf1()
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        assert np.array_equal(m.ground_pose_nf1_query(goal, [-1]), Q.query(first[0], goal, [-1], pvt, W))
        m.ground_nf1_compute(goal, 4)                           # ground NF1 does not invalidate it
        assert m.read_ground_pose_nf1()[0].tobytes() == first[0].tobytes()
        m.ground_pose_nf1_compute(goal, None, 0, 0, 0)          # nor the other way round
        assert np.array_equal(m.read_ground_nf1(), N.field(g, goal, pvt, W, 4)[0])
        z = m.pivot()[2]
        m.ground_compute(z, z + 7)                              # a new ground field invalidates it
        buf = np.zeros(8 * 65 * 40, np.int32)
        p = buf.ctypes.data_as(C.c_void_p)
        xy = goal.ctypes.data_as(C.c_void_p)
        assert m._f["read_ground_pose_nf1"](m._h, p, None) == INVALID and m._f["ground_pose_nf1_query"](m._h, xy, None, 1, p) == INVALID
        assert m._f["ground_pose_nf1_path"](m._h, xy, None, 1, 4, p, p) == INVALID and not buf.any()
        m.ground_pose_nf1_compute(goal, None, 0, 0, 0)
        assert m.read_ground_pose_nf1()[0].shape == (8, 40, 65)
    finally:
        m.close()


def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, t = _mapper(size), _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        f = m._f
        n = 3
        host = np.frombuffer(P5A * 32768, np.uint8).copy()
        dbuf = torch.full((32768,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [(3, 3), (9, 9), (20, 4)])
        ks = np.array([0, -1, 3], np.int32)
        dxy, dks = torch.from_numpy(xy).to("cuda:0"), torch.from_numpy(ks).to("cuda:0")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        hp, hp2 = ptr(host), ptr(host[16384:])
        dp, dp2 = C.c_void_p(dbuf.data_ptr()), C.c_void_p(dbuf.data_ptr() + 16384)
        dx, dk = C.c_void_p(dxy.data_ptr()), C.c_void_p(dks.data_ptr())

        def PP(**kw):
            p = _capi.GroundPoseNf1Param(1, 1, 1, 0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert host.tobytes() == P5A * host.size and bool((dbuf == 0x5a).all())

        def compute_refused(h, who, p="default", n_=n, a=True):
            p = PP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_pose_nf1_compute"](h, ptr(xy) if a else None, ptr(ks), n_, pr, hp) == INVALID, who
            assert f["ground_pose_nf1_compute_dev"](h, dx if a else None, dk, n_, pr, dp) == INVALID, who

        def readers_refused(h, who, n_=n, max_len=4, a=True, out=True, out2=True):
            assert f["read_ground_pose_nf1"](h, hp if out else None, hp2 if out2 else None) == INVALID, who
            assert f["read_ground_pose_nf1_dev"](h, dp if out else None, dp2 if out2 else None) == INVALID, who
            assert f["ground_pose_nf1_query"](h, ptr(xy) if a else None, ptr(ks), n_, hp if out else None) == INVALID, who
            assert f["ground_pose_nf1_query_dev"](h, dx if a else None, dk, n_, dp if out else None) == INVALID, who
            assert f["ground_pose_nf1_path"](h, ptr(xy) if a else None, ptr(ks), n_, max_len, hp if out else None, hp2 if out2 else None) == INVALID, who
            assert f["ground_pose_nf1_path_dev"](h, dx if a else None, dk, n_, max_len, dp if out else None, dp2 if out2 else None) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            compute_refused(h, who)
            readers_refused(h, who)
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper
        compute_refused(t._h, "tiled")
        readers_refused(t._h, "tiled")
        unwritten()
        m.ground_compute(pvt[2], pvt[2] + 7)
        readers_refused(m._h, "before a compute")
        compute_refused(m._h, "null param", None)
        big = Q.MAX_SQ + 1
        bad = [PP(front_sq=-1), PP(front_sq=big), PP(back_sq=-1), PP(back_sq=big), PP(side_sq=-1), PP(side_sq=big), PP(side_sq=2 ** 31 - 1), PP(front_sq=-2 ** 31),
               PP(clearance_sq=-1), PP(clearance_sq=-2 ** 31), PP(flags=8), PP(flags=15), PP(flags=-2 ** 31), PP(flags=16)] + [PP(reserved=i) for i in range(3)]
        for p in bad:
            compute_refused(m._h, (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags, list(p.reserved)), p)
        compute_refused(m._h, "n < 0", n_=-1)
        compute_refused(m._h, "null goals", a=False)
        readers_refused(m._h, "still no compute")
        unwritten()
        assert f["ground_pose_nf1_compute"](m._h, None, None, 0, C.byref(PP(flags=7)), None) == 0            # n == 0 and NULL counts are valid
        assert f["ground_pose_nf1_compute_dev"](m._h, dx, None, n, C.byref(PP(front_sq=Q.MAX_SQ)), None) == 0
        unwritten()
        # with a field: the readers' own refusals (a reader with one NULL output is valid: out2=True there)
        assert f["read_ground_pose_nf1"](m._h, None, None) == INVALID and f["read_ground_pose_nf1_dev"](m._h, None, None) == INVALID
        for kw in (dict(n_=-1), dict(a=False), dict(out=False, out2=True)):
            for name, form in (("ground_pose_nf1_query", 0), ("ground_pose_nf1_path", 1)):
                a_, n_, out = kw.get("a", True), kw.get("n_", n), kw.get("out", True)
                if form == 0:
                    assert f[name](m._h, ptr(xy) if a_ else None, ptr(ks), n_, hp if out else None) == INVALID, (name, kw)
                    assert f[name + "_dev"](m._h, dx if a_ else None, dk, n_, dp if out else None) == INVALID, (name, kw)
                else:
                    assert f[name](m._h, ptr(xy) if a_ else None, ptr(ks), n_, 4, hp if out else None, hp2) == INVALID, (name, kw)
                    assert f[name + "_dev"](m._h, dx if a_ else None, dk, n_, 4, dp if out else None, dp2) == INVALID, (name, kw)
        assert f["ground_pose_nf1_path"](m._h, ptr(xy), ptr(ks), n, 4, hp, None) == INVALID and f["ground_pose_nf1_path_dev"](m._h, dx, dk, n, 4, dp, None) == INVALID
        for bad_len in (0, -1, -2 ** 31):
            assert f["ground_pose_nf1_path"](m._h, ptr(xy), ptr(ks), n, bad_len, hp, hp2) == INVALID and f["ground_pose_nf1_path_dev"](m._h, dx, dk, n, bad_len, dp, dp2) == INVALID
            assert f["ground_pose_nf1_path"](m._h, None, None, 0, bad_len, None, None) == INVALID
        unwritten()
        assert f["ground_pose_nf1_query"](m._h, None, None, 0, None) == 0 and f["ground_pose_nf1_path_dev"](m._h, None, None, 0, 1, None, None) == 0
        unwritten()
        assert f["ground_pose_nf1_query"](m._h, ptr(xy), None, n, hp) == 0 and (host[:12].view(np.int32) == -1).all() and host[12:].tobytes() == P5A * (host.size - 12)
    finally:
        m.close()
        t.close()


def test_section_calls_change_nothing_of_the_map_update():
    size = (48, 40, 16)
    rng = np.random.default_rng(5)
    boxes = []
    for _ in range(40):
        s = rng.integers(3, 10, size=3)
        c = rng.integers((-30, -24, -10), (50, 20, 8))
        boxes.append((c, c + s))

    def frame(k):
        pos, q = scenes.pose(k, W, delta_vox=3, yaw_deg=0.0)
        return pos, q, box_labels(scenes.local_pivot(pos, W, size), size, k, boxes, unknown_slab=3)

    field = {}

    def calls(a, k, phase, pos):
        if phase == "fuse" and k % 2 == 0:                       # a new ground field and ground NF1 every other frame, between fuse and merge
            field["pvt"] = scenes.local_pivot(pos, W, size)
            a.ground_compute(field["pvt"][2] + 2, field["pvt"][2] + 9, 2, k % 4 == 2)
            a.ground_nf1_compute(_xy(field["pvt"], [(24, 20)]), 0, True)
            field["nf"], field["g"] = a.read_ground_nf1(), a.read_ground()
        if phase in ("fuse", "edt", "merge"):
            goal = _xy(field["pvt"], [(24, 20), (40, 8)])
            a.ground_pose_nf1_compute(goal, [-1, k % 8], 16, 4, 4, k % 3, k % 2 == 0, True, phase == "edt")
            a.read_ground_pose_nf1()
            a.ground_pose_nf1_query(goal)
            a.ground_pose_nf1_path(goal + np.float32(0.3), None, 50)
            assert np.array_equal(a.read_ground_nf1(), field["nf"])
            g = a.read_ground()
            assert all(np.array_equal(g[key], field["g"][key]) for key in g)

    stage_calls_change_nothing(size, (frame(k) for k in range(5)), _mapper, calls, n_probe=2000)


# ---------------------------------------------------------------------------------------------------------- 7. profile and launches
def test_profile_counts_under_ground_nf1():
    import torch
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.profile_enable(True)
        m.profile_read()
        goal = _xy(pvt, [(20, 9)])
        m.ground_pose_nf1_compute(goal, None, 4, 4, 4)
        prof = m.profile_read()
        assert prof["ground_nf1"][1] == 1 and prof["ground_nf1"][0] > 0
        m.read_ground_pose_nf1()
        m.ground_pose_nf1_query(goal)
        m.ground_pose_nf1_path(goal, None, 5)
        d = torch.zeros((8 * 32 * 24,), dtype=torch.int32, device="cuda:0")
        dg = torch.from_numpy(goal).to("cuda:0")
        m.ground_pose_nf1_compute_dev(dg.data_ptr(), 0, 1, 0, 4, 4, 4)
        m.read_ground_pose_nf1_dev(d.data_ptr(), 0)
        m.ground_pose_nf1_query_dev(dg.data_ptr(), 0, 1, d.data_ptr())
        m.ground_pose_nf1_path_dev(dg.data_ptr(), 0, 1, 5, d.data_ptr(), d.data_ptr() + 1024)
        m.ground_pose_nf1_query(np.zeros((0, 2), np.float32))   # n == 0 adds nothing
        m.ground_pose_nf1_path(np.zeros((0, 2), np.float32), None, 5)
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_nf1"][1] == 7 and prof["ground_nf1"][0] > 0
        assert all(v[1] == 0 for k, v in prof.items() if k != "ground_nf1")
        assert list(prof) == NAMES
    finally:
        m.close()


_TRACE_CHILD = r"""
import sys
import numpy as np
from hooks_py import HooksMapper
import gie
m = HooksMapper(gie.make_config(0.1, (32, 24, 8), fast_mode=False, cutoff_dist=3.0))
for _ in range(2):
    m.set_pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    m.ogm_labels(np.ones((8, 24, 32), np.int8))
    m.step()
pvt = m.pivot()
m.ground_compute(pvt[2], pvt[2] + 7)
xy = ((np.array([(8, 8), (15, 15)], np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(0.1)).astype(np.float32)
def call(fn):
    sys.stderr.write("BEGIN\n"); sys.stderr.flush()
    r = fn()
    sys.stderr.write("END\n"); sys.stderr.flush()
    return r
assert call(lambda: m.ground_pose_nf1_compute(xy[:0], None, 9, 1, 4))[0] == 0
assert call(lambda: m.ground_pose_nf1_compute(xy, None, 9, 1, 4, 0, False, False, True))[0] == 16
call(lambda: m.read_ground_pose_nf1())
assert call(lambda: m.ground_pose_nf1_query(xy)).tolist() == [0, 0]
assert call(lambda: m.ground_pose_nf1_path(xy, None, 4))[1].tolist() == [1, 1]
call(lambda: m.ground_pose_nf1_query(xy[:0]))
m.close()
"""


def test_the_launches_of_every_call():
    """named by the test build's launch trace (a switch read once per process: a child process)"""
    import os
    import sys
    env = dict(os.environ, GIE_TRACE_LAUNCHES="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    res = subprocess.run([sys.executable, "-c", _TRACE_CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr)
    calls = [blk.split("END")[0] for blk in res.stderr.split("BEGIN\n")[1:]]
    names = [[ln.split("launch ")[1].strip() for ln in c.splitlines() if "launch " in ln] for c in calls]
    assert names == [["k_glos_prep", "k_gpose_cspace", "k_gpose_prep", "k_gpose_bfs<true>"],
                     ["k_glos_prep", "k_gpose_cspace", "k_gpose_prep", "k_gpose_goals", "k_gpose_bfs<true>"],
                     ["k_lin<F>"], ["k_gpose_query"], ["k_gpose_path"], []], names


# ---------------------------------------------------------------------------------------------------------- 8. host layer
def test_host_layer_ground_plan_footprint_matches_the_mapper(tmp_path):
    from stage_common import build_host_probe, lidar_frames
    exe = build_host_probe(tmp_path, "ground_pose_plan_probe")
    size, w, cutoff, gmin, gmax, min_known = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2
    yaw, max_len = 2.4, 40
    fp = (0.35, 0.15, 0.2)                                      # metres: front, back, half width
    frames, fpath = lidar_frames(tmp_path)
    robot = np.asarray(frames[-1][0][:2], np.float32)
    goal = np.array([[robot[0] + 1.5, robot[1] - 1.0], [robot[0] - 1.4, robot[1] + 1.2]], np.float32)
    gyaw = [float("nan"), -1.6]

    def run(out, footprint, band, reverse):
        args = [exe, fpath, out, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), repr(gmin), repr(gmax), str(min_known), footprint, str(band),
                repr(yaw), str(int(reverse)), str(max_len)]
        for g, a in zip(goal, gyaw):
            args += [repr(float(g[0])), repr(float(g[1])), repr(a)]
        res = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, (res.stdout, res.stderr)
        return res.stdout, np.fromfile(out + ".path", np.int32).reshape(-1, 3), np.fromfile(out + ".info", np.int32).tolist()

    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        sq = [int(np.floor((np.float32(x) / np.float32(w)) * (np.float32(x) / np.float32(w)))) for x in fp]
        k0 = Q.heading_index(float(np.float32(yaw)))
        gk = [-1, Q.heading_index(float(np.float32(gyaw[1])))]
        assert sq == [12, 2, 4] and k0 == 3 and gk == [-1, 6]
        some = False
        for reverse in (False, True):
            out, path, info = run(str(tmp_path / ("on%d" % reverse)), "[%r, %r, %r]" % fp, 1, reverse)
            counts = m.ground_pose_nf1_compute(goal, gk, sq[0], sq[1], sq[2], 0, False, False, reverse)
            wp, wl = m.ground_pose_nf1_path(robot[None], [k0], max_len)
            nf, cb, wc = Q.field(m.read_ground(), goal, gk, m.pivot(), w, sq[0], sq[1], sq[2], 0, Q.REVERSE if reverse else 0)
            assert counts == wc and np.array_equal(m.read_ground_pose_nf1()[0], nf)
            assert info == [4, int(wl[0]), counts[0], k0] + sq and "made 4 " in out
            n = min(int(wl[0]), max_len)
            assert path.shape == (n, 3) and path.tobytes() == wp[0, :n].tobytes()            # the Mapper's triples on the same inputs
            if n:
                some = True
                pxy = (path[:, :2].astype(np.float32) * np.float32(w)).astype(np.float32).reshape(-1, 1, 2)
                hd = np.array([Q.DIRS[k] for k in path[:, 2]], np.int32).reshape(-1, 1, 2)
                assert (m.ground_footprints(pxy, hd, sq[0], sq[1], sq[2])["end"] == 0).all()      # every pose is clear
        assert some
    finally:
        m.close()
    for name, footprint, band in (("nofp", "-", 1), ("noband", "[%r, %r, %r]" % fp, 0)):           # refused: everything left alone
        out, path, info = run(str(tmp_path / name), footprint, band, False)
        assert "made 0 len -5 sources -6 triples 2" in out and path.tolist() == [[-7] * 3] * 2 and info[:3] == [0, -5, -6]

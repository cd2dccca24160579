"""Ground line of sight on the device (include/gie.h "ground line of sight", gie_ground_los.inc.h) against the numpy statement of
tests/ground_los_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is exact, most of bytes:
the waypoint arrays including the entries beyond a path's records (prefilled with 0x5a)."""
import ctypes as C
import subprocess
import time

import numpy as np
import pytest

import gie
import ground_los_ref as L
import ground_nf1_ref as N
import ground_ref as R
import los_ref
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, ground as _ground, xy as _xy, scene as _scene, same as _same
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries before this section existed


def _prefill(n, cap):
    return np.frombuffer(P5A * (24 * n * cap), gie.GROUND_WAYPOINT_DTYPE).reshape(n, cap).copy()


def _segment_cells(rng, size):
    """300 pairs of cells (local, some outside): random ones, a == b, axis-parallel lines, exact diagonals, lines across the word
    boundaries of a row"""
    X, Y = size[0], size[1]
    def rnd(k):
        return np.stack([rng.integers(-3, X + 3, k), rng.integers(-3, Y + 3, k)], 1)
    a, b = [rnd(190)], [rnd(190)]
    same = rnd(20)
    a.append(same); b.append(same)
    ax = np.stack([rng.integers(0, X, 30), rng.integers(0, Y, 30)], 1)      # axis-parallel: along x, then along y
    bx = ax.copy()
    bx[:15, 0] = rng.integers(0, X, 15)
    bx[15:, 1] = rng.integers(0, Y, 15)
    a.append(ax); b.append(bx)
    d0 = np.stack([rng.integers(0, X, 30), rng.integers(0, Y, 30)], 1)      # exact diagonals inside the rectangle
    sg = rng.choice([-1, 1], (30, 2))
    room = np.minimum(np.where(sg[:, 0] > 0, X - 1 - d0[:, 0], d0[:, 0]), np.where(sg[:, 1] > 0, Y - 1 - d0[:, 1], d0[:, 1]))
    d1 = d0 + np.minimum(rng.integers(0, max(X, Y), 30), room)[:, None] * sg
    a.append(d0); b.append(d1)
    wa = np.stack([rng.integers(max(min(60, X - 1) - 8, 0), min(62, X), 30), rng.integers(0, Y, 30)], 1)          # across x = 63 | 64 (and 127 | 128)
    wb = np.stack([rng.integers(min(64, X - 1), X, 30), rng.integers(0, Y, 30)], 1)
    a.append(wa); b.append(wb)
    a, b = np.concatenate(a), np.concatenate(b)
    assert len(a) == 300
    return a, b


def _segment_points(rng, size, pvt):
    a, b = _segment_cells(rng, size)
    pa, pb = _xy(pvt, a), _xy(pvt, b)
    pa[:40] = _xy(pvt, a[:40], 0.5)                             # ties of gie_pos2coord's rounding
    odd = np.array([np.nan, np.inf, -np.inf, 1e30, -3e9], np.float32)
    pa[40:45, 0] = odd
    pb[45:50, 1] = odd
    return pa, pb


# ---------------------------------------------------------------------------------------------------------- 1. segments
@pytest.mark.parametrize("size", [(64, 24, 8), (65, 24, 8), (70, 24, 8), (130, 24, 8), (130, 1, 8)])
def test_segments_equal_the_reference(size):
    import torch
    pos, lab = _scene(size, 100 + size[0] + size[1])
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        rng = np.random.default_rng(size[0])
        pa, pb = _segment_points(rng, size, pvt)
        seen = set()
        for blocks in (False, True):
            g = _ground(m, size, blocks=blocks)
            assert (g["type"] == R.UNKNOWN).any() and (g["type"] == R.OCCUPIED).any()
            for csq in (0, 4, 9):
                for ut in (False, True):
                    got = m.ground_segments(pa, pb, csq, ut)
                    want = L.segments(g, pa, pb, pvt, W, csq, int(ut))
                    assert got.dtype == L.HIT_DTYPE
                    _same(got, want, (blocks, csq, ut))
                    fs = want["first"]
                    seen |= {int(v) for v in np.unique(fs[fs <= 0])} | ({"hit%d" % (csq > 0)} if (fs > 0).any() else set())
                    ok = want["first"] != -2
                    assert ((want["min_dist_sq"][want["first"] == -1] >= csq) | (want["min_dist_sq"][want["first"] == -1] == -1)).all()
                    assert (want["len"][ok] >= 1).all() and not want["reserved"].any()
        assert {-2, -1, 0, "hit0", "hit1"} <= seen              # outside or not finite, clear, blocked at the start, blocked on the way
        # the _dev form: the same bytes
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            da, db = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
            dout = torch.full((len(pa) * 24 + 1,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_segments_dev(da.data_ptr(), db.data_ptr(), len(pa), dout.data_ptr(), 4, True)
        m.sync()
        o = dout.cpu().numpy()
        assert o[:-1].tobytes() == m.ground_segments(pa, pb, 4, True).tobytes() and o[-1] == 0x5a
        assert len(m.ground_segments(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))) == 0      # n == 0
    finally:
        m.close()


def test_a_field_without_an_obstacle_column_passes_every_clearance():
    size = (70, 30, 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((2, 30, 70), np.int8))
        g = _ground(m, size)
        assert (g["dist_sq"] == -1).all()
        pa, pb = _segment_points(np.random.default_rng(1), size, pvt)
        cells = np.array([[(x, 3) for x in range(60)] + [(59, y) for y in range(4, 24)]])
        path = (cells + np.array(pvt[:2])).astype(np.int32)
        for csq in (0, 9, 2 ** 31 - 1):
            got = m.ground_segments(pa, pb, csq)
            _same(got, L.segments(g, pa, pb, pvt, W, csq), csq)
            ok = got["first"] != -2
            assert ok.sum() > 100 and (got["first"][ok] == -1).all() and (got["min_dist_sq"][ok] == -1).all()
            wp, info = m.ground_shortcut(path, [80], 4096, 4, csq, wp=_prefill(1, 4))
            rwp, rinfo = L.shortcut(g, path, [80], pvt, 4096, 4, csq, wp_init=_prefill(1, 4))
            _same(wp, rwp, csq)
            _same(info, rinfo, csq)
            assert info["count"][0] == 2 and wp["index"][0, :2].tolist() == [0, 79] and wp["min_dist_sq"][0, :2].tolist() == [-1, -1]
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. shortcut
KS = (1, 63, 64, 65, 128, 4096)


def _invariants(wp, info, lens, max_len, csq):
    """stated without the reference: indices rise strictly from 0 to m - 1; a clear leg's minimum passes the clearance"""
    for i in range(len(info)):
        m_ = int(min(max(int(lens[i]), 0), max_len))
        c = int(info["count"][i])
        assert (c == 0) == (m_ == 0)
        if c:
            idx = wp["index"][i, :c]
            assert idx[0] == 0 and idx[-1] == m_ - 1 and (np.diff(idx) > 0).all()
            leg = wp[i, 1:c]
            cl = leg[leg["forced"] == 0]
            assert ((cl["min_dist_sq"] >= csq) | (cl["min_dist_sq"] == -1)).all() and (leg["min_dist_sq"][leg["forced"] == 1] == -2).all()
            assert int(leg["forced"].sum()) == info["forced"][i]


@pytest.mark.parametrize("size", [(70, 24, 8), (130, 24, 8)])
def test_shortcut_of_ground_nf1_paths_without_a_host_step(size):
    import torch
    pos, lab = _scene(size, 300 + size[0], n_boxes=10)
    m = _mapper(size)
    max_len, csq, ample = 100, 4, 100
    try:
        pvt = _settle(m, lab, pos)
        z = pvt[2]
        g = _ground(m, size)
        rng = np.random.default_rng(size[0])
        free = np.argwhere(~L.blocked(g, csq))[:, ::-1]          # (over the whole height most columns are FNT: the volume's own faces)
        goal = _xy(pvt, [free[0]])
        cells = np.stack([rng.integers(-1, size[0] + 1, 24), rng.integers(-1, size[1] + 1, 24)], 1)
        cells[:4] = [(-1, 3), free[-1], free[-5], free[-9]]     # one start outside, three far from the goal
        starts = _xy(pvt, cells)
        n = len(starts)
        combos = [(K, ample) for K in KS] + [(64, 0), (64, 1), (4096, 1), (63, 3)]
        other = 9                                               # another clearance than the paths': legs are forced
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        out = {}
        with torch.cuda.stream(st):
            dg, ds = torch.from_numpy(goal).to(dev), torch.from_numpy(starts).to(dev)
            dpath = torch.full((n, max_len, 2), 0x5a5a5a5a, dtype=torch.int32, device=dev)
            dlen = torch.zeros(n, dtype=torch.int32, device=dev)
            m.ground_compute_dev(z, z + size[2] - 1, 1, False, 0)
            m.ground_nf1_compute_dev(dg.data_ptr(), 1, csq, False, False, 0)
            m.ground_nf1_path_dev(ds.data_ptr(), n, max_len, dpath.data_ptr(), dlen.data_ptr())
            for K, cap in combos + [(64, -1), (128, -2)]:
                c_sq = other if cap == -2 else csq
                cap_ = ample if cap < 0 else cap
                dwp = torch.full((n * cap_ * 24 + 1,), 0x5a, dtype=torch.uint8, device=dev)
                dinfo = torch.full((n * 16 + 1,), 0x5a, dtype=torch.uint8, device=dev)
                m.ground_shortcut_dev(dpath.data_ptr(), dlen.data_ptr(), n, max_len, dwp.data_ptr() if cap_ else 0, 0 if cap == -1 else dinfo.data_ptr(),
                                      K, cap_, c_sq)
                out[K, cap] = (dwp, dinfo)
        m.sync()                                                # the only wait
        buf, lens = dpath.cpu().numpy(), dlen.cpu().numpy()
        nf = N.field(g, goal, pvt, W, csq)[0]
        rp, rl = N.path(nf, starts, pvt, W, max_len, fill=0x5a5a5a5a)
        assert np.array_equal(buf, rp) and np.array_equal(lens, rl)
        assert (lens == 0).any() and (lens > 20).sum() >= 3
        ref = {}
        for K, cap in combos + [(64, -1), (128, -2)]:
            c_sq = other if cap == -2 else csq
            cap_ = ample if cap < 0 else cap
            key = (K, c_sq)
            if key not in ref:                                  # (the records do not depend on the capacity: one statement per look-ahead)
                ref[key] = L.shortcut(g, buf, lens, pvt, K, ample, c_sq)
            full, rinfo = ref[key]
            rwp = _prefill(n, cap_)
            for i in range(n):
                k = min(int(rinfo["count"][i]), cap_)
                rwp[i, :k] = full[i, :k]
            gw, gi = out[K, cap][0].cpu().numpy(), out[K, cap][1].cpu().numpy()
            assert gw[:-1].tobytes() == rwp.tobytes() and gw[-1] == 0x5a, (K, cap)
            assert gi[:-1].tobytes() == (P5A * (16 * n) if cap == -1 else rinfo.tobytes()) and gi[-1] == 0x5a, (K, cap)
            _invariants(full, rinfo, lens, max_len, c_sq)
            if cap != -2:
                assert not rinfo["forced"].any()                # consecutive cells of an NF1 path are traversable neighbours
        assert ref[128, other][1]["forced"].sum() > 0
        assert (ref[4096, csq][1]["count"] < np.clip(lens, 0, max_len)).any() and (ref[4096, csq][1]["count"] >= 3).any()
        assert (ref[1, csq][1]["count"] == np.clip(lens, 0, max_len)).all()
        # the capacity's own statement and the host form: the same bytes
        for K, cap in ((64, 1), (63, 3)):
            rwp, rinfo = L.shortcut(g, buf, lens, pvt, K, cap, csq, wp_init=_prefill(n, cap))
            assert out[K, cap][0].cpu().numpy()[:-1].tobytes() == rwp.tobytes() and out[K, cap][1].cpu().numpy()[:-1].tobytes() == rinfo.tobytes()
        hwp, hinfo = m.ground_shortcut(buf, lens, 65, ample, csq, wp=_prefill(n, ample))
        assert hwp.tobytes() == out[65, ample][0].cpu().numpy()[:-1].tobytes() and hinfo.tobytes() == out[65, ample][1].cpu().numpy()[:-1].tobytes()
    finally:
        m.close()


def test_shortcut_of_random_polylines_of_any_int32():
    size = (65, 24, 8)
    pos, lab = _scene(size, 77, n_boxes=6)
    m = _mapper(size)
    n, max_len = 40, 80
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size, blocks=True)
        rng = np.random.default_rng(8)
        inside = np.stack([rng.integers(0, size[0], (n, max_len)), rng.integers(0, size[1], (n, max_len))], 2)
        steps = np.cumsum(rng.integers(-1, 2, (n, max_len, 2)), axis=1) + inside[:, :1]           # slow drifts, points repeat
        pts = np.where(rng.random((n, 1, 1)) < 0.5, inside, steps) + np.array(pvt[:2])
        near = rng.random((n, max_len)) < 0.05
        pts[near] += rng.integers(-80, 80, (int(near.sum()), 2))                                  # some just outside
        wild = rng.random((n, max_len)) < 0.03
        pts = pts.astype(np.int64)
        pts[wild] = rng.integers(-2 ** 31, 2 ** 31, (int(wild.sum()), 2))
        pts[0, 0], pts[1, 5] = (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)
        buf = pts.astype(np.int32)
        lens = rng.integers(1, max_len + 1, n).astype(np.int32)
        lens[:8] = [0, -1, -2 ** 31, 1, 2, max_len + 1, 2 ** 31 - 1, max_len]
        f = m._f
        for K in (1, 64, 4096):
            for csq, ut in ((0, True), (4, False)):
                full, rinfo = L.shortcut(g, buf, lens, pvt, K, max_len, csq, int(ut), wp_init=_prefill(n, max_len))
                _invariants(full, rinfo, lens, max_len, csq)
                assert rinfo["forced"].sum() > 0 and (rinfo["forced"] == 0).sum() > 0 and (rinfo["length"] > 0).any()
                for cap in (0, 1, max_len):
                    rwp = _prefill(n, cap)
                    for i in range(n):
                        k = min(int(rinfo["count"][i]), cap)
                        rwp[i, :k] = full[i, :k]
                    wp, info = m.ground_shortcut(buf, lens, K, cap, csq, ut, wp=_prefill(n, cap))
                    _same(info, rinfo, (K, csq, cap))
                    _same(wp, rwp, (K, csq, cap))
            # info NULL; wp NULL with max_wp 0
            p = m.ground_shortcut_param(K, max_len, 4, False)
            wp = _prefill(n, max_len)
            assert f["ground_shortcut"](m._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, max_len, C.byref(p), wp.ctypes.data_as(C.c_void_p), None) == 0
            assert wp.tobytes() == full.tobytes()
            p0 = m.ground_shortcut_param(K, 0, 4, False)
            info = np.zeros(n, gie.SHORTCUT_INFO_DTYPE)
            assert f["ground_shortcut"](m._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, max_len, C.byref(p0), None, info.ctypes.data_as(C.c_void_p)) == 0
            assert info.tobytes() == rinfo.tobytes()
        assert f["ground_shortcut"](m._h, None, None, 0, 4, C.byref(p0), None, info.ctypes.data_as(C.c_void_p)) == 0     # n == 0 (max_wp 0: wp may be NULL)
        assert info.tobytes() == rinfo.tobytes()                # (and nothing was written)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. against the 3-D section
def test_a_flat_volume_agrees_with_the_3d_line_of_sight_and_shortcut():
    size = (70, 24, 1)
    pos, lab = _scene(size, 41, n_boxes=8)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        loc = m.read_local(dist_sq=False, coc=False)
        g = _ground(m, size)
        assert np.array_equal(g["type"], loc["type"][0])        # every column is its one voxel: ground_ref.columns' rule at Z = 1, min_known = 1
        assert np.array_equal(g["type"], R.columns(loc["type"], pvt[2], pvt[2], pvt[2])[0])
        assert (g["type"] == R.UNKNOWN).any() and (g["type"] == R.OCCUPIED).any()
        pa, pb = _segment_points(np.random.default_rng(3), size, pvt)
        zw = np.full((len(pa), 1), np.float32(pvt[2]) * np.float32(W), np.float32)
        a3, b3 = np.concatenate([pa, zw], 1), np.concatenate([pb, zw], 1)
        free = np.argwhere(~L.blocked(g))[:, ::-1]
        goal = _xy(pvt, [free[len(free) // 3]])
        rng = np.random.default_rng(4)
        starts = _xy(pvt, np.stack([rng.integers(0, size[0], 30), rng.integers(0, size[1], 30)], 1))
        m.ground_nf1_compute(goal, 0, True)
        path, lens = m.ground_nf1_path(starts, 90)
        path3 = np.concatenate([path, np.full(path.shape[:2] + (1,), pvt[2], np.int32)], 2)
        assert (lens > 20).sum() >= 3
        for flag3 in (0, los_ref.UNKNOWN_OPAQUE):               # 3-D flag 0 = UNKNOWN is transparent = the ground flag set, and the reverse
            ut = flag3 == 0
            m.los_prepare(0.0, flag3)
            h3, h2 = m.los_segments(a3, b3), m.ground_segments(pa, pb, 0, ut)
            assert np.array_equal(h3["first"], h2["first"]) and np.array_equal(h3["len"], h2["len"]) and np.array_equal(h3["hit"][:, :2], h2["hit"])
            assert (h2["first"] >= 0).sum() > 20 and (h2["first"] == -1).sum() > 20 and (h2["first"] == -2).sum() > 5
            for K in (1, 64, 4096):
                w3, i3 = m.path_shortcut(path3, lens, K, 90)
                w2, i2 = m.ground_shortcut(path, lens, K, 90, 0, ut)
                assert np.array_equal(w3["index"], w2["index"]) and np.array_equal(w3["forced"], w2["forced"])
                assert i3.tobytes() == i2.tobytes()
                assert ut is False or not i2["forced"].any()    # (the paths' own rule: nothing is forced)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, t = _mapper(size), _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        f = m._f
        n = 4
        host = [np.frombuffer(P5A * 4096, np.uint8).copy() for _ in range(2)]
        dbuf = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [(3, 3), (9, 9), (20, 4), (1, 1)])
        path = (np.array([[(3, 3), (4, 3), (5, 3), (6, 3)]] * n) + np.array(pvt[:2])).astype(np.int32)
        lens = np.full(n, 4, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())

        def SP(**kw):
            p = _capi.GroundLosParam(0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def CP(**kw):
            p = _capi.GroundShortcutParam(8, 4, 0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert all(a.tobytes() == P5A * a.size for a in host) and bool((dbuf == 0x5a).all())

        def seg(h, who, p="default", n_=n, a=True, b=True, out=True):
            p = SP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_segments"](h, ptr(xy) if a else None, ptr(xy) if b else None, n_, pr, ptr(host[0]) if out else None) == INVALID, who
            assert f["ground_segments_dev"](h, dp if a else None, dp if b else None, n_, pr, dp if out else None) == INVALID, who

        def cut(h, who, p="default", n_=n, max_len=4, pa=True, le=True, wp=True, info=True):
            p = CP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_shortcut"](h, ptr(path) if pa else None, ptr(lens) if le else None, n_, max_len, pr, ptr(host[0]) if wp else None,
                                        ptr(host[1]) if info else None) == INVALID, who
            assert f["ground_shortcut_dev"](h, dp if pa else None, dp if le else None, n_, max_len, pr, dp if wp else None, dp if info else None) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            seg(h, who)
            cut(h, who)
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper: all four refuse
        seg(t._h, "tiled")
        cut(t._h, "tiled")
        unwritten()
        z = pvt[2]
        m.ground_compute(z, z + 7)
        seg(m._h, "null param", None)
        cut(m._h, "null param", None)
        for p in [SP(clearance_sq=-1), SP(clearance_sq=-2 ** 31), SP(flags=2), SP(flags=3), SP(flags=-2 ** 31), SP(reserved=0), SP(reserved=1)]:
            seg(m._h, (p.clearance_sq, p.flags, list(p.reserved)), p)
        for p in [CP(clearance_sq=-1), CP(flags=2), CP(flags=-2 ** 31), CP(lookahead=0), CP(lookahead=-1), CP(lookahead=4097), CP(max_wp=-1)] + \
                 [CP(reserved=i) for i in range(4)]:
            cut(m._h, (p.lookahead, p.max_wp, p.clearance_sq, p.flags, list(p.reserved)), p)
        seg(m._h, "n < 0", n_=-1)
        cut(m._h, "n < 0", n_=-1)
        seg(m._h, "null a", a=False)
        seg(m._h, "null b", b=False)
        seg(m._h, "null out", out=False)
        cut(m._h, "null path", pa=False)
        cut(m._h, "null len", le=False)
        cut(m._h, "max_len 0", max_len=0)
        cut(m._h, "max_len < 0", max_len=-3)
        cut(m._h, "max_len 0 with n 0", n_=0, max_len=0)
        cut(m._h, "wp null with max_wp > 0", wp=False)
        cut(m._h, "wp and info null", CP(max_wp=0), wp=False, info=False)
        unwritten()
        # (the same calls with good arguments work)
        assert f["ground_segments"](m._h, ptr(xy), ptr(xy[::-1].copy()), n, C.byref(SP()), ptr(host[0])) == 0
        assert host[0][:24 * n].view(L.HIT_DTYPE)["first"].tolist() == [-1] * n
        p = CP()
        assert f["ground_shortcut"](m._h, ptr(path), ptr(lens), n, 4, C.byref(p), ptr(host[0]), ptr(host[1])) == 0
        assert host[1][:16 * n].view(L.INFO_DTYPE)["count"].tolist() == [2] * n
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 5. nothing else is written
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
        if phase == "fuse" and k % 2 == 0:                       # a new ground field every other frame, between fuse and merge
            field["pvt"] = scenes.local_pivot(pos, W, size)
            a.ground_compute(field["pvt"][2] + 2, field["pvt"][2] + 9, 2, k % 4 == 2)
        if phase in ("fuse", "edt", "merge"):
            gp = field["pvt"]
            r = np.random.default_rng(k)
            pa, pb = _xy(gp, r.integers(0, 40, (50, 2))), _xy(gp, r.integers(0, 40, (50, 2)))
            a.ground_segments(pa, pb, k % 3, k % 2 == 0)
            path = (np.stack([np.arange(30) + 5, np.full(30, 7 + k)], 1)[None] + np.array(gp[:2])).astype(np.int32)
            a.ground_shortcut(path, [30], 64, 8, 1)

    stage_calls_change_nothing(size, (frame(k) for k in range(5)), _mapper, calls, n_probe=2000)


def test_the_field_decides_and_a_map_update_does_not():
    size = (64, 48, 8)
    rng = np.random.default_rng(7)
    boxes = []
    for _ in range(40):
        s = rng.integers(3, 10, size=3)
        c = rng.integers((-40, -28, -6), (60, 24, 4))
        boxes.append((c, c + s))
    m = _mapper(size)
    try:
        def step(k):
            pos, q = scenes.pose(k, W, delta_vox=5, yaw_deg=0.0)
            pvt = scenes.local_pivot(pos, W, size)
            m.set_pose(pos, q)
            m.ogm_labels(box_labels(pvt, size, k, boxes, unknown_slab=2))
            m.step()
            return pvt
        pvt0 = step(0)
        g0 = _ground(m, size)
        goal = _xy(pvt0, [(30, 24)])
        m.ground_nf1_compute(goal, 1, False, True)
        nf0 = m.read_ground_nf1()
        starts = _xy(pvt0, [(5, 5), (60, 40), (33, 20), (50, 8)])
        path, lens = m.ground_nf1_path(starts, 96)
        pa, pb = _segment_points(np.random.default_rng(9), size, pvt0)
        h0 = m.ground_segments(pa, pb, 1)
        w0, i0 = m.ground_shortcut(path, lens, 64, 32, 1)
        _same(h0, L.segments(g0, pa, pb, pvt0, W, 1), "before")
        # the calls wrote nothing of the ground field or of its navigation function
        g0b = m.read_ground()
        assert all(np.array_equal(g0[k], g0b[k]) for k in g0) and np.array_equal(m.read_ground_nf1(), nf0)
        p1, l1 = m.ground_nf1_path(starts, 96)
        assert np.array_equal(p1, path) and np.array_equal(l1, lens)
        # a map update between two calls changes no result: the field stays at its own pivot
        pvt1 = step(1)
        assert tuple(pvt1) != tuple(pvt0)
        assert m.ground_segments(pa, pb, 1).tobytes() == h0.tobytes()
        w1, i1 = m.ground_shortcut(path, lens, 64, 32, 1)
        assert w1.tobytes() == w0.tobytes() and i1.tobytes() == i0.tobytes()
        # a new ground field does: later calls see it, at its pivot, with no prepare in between (and without a navigation function)
        g1 = _ground(m, size)
        h1 = m.ground_segments(pa, pb, 1)
        _same(h1, L.segments(g1, pa, pb, pvt1, W, 1), "after")
        assert h1.tobytes() != h0.tobytes()
        w2, i2 = m.ground_shortcut(path, lens, 64, 32, 1)
        rw, ri = L.shortcut(g1, path, lens, pvt1, 64, 32, 1)
        _same(w2, rw, "after")
        _same(i2, ri, "after")
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. profile
def test_profile_counts_under_ground_query():
    import torch
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.profile_enable(True)
        m.profile_read()
        xy = _xy(pvt, [(3, 3), (20, 9)])
        path = (np.array([[(3, 3), (4, 3), (5, 3)]]) + np.array(pvt[:2])).astype(np.int32)
        m.ground_segments(xy, xy[::-1].copy())
        m.ground_shortcut(path, [3], 8, 4)
        d = torch.zeros((256,), dtype=torch.uint8, device="cuda:0")
        dxy = torch.from_numpy(xy).to("cuda:0")
        m.ground_segments_dev(dxy.data_ptr(), dxy.data_ptr(), 2, d.data_ptr())
        m.ground_segments(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))      # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_query"][1] == 3 and prof["ground_query"][0] > 0
        assert all(v[1] == 0 for k, v in prof.items() if k != "ground_query")
        assert list(prof) == NAMES
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. at size
def test_at_size_512x512x24():
    size = (512, 512, 24)
    rng = np.random.default_rng(512)
    boxes = [(lo, lo + s) for lo, s in zip(np.stack([rng.integers(-250, 250, 300), rng.integers(-250, 250, 300), rng.integers(-14, 10, 300)], 1),
                                           rng.integers(2, 12, (300, 3)))]
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, W, size)
        lab = box_labels(pvt, size, 0, boxes, unknown_slab=6)
        assert tuple(_settle(m, lab, pos)) == tuple(pvt)
        m.ground_compute(pvt[2] + 4, pvt[2] + 15, 3)
        g = m.read_ground()
        free = np.argwhere((g["type"] == R.FREE) & (g["dist_sq"] >= 9))
        goal = free[np.argmin(np.abs(free - 256).sum(axis=1))][::-1]
        m.ground_nf1_compute(_xy(pvt, [goal]), 9)
        nf = m.read_ground_nf1()
        far = np.argwhere(nf == nf.max())[0][::-1]
        path, lens = m.ground_nf1_path(_xy(pvt, [far]), 1024)
        assert lens[0] > 400
        wp, info = m.ground_shortcut(path, lens, 256, 1024, 9, wp=_prefill(1, 1024))
        t0 = time.time()
        rwp, rinfo = L.shortcut(g, path, lens, pvt, 256, 1024, 9, wp_init=_prefill(1, 1024))
        print("reference: %.2f s, %d waypoints of %d points" % (time.time() - t0, rinfo["count"][0], lens[0]))
        _same(info, rinfo, "at size")
        _same(wp, rwp, "at size")
        _invariants(wp, info, lens, 1024, 9)
        assert info["forced"][0] == 0 and 2 <= info["count"][0] < min(int(lens[0]), 1024)
        # segments from the start to every waypoint's cell: clear exactly along the legs' own lines
        ends = wp["xy"][0, 1:info["count"][0]].astype(np.int64) - np.array(pvt[:2])
        begs = wp["xy"][0, :info["count"][0] - 1].astype(np.int64) - np.array(pvt[:2])
        h = m.ground_segments(_xy(pvt, begs), _xy(pvt, ends), 9)
        assert (h["first"] == -1).all() and np.array_equal(h["min_dist_sq"], wp["min_dist_sq"][0, 1:info["count"][0]])
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. host layer
def test_host_layer_ground_waypoints_match_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_waypoints_probe")
    size, w, cutoff, gmin, gmax, min_known, radius, max_len, lookahead = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15, 24, 16
    frames, fpath = lidar_frames(tmp_path)
    goal = np.array([[frames[-1][0][0] + 1.5, frames[-1][0][1] - 1.0], [frames[-1][0][0] - 1.4, frames[-1][0][1] + 1.2]], np.float32)
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.set_ext_boxes(np.array([[-3.6, -3.2, 0.2]], np.float32), np.array([[4.4, 3.4, 2.6]], np.float32), np.zeros(1, np.uint8))
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        g = m.read_ground()
        pvt = m.pivot()
        csq = int(np.ceil(np.float32(radius) / np.float32(w))) ** 2
        assert csq == 4
        start = np.array([frames[-1][0][:2]], np.float32)
        results = {}
        for ff in (0, 1):
            ns = m.ground_nf1_compute(goal, csq, False, bool(ff))
            path, ln = m.ground_nf1_path(start, max_len)
            k = min(int(ln[0]), max_len)
            wp, info = m.ground_shortcut(path[:, :max(k, 1)], [k], lookahead, max(k, 1), csq)
            rwp, rinfo = L.shortcut(g, path[:, :max(k, 1)], [k], pvt, lookahead, max(k, 1), csq)
            _same(wp, rwp, ff)
            _same(info, rinfo, ff)
            results[ff] = (wp[0, :info["count"][0]], info[0], int(ln[0]), ns)
    finally:
        m.close()
    assert results[0][2] > 1 and results[0][1]["count"] >= 2 and results[0][1]["forced"] == 0
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    gs = [repr(float(v)) for v in goal.ravel()]
    for ff in (0, 1):
        out = str(tmp_path / ("on%d" % ff))
        res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), repr(radius), str(ff), str(max_len), str(lookahead)] + gs,
                             capture_output=True, text=True, timeout=120)
        wp, info, ln, ns = results[ff]
        assert res.returncode == 0 and "made 4 waypoints %d" % len(wp) in res.stdout, (res.stdout, res.stderr)
        assert np.fromfile(out + ".wp", np.uint8).tobytes() == wp.tobytes()
        got = np.fromfile(out + ".info", np.int32)
        assert got.tolist() == [int(info["count"]), int(info["forced"]), int(np.float32(info["length"]).view(np.int32)), ln, ns, csq]
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", repr(radius), "1", str(max_len), str(lookahead)] + gs, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 waypoints 2" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".wp", np.uint8).tobytes() == P5A * 48 and np.fromfile(out + ".info", np.int32).tolist() == [0, 0, 0, 0, 0, csq]

"""Path shortcutting on the device (include/gie.h gie_path_shortcut*) against the numpy statement of tests/path_ref.py.  The
reference works on read_local's type and edt taken at the same point of the mapper's stream; every comparison is of bytes: the
waypoint array including the entries beyond a path's records (prefilled with 0x5a), and the info records."""
import ctypes as C

import numpy as np
import pytest

import gie
import los_ref as lr
import nf1_ref
import path_cases as pc
import path_ref as pr
from gie import scenes
from stage_common import W, BoxDrive, bits, cv, mapper, probe, update, world

pytestmark = pytest.mark.gpu


def _settle(m, lab):
    """two updates of a label plane at the origin pose: (read_local, pivot); every labelled voxel has its type"""
    pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
    for _ in range(2):
        update(m, pos, q, lab)
    loc = m.read_local(dist_sq=False, coc=False)
    assert np.array_equal(loc["type"] == lr.OCCUPIED, lab == 2) and np.array_equal(loc["type"] == lr.UNKNOWN, lab == 0)
    return loc, np.array(m.pivot(), np.int64)


def _prefill(n, cap):
    return np.frombuffer(bytes([0x5a]) * (24 * n * cap), gie.WAYPOINT_DTYPE).reshape(n, cap).copy()


def _check(m, edt, opq, buf, lens, pvt, K, cap, legs=None):
    """the host form on a prefilled array against the statement, byte for byte; returns (wp, info, legs) of the statement"""
    n = buf.shape[0]
    legs = [] if legs is None else legs
    rwp, rinfo = pr.shortcut(edt, opq, buf, lens, pvt, K, cap, wp_init=_prefill(n, cap), legs=legs)
    wp, info = m.path_shortcut(buf, lens, K, cap, wp=_prefill(n, cap))
    assert wp.dtype == pr.WAYPOINT_DTYPE and info.dtype == pr.INFO_DTYPE
    for key in info.dtype.names:
        assert np.array_equal(bits(info[key]), bits(rinfo[key])), (K, cap, key, info[key], rinfo[key])
    for key in wp.dtype.names:
        assert np.array_equal(bits(wp[key]), bits(rwp[key])), (K, cap, key, int((bits(wp[key]) != bits(rwp[key])).sum()))
    assert wp.tobytes() == rwp.tobytes() and info.tobytes() == rinfo.tobytes()
    return rwp, rinfo, legs


# ---- the pillar scenes: answers in the second, third and fourth chunk of a window, with blocked indices below them
def test_pillar_scenes():
    chunks = []
    for long, ks in ((True, (200, 250, 280, 4096)), (False, (47, 64, 137, 1, 2, 63, 65, 127, 128, 129))):
        size, lab, path = pc.pillar_scene(long)
        m = mapper(size)
        try:
            loc, pvt = _settle(m, lab)
            assert m.los_prepare(0.0, 0) == int((lab == 2).sum())
            opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
            buf, lens = pc.pack([path], len(path), pvt)
            for K in ks:
                wp, info, legs = _check(m, loc["edt"], opq, buf, lens, pvt, K, len(path))
                chunks += pc.answer_chunks(legs)
                idx = wp["index"][0, :info["count"][0]].tolist()
                if long:
                    assert idx == [0, 113, 307], (K, idx)
                elif K in (47, 64, 137):
                    assert idx == {47: [0, 42, 89, 136, 137], 64: [0, 64, 128, 137], 137: [0, 113, 137]}[K], (K, idx)
                assert info["forced"][0] == 0 and info["length"][0] > 0
        finally:
            m.close()
    # (on the statement, not only on the device) every one of the first three chunks decides some window, and some answer has a
    # blocked index below it: "the last before the first failure" would not pass
    assert {0, 1, 2} <= {c for c, _ in chunks} and any(gap for _, gap in chunks), sorted({c for c, _ in chunks})


# ---- NF1 paths, handed on without leaving the device
NF1_SIZE = (36, 33, 20)


@pytest.mark.parametrize("max_len", [24, 96])
@pytest.mark.parametrize("clearance", [0.0, 0.15], ids=["clear0", "clear1.5"])
def test_nf1_paths_through_device_buffers(max_len, clearance):
    import torch
    rng = np.random.default_rng(1)
    lab = pc.random_boxes_labels(rng, NF1_SIZE, 14, 3, 9)
    free = np.argwhere(lab == 1)[:, ::-1]
    goal = free[rng.integers(0, len(free))]
    starts = rng.integers(0, NF1_SIZE, (64, 3))
    n = len(starts)
    m = mapper(NF1_SIZE)
    try:
        loc, pvt = _settle(m, lab)
        w = m.cfg.voxel_width
        hs = world(m, starts)
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        combos = [(K, cap) for K in (1, 7, 64, 1000) for cap in (0, 1, 3, 96)]
        out = {}
        with torch.cuda.stream(st):
            dg = torch.from_numpy(world(m, goal[None])).to(dev)
            m.nf1_compute_dev(dg.data_ptr(), 1, 0.0)                     # the field at clearance 0 whatever the plane's is
            ds = torch.from_numpy(hs).to(dev)
            dpath = torch.zeros((n, max_len, 3), dtype=torch.int32, device=dev)
            dlen = torch.zeros(n, dtype=torch.int32, device=dev)
            m.nf1_path_dev(ds.data_ptr(), n, max_len, dpath.data_ptr(), dlen.data_ptr())
            m.los_prepare_dev(clearance, 0)
            for K, cap in combos:
                dwp = torch.full((n * cap * 24 + 1,), 0x5a, dtype=torch.uint8, device=dev)
                dinfo = torch.full((n * 16,), 0x5a, dtype=torch.uint8, device=dev)
                m.path_shortcut_dev(dpath.data_ptr(), dlen.data_ptr(), n, max_len, dwp.data_ptr() if cap else 0, dinfo.data_ptr(), K, cap)
                out[K, cap] = (dwp, dinfo)
        m.sync()
        buf, lens = dpath.cpu().numpy(), dlen.cpu().numpy()
        tp = tuple(int(v) for v in pvt)
        f, _, _ = nf1_ref.field(loc["type"], loc["edt"], 0.0, 0, world(m, goal[None]), w, tp)
        pts, rl = nf1_ref.paths(f, hs, w, tp, max_len)
        assert np.array_equal(lens, rl) and all(np.array_equal(buf[i, :len(p)], p) for i, p in enumerate(pts))
        assert (lens > max_len).any() == (max_len == 24) and (lens == 0).any()
        opq = lr.opaque(loc["type"], loc["edt"], cv(m, clearance), 0)
        ms = np.clip(lens, 0, max_len)
        for K in (1, 7, 64, 1000):
            legs = []
            for cap in (0, 1, 3, 96):
                rwp, rinfo = pr.shortcut(loc["edt"], opq, buf, lens, pvt, K, cap, wp_init=_prefill(n, cap), legs=legs)
                dwp, dinfo = out[K, cap]
                gw = dwp.cpu().numpy()
                assert gw[:-1].tobytes() == rwp.tobytes() and gw[-1] == 0x5a, (K, cap)
                assert dinfo.cpu().numpy().tobytes() == rinfo.tobytes(), (K, cap)
            if K >= 64:                                                   # what the scene has to give, on the statement
                ch = pc.answer_chunks(legs)
                assert ((rinfo["count"] * 2 < ms) & (ms > 0)).sum() >= n // 10 + 1 and (rinfo["count"] >= 3).sum() >= n // 10 + 1
                assert any(gap for _, gap in ch)
            assert (rinfo["forced"].sum() > 0) == (clearance > 0), (K, int(rinfo["forced"].sum()))
        # the host form on the same buffers: the same bytes
        hwp, hinfo = m.path_shortcut(buf, lens, 64, 96, wp=_prefill(n, 96))
        assert hwp.tobytes() == out[64, 96][0].cpu().numpy()[:-1].tobytes() and hinfo.tobytes() == out[64, 96][1].cpu().numpy().tobytes()
    finally:
        m.close()


# ---- arbitrary polylines
def test_arbitrary_polylines():
    size, max_len, n = (33, 31, 29), 70, 37                               # 37 paths: the last workgroup has one wave
    rng = np.random.default_rng(7)
    lab = pc.random_boxes_labels(rng, size, 12, 3, 9)
    m = mapper(size)
    try:
        loc, pvt = _settle(m, lab)
        m.los_prepare(0.0, 0)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        paths = pc.polylines(rng, size, n, max_len)
        buf, lens = pc.pack(paths, max_len, pvt, fill=77)
        lens[7] = -3
        assert {-3, 0, 1, 2, 69, 70, 71, 500} <= set(lens.tolist()) and len(lens) == n
        ext = [(pc.INT_MAX, pc.INT_MAX, pc.INT_MAX), (pc.INT_MIN, pc.INT_MIN, pc.INT_MIN), (pc.INT_MAX, pc.INT_MIN, 0), (pc.INT_MIN, 5, pc.INT_MAX)]
        for t, e in enumerate(ext):                                       # the four int32 extremes, in the middle of long paths
            buf[3 + t, 10 + 7 * t] = e
            buf[10 + t, 0] = e                                            # ... and as a first point
        outside = ~pr.local(buf, pvt, size)[1]
        assert outside[np.arange(max_len)[None, :] < np.clip(lens, 0, max_len)[:, None]].sum() >= 20
        nforced = 0
        for K, cap in ((1, 70), (3, 4), (64, 70), (100, 70), (4096, 1)):
            _, info, _ = _check(m, loc["edt"], opq, buf, lens, pvt, K, cap)
            nforced += int(info["forced"].sum())
            assert info["count"][lens <= 0].tolist() == [0, 0]
        assert nforced >= 50
        _check(m, loc["edt"], opq, buf[5:6], lens[5:6], pvt, 64, 70)      # n = 1
        wp, info = m.path_shortcut(np.zeros((0, max_len, 3), np.int32), np.zeros(0, np.int32), 64, 70)      # n = 0
        assert wp.shape == (0, 70) and info.shape == (0,)
    finally:
        m.close()


# ---- a line as long as a volume can be
@pytest.mark.parametrize("blocked", [False, True], ids=["free", "one_opaque_voxel"])
def test_axis_of_1024_voxels(blocked):
    size = (1024, 3, 3)
    lab = np.ones(size[::-1], np.int8)
    if blocked:
        lab[1, 1, 511] = 2
    path = np.array([(x, 1, 1) for x in range(1024)], np.int64)
    m = mapper(size)
    try:
        loc, pvt = _settle(m, lab)
        m.los_prepare(0.0, 0)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        buf, lens = pc.pack([path], 1024, pvt)
        wp, info, _ = _check(m, loc["edt"], opq, buf, lens, pvt, 4096, 8)
        idx = wp["index"][0, :info["count"][0]].tolist()
        if blocked:
            assert idx == [0, 510, 511, 512, 1023] and info["forced"][0] == 2 and wp["forced"][0, :5].tolist() == [0, 0, 1, 1, 0]
            assert info["length"][0] == np.float32(510.0) + np.float32(511.0)
        else:
            assert idx == [0, 1023] and info["forced"][0] == 0
            assert bits(info["length"])[:4].tobytes() == np.float32(1023.0).tobytes()
    finally:
        m.close()


# ---- a never-observed region under GIE_LOS_UNKNOWN_OPAQUE: every leg forced, without a walk
def test_unknown_opaque_region():
    size = (40, 32, 16)
    lab = np.ones(size[::-1], np.int8)
    lab[:, :, :20] = 0
    m = mapper(size)
    try:
        loc, pvt = _settle(m, lab)
        m.los_prepare(0.0, gie.LOS_UNKNOWN_OPAQUE)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, gie.LOS_UNKNOWN_OPAQUE)
        inside = pc.staircase(30, (2, 3, 2))                              # wholly in the never-seen slab
        assert inside[:, 0].max() < 20
        leaving = np.array([(x, 10, 8) for x in range(8, 36)], np.int64)  # out of it into free space
        buf, lens = pc.pack([inside, leaving], 32, pvt)
        for K in (1, 9, 64):
            wp, info, _ = _check(m, loc["edt"], opq, buf, lens, pvt, K, 32)
            assert info["count"][0] == 30 and info["forced"][0] == 29 and info["length"][0] == 0
            assert (wp["forced"][0, 1:30] == 1).all() and (wp["min_edt"][0, 1:30] == -1).all()
            assert 12 <= info["forced"][1] < 27 and info["length"][1] > 0
        m.los_prepare(0.0, 0)                                             # without the flag the slab is see-through
        _, info, _ = _check(m, loc["edt"], lr.opaque(loc["type"], loc["edt"], 0.0, 0), buf, lens, pvt, 64, 32)
        assert info["forced"].tolist() == [0, 0] and info["count"].tolist() == [2, 2]
    finally:
        m.close()


# ---- life cycle
def _drive_paths(rng, size, n, max_len):
    """polylines of short hops that start near the low-x face (what a drive along +x leaves behind first), and random ones"""
    paths = pc.polylines(rng, size, n // 2, max_len)
    for _ in range(n - n // 2):
        p = np.zeros((max_len, 3), np.int64)
        cur = np.array([rng.integers(0, 6), rng.integers(0, size[1]), rng.integers(0, size[2])])
        for t in range(max_len):
            p[t] = cur
            cur = np.clip(cur + rng.integers(-1, 3, 3), 0, np.array(size) - 1)
        paths.append(p)
    return paths


def test_life_cycle_over_a_drive():
    import torch
    size, max_len, n, K, cap = (64, 48, 40), 40, 24, 25, 12
    d = BoxDrive(size, seed=6)
    m, twin = mapper(size), mapper(size)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        old = None
        left = 0
        for k in range(5):
            pos, q, lab = d.frame(k)
            for mm in (m, twin):
                update(mm, pos, q, lab)
            loc = m.read_local(dist_sq=False, coc=False)
            pvt = np.array(m.pivot(), np.int64)
            cl = 0.1 if k % 2 else 0.0
            m.los_prepare(cl, 0)
            opq = lr.opaque(loc["type"], loc["edt"], cv(m, cl), 0)
            buf, lens = pc.pack(_drive_paths(np.random.default_rng(k), size, n, max_len), max_len, pvt)
            rwp, rinfo, _ = _check(m, loc["edt"], opq, buf, lens, pvt, K, cap)           # the host form
            with torch.cuda.stream(st):                                                   # the _dev form: the same bytes
                dp, dl = torch.from_numpy(buf).to(dev), torch.from_numpy(lens).to(dev)
                dwp = torch.from_numpy(_prefill(n, cap).view(np.uint8)).to(dev)
                dinfo = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
                m.path_shortcut_dev(dp.data_ptr(), dl.data_ptr(), n, max_len, dwp.data_ptr(), dinfo.data_ptr(), K, cap)
            m.sync()
            assert dwp.cpu().numpy().tobytes() == rwp.tobytes() and dinfo.cpu().numpy().tobytes() == rinfo.tobytes(), k
            if old is not None:                                           # update k - 1's paths on this prepare: points have left
                obuf, olens = old
                real = np.arange(max_len)[None, :] < np.clip(olens, 0, max_len)[:, None]
                left += int((pr.local(obuf, old_pvt, size)[1] & ~pr.local(obuf, pvt, size)[1] & real).sum())
                _check(m, loc["edt"], opq, obuf, olens, pvt, K, cap)
            old, old_pvt = (buf, lens), pvt
            lt = twin.read_local(dist_sq=False, coc=False)                # the twin that never calls the feature
            for key in loc:
                assert np.array_equal(loc[key], lt[key]), (k, key)
            assert m.stats() == twin.stats(), k
            assert np.array_equal(probe(m, size, np.random.default_rng(k)), probe(twin, size, np.random.default_rng(k))), k
        assert left >= 1, left
        # three further updates without a new prepare: the same bytes for the same paths, whatever the map does
        first = m.path_shortcut(buf, lens, K, cap, wp=_prefill(n, cap))
        pv = m.pivot()
        for k in range(5, 8):
            pos, q, lab = d.frame(k)
            update(m, pos, q, lab)
            again = m.path_shortcut(buf, lens, K, cap, wp=_prefill(n, cap))
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes(), k
        assert m.pivot() != pv
        assert first[0].tobytes() == rwp.tobytes() and first[1].tobytes() == rinfo.tobytes()
        # the launch counts under "los_query"
        m.profile_enable(True)
        m.path_shortcut(buf, lens, K, cap)
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["los_query"][1] == 1 and prof["los_query"][0] > 0
    finally:
        m.close()
        twin.close()


def test_refusals():
    size = (32, 32, 16)
    m, t = mapper(size), mapper(size)
    try:
        f, h = m._f, m._h
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
        path = np.zeros((4, 8, 3), np.int32)
        lens = np.full(4, 8, np.int32)
        wp = np.zeros((4, 5), gie.WAYPOINT_DTYPE)
        info = np.zeros(4, gie.SHORTCUT_INFO_DTYPE)
        good = m.shortcut_param(4, 5)

        def both(hh, pa, ln, n, max_len, p, w, i):
            p = None if p is None else C.byref(p)
            w, i, pa, ln = (None if a is None else ptr(a) for a in (w, i, pa, ln))
            return [f["path_shortcut"](hh, pa, ln, n, max_len, p, w, i), f["path_shortcut_dev"](hh, pa, ln, n, max_len, p, w, i)]
        assert both(h, path, lens, 4, 8, good, wp, info) == [1, 1]       # before the first prepare
        pos, q = scenes.pose(0, W, delta_vox=0, yaw_deg=0.0)
        for mm in (m, t):
            update(mm, pos, q, np.ones(size[::-1], np.int8))
        m.los_prepare(0.0, 0)
        assert f["path_shortcut"](h, ptr(path), ptr(lens), 4, 8, C.byref(good), ptr(wp), ptr(info)) == 0
        assert f["path_shortcut"](None, ptr(path), ptr(lens), 4, 8, C.byref(good), ptr(wp), ptr(info)) == 1
        assert both(h, path, lens, 4, 8, None, wp, info) == [1, 1]       # a NULL param
        for look in (0, -1, 4097, pc.INT_MIN):                            # lookahead outside 1..4096
            assert both(h, path, lens, 4, 8, m.shortcut_param(look, 5), wp, info) == [1, 1]
        assert f["path_shortcut"](h, ptr(path), ptr(lens), 4, 8, C.byref(m.shortcut_param(4096, 5)), ptr(wp), ptr(info)) == 0
        assert both(h, path, lens, 4, 8, m.shortcut_param(4, -1), wp, info) == [1, 1]        # max_wp < 0
        assert both(h, path, lens, -1, 8, good, wp, info) == [1, 1]      # n < 0
        assert both(h, path, lens, 4, 0, good, wp, info) == [1, 1]       # with n > 0: max_len < 1 ...
        assert both(h, None, lens, 4, 8, good, wp, info) == [1, 1] and both(h, path, None, 4, 8, good, wp, info) == [1, 1]   # ... NULL inputs
        assert both(h, path, lens, 4, 8, good, None, info) == [1, 1]     # wp NULL while max_wp > 0
        assert both(h, path, lens, 4, 8, m.shortcut_param(4, 0), None, None) == [1, 1]       # wp and info both NULL
        # what is valid: no info; no waypoints with max_wp == 0; n == 0 with nothing else
        assert f["path_shortcut"](h, ptr(path), ptr(lens), 4, 8, C.byref(good), ptr(wp), None) == 0
        assert f["path_shortcut"](h, ptr(path), ptr(lens), 4, 8, C.byref(m.shortcut_param(4, 0)), None, ptr(info)) == 0
        assert (info["count"] >= 2).all() and (info["reserved"] == 0).all()
        assert both(h, None, None, 0, 0, good, wp, info) == [0, 0] and both(h, None, None, 0, 8, good, wp, None) == [0, 0]
        # a tiled mapper
        t.set_tile((8, 0, 0), (64, 32, 16))
        assert both(t._h, path, lens, 4, 8, good, wp, info) == [1, 1]
    finally:
        m.close()
        t.close()

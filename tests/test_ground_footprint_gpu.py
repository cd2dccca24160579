"""Ground footprints on the device (include/gie.h "ground footprints", gie_ground_footprint.inc.h) against the numpy statement of
tests/ground_footprint_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is of bytes."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import gie
import ground_footprint_ref as P
import ground_ref as R
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, ground as _ground, xy as _xy, open_cells as _open, same as _same, arc as _arc, scene
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries of a mapper without frontier clusters
FD = gie.GROUND_FOOTPRINT_DTYPE
SMALL, LONG = (9, 1, 4), (1600, 4, 9)                           # (front_sq, back_sq, side_sq): 3 ahead, 1 behind, 2 aside; 40 ahead: three words at (1, 0)
FLAG_PAIRS = ((False, False), (True, True), (False, True), (True, False))      # (unknown traversable, margin)
RULES = [(e, c) for c, e in itertools.product((0, 1, 9), (SMALL, LONG))]       # a rectangle and a clearance_sq
COMBOS = [(e, c, u, mg) for (e, c), (u, mg) in itertools.product(RULES, FLAG_PAIRS)]      # the 24 combinations


def _flags(unknown, margin):
    return (P.UNKNOWN_TRAVERSABLE if unknown else 0) | (P.MARGIN if margin else 0)


def _both_forms(m, st, xy, hd, e, c, u, mg, want, what):
    """the host form and the _dev form over a buffer one record longer, with a poisoned tail: the reference's bytes, nothing beyond"""
    import torch
    n, T = xy.shape[0], xy.shape[1]
    got = m.ground_footprints(xy, hd, e[0], e[1], e[2], c, u, mg)
    assert got.dtype == FD
    _same(got, want, what)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(st):
        dxy = torch.from_numpy(xy).to(dev)
        dhd = torch.from_numpy(hd).to(dev)
        dout = torch.full(((n + 1) * 32,), 0x5a, dtype=torch.uint8, device=dev)
        m.ground_footprints_dev(dxy.data_ptr(), dhd.data_ptr(), n, T, dout.data_ptr(), e[0], e[1], e[2], c, u, mg)
    m.sync()
    o = dout.cpu().numpy()
    assert o[:n * 32].tobytes() == want.tobytes() and o[n * 32:].tobytes() == P5A * 32, what
    return got


def _fan(g, size, T, rng, n=13):
    """n trajectories of T poses: straight lines and arcs from open cells, small circles in the most open places (the long clear ones), a
    run along x over the word boundaries, one towards and over the field's border, and (the thirteenth) a wait with four last steps towards an obstacle"""
    X, Y = size[0], size[1]
    d = np.asarray(g["dist_sq"])
    free = np.argwhere(_open(g))[:, ::-1]
    inner = free[(free[:, 0] >= 6) & (free[:, 0] < X - 6) & (free[:, 1] >= 6) & (free[:, 1] < Y - 6)]
    far = inner[np.argsort(-d[inner[:, 1], inner[:, 0]], kind="stable")[:6]]
    xs, hs = [], []
    for j in range(n):
        kind = j % 6
        if j == 12:                                             # wait in the most open place, then four steps of a cell straight at its nearest obstacle
            occ = np.argwhere(np.asarray(g["type"]) == R.OCCUPIED)[:, ::-1]          # column: dist_sq falls with the last poses, the margin is attained last
            to = (occ[np.argmin(((occ - far[0]) ** 2).sum(1))] - far[0]).astype(np.float64)
            th = np.arctan2(to[1], to[0])
            a = (far[0] + np.maximum(np.arange(T) - (T - 5), 0)[:, None] * np.array([np.cos(th), np.sin(th)]), _arc(far[0], th, 0.0, 0.0, T)[1])
        elif kind == 0:
            a = _arc(free[rng.integers(len(free))] + rng.uniform(-0.4, 0.4, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1.0), 0.0, T)
        elif kind == 1:
            a = _arc(free[rng.integers(len(free))] + rng.uniform(-0.4, 0.4, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1.0), rng.uniform(-0.2, 0.2), T)
        elif kind in (2, 3):                                    # a small circle in an open place
            a = _arc(far[(j // 6 + kind) % len(far)], rng.uniform(0, 2 * np.pi), 0.25, rng.choice([-1, 1]) * rng.uniform(0.15, 0.5), T)
        elif kind == 4:                                         # along x over a word boundary of the bit plane
            x0 = [max(64 - T // 2, 4), max(128 - T // 2, 4)][(j // 6) % 2]
            a = _arc((min(x0, X - 6), int(far[0][1])), 0.0, 1.0, 0.0, T)
        else:                                                   # out of the field over its nearest border
            s = far[(j // 6) % len(far)].astype(np.float64)
            a = _arc(s, [np.pi / 2, -np.pi / 2][int(s[1] < Y / 2)] + rng.uniform(-0.3, 0.3), 1.0, 0.0, T)
        xs.append(a[0])
        hs.append(a[1])
    return np.stack(xs), np.ascontiguousarray(np.stack(hs))


# ---------------------------------------------------------------------------------------------------------- 1. the sweep
def _sweep_cases(g, pvt, size):
    """(T, n, xy, headings, (extents, clearance_sq, unknown, margin), the reference's records): T in {1, 5, 64, 65, 130} x n in {1, 5, 13}, and for
    each of these 15 all FOUR flag pairs, with a rectangle and a clearance_sq that change from one (T, n) to the next: 60 calls, every
    one of the 24 combinations at least twice, every flag pair at every T"""
    rng = np.random.default_rng(size[0])
    group = 0
    for T in (1, 5, 64, 65, 130):
        cells, hd_all = _fan(g, size, T, rng)
        xy_all = _xy(pvt, cells)
        if T > 1:
            xy_all[1, T // 2:] = np.nan                         # a NaN tail
            hd_all[7, T - 1] = 0                                # a zero-heading tail
        for n in (1, 5, 13):
            xy, hd = np.ascontiguousarray(xy_all[:n]), np.ascontiguousarray(hd_all[:n])
            e, c = RULES[group % len(RULES)]
            group += 1
            for u, mg in FLAG_PAIRS:
                yield T, n, xy, hd, (e, c, u, mg), P.footprints(g, xy, hd, pvt, W, e[0], e[1], e[2], c, _flags(u, mg))


def _sweep_conditions(cases, pvt, shape):
    """no case passes vacuously, all of it from the reference's records: every combination has run, and every flag pair at every T;
    every ending occurs, the complete and the blocked ones a tenth each; a prefix beyond one chunk of poses; a hit outside the
    rectangle; margins that are not trivial, with and without the UNKNOWN flag one attained in the SECOND chunk of poses
    (min_at >= 64) and one in the third (>= 128)"""
    Y, X = shape
    ends, longest, outside, margins, late = [], 0, 0, set(), {False: 0, True: 0}
    for T, n, xy, hd, (e, c, u, mg), want in cases:
        ends += want["end"].tolist()
        longest = max(longest, int(want["poses"].max()))
        h = want["hit"][want["end"] == 1] - np.array(pvt[:2])
        outside += int(((h[:, 0] < 0) | (h[:, 0] >= X) | (h[:, 1] < 0) | (h[:, 1] >= Y)).sum())
        if mg:
            margins |= set(want["min_at"][want["min_at"] > 0].tolist())
            late[u] = max(late[u], int(want["min_at"].max()))
        else:
            assert (want["min_at"] == -2).all() and (want["min_dist_sq"] == -2).all()
    cnt = [ends.count(e) for e in (0, 1, 2)]
    print("trajectories %d: complete %d blocked %d no placement %d; hits outside %d; longest prefix %d; distinct min_at > 0: %d; the latest min_at %s" %
          (len(ends), cnt[0], cnt[1], cnt[2], outside, longest, len(margins), late))
    assert {combo for T, n, xy, hd, combo, want in cases} == set(COMBOS)
    for T in (1, 5, 64, 65, 130):
        assert {combo[2:] for T_, n, xy, hd, combo, want in cases if T_ == T} == set(FLAG_PAIRS), T
    assert cnt[0] * 10 >= len(ends) and cnt[1] * 10 >= len(ends) and cnt[2] >= 1
    assert outside >= 1 and longest > 64 and len(margins) >= 3
    assert min(late.values()) >= 64 and max(late.values()) >= 128 and any(64 <= v < 128 for v in margins)


@pytest.mark.parametrize("size", [(70, 40, 4), (130, 48, 4)])
def test_footprints_equal_the_reference(size):
    import torch
    pos, lab = scene(size, 300 + size[0], n_boxes=7, unknown_slab=3, smax=7)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        t = np.asarray(g["type"])
        assert (t == R.UNKNOWN).any() and (t == R.OCCUPIED).any() and _open(g).sum() > 100
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        cases = list(_sweep_cases(g, pvt, size))
        for T, n, xy, hd, (e, c, u, mg), want in cases:
            _both_forms(m, st, xy, hd, e, c, u, mg, want, (size, T, n, e, c, u, mg))
        _sweep_conditions(cases, pvt, t.shape)
        assert len(m.ground_footprints(np.zeros((0, 5, 2), np.float32), np.zeros((0, 5, 2), np.int32), 1, 1, 1)) == 0      # n == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. pinned poses
HEADS = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (32767, 1), (1, -32767), (0, 0), (40000, 0)]


@pytest.mark.parametrize("size", [(70, 40, 4), (130, 48, 4)])
def test_pinned_poses_on_the_borders_and_word_boundaries(size):
    import torch
    X, Y = size[0], size[1]
    pos, lab = scene(size, 300 + size[0], n_boxes=7, unknown_slab=3, smax=7)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))
        centres = [(x, y) for y in (0, Y // 2, Y - 1) for x in (0, 63, 64, X - 1)]
        cells = np.array([c for c in centres for _ in HEADS], np.float64)[:, None, :]          # T = 1: a trajectory per pose
        hd = np.ascontiguousarray(np.array([h for _ in centres for h in HEADS], np.int32)[:, None, :])
        xy = _xy(pvt, cells)
        seen = set()
        for e in ((0, 0, 0), (25, 4, 9), (P.MAX_SQ, P.MAX_SQ, P.MAX_SQ), (P.MAX_SQ, 0, 1)):       # at the cap the footprint covers the whole field and more
            for c, u, mg in ((0, False, True), (0, True, True), (9, True, False), (1, False, False))[:2 if e[2] == P.MAX_SQ else 4]:
                want = P.footprints(g, xy, hd, pvt, W, e[0], e[1], e[2], c, _flags(u, mg))
                _both_forms(m, st, xy, hd, e, c, u, mg, want, (size, e, c, u, mg))
                seen |= set(want["end"].tolist())
                bad = [i for i, h in enumerate(hd[:, 0].tolist()) if tuple(h) in ((0, 0), (40000, 0))]
                assert (want["end"][bad] == 2).all() and len(bad) == 2 * len(centres)
                if e[2] == P.MAX_SQ and not u:                  # the rows above or below the field come first in (y, x)
                    ok = want["end"] == 1
                    assert ok.sum() == len(want) - len(bad) and (want["hit_cells"][ok] > X * Y // 4).any()
        assert seen == {0, 1, 2}
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. against the rollouts
def test_zero_extents_agree_with_the_rollouts_on_the_same_poses():
    size = (70, 40, 4)
    pos, lab = scene(size, 370, n_boxes=7, unknown_slab=3, smax=7)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        _ground(m, size)
        rng = np.random.default_rng(5)
        cells = np.stack([rng.integers(-2, size[0] + 2, 400), rng.integers(-2, size[1] + 2, 400)], 1)[:, None, :]
        xy = _xy(pvt, cells)
        hd = np.ascontiguousarray(np.broadcast_to(np.array([3, -4], np.int32), (400, 1, 2)))
        for c, u in ((0, False), (4, False), (1, True)):
            got = m.ground_footprints(xy, hd, 0, 0, 0, c, u, True)
            ro = m.ground_rollouts(xy, c, 0, u)
            for key in ("end", "poses", "hit", "min_dist_sq"):
                assert np.array_equal(got[key], ro[key]), (c, u, key)
            assert np.array_equal(got["hit_cells"], (ro["end"] == 1).astype(np.int32)) and np.array_equal(got["min_at"], ro["poses"] - 1)
            assert len(set(got["end"].tolist())) == 3
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. the mask
def test_mask_equals_the_reference_and_keeps_the_record():
    import torch
    size = (70, 40, 4)
    pos, lab = scene(size, 370, n_boxes=7, unknown_slab=3, smax=7)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        ends = set()
        for cell, h, e, c, u, mg in (((30, 20), (3, 1), (100, 16, 25), 0, False, True), ((64, 3), (-1, 1), (1600, 4, 9), 1, True, True),
                                     ((0, 39), (0, -1), (49, 49, 4), 0, True, False), ((69, 0), (32767, 1), LONG, 9, False, False),
                                     ((35, 20), (1, 2), (P.MAX_SQ, P.MAX_SQ, P.MAX_SQ), 0, True, True), ((35, 20), (0, 0), SMALL, 0, False, True),
                                     ((80, 20), (1, 0), SMALL, 0, False, False)):
            xy, hd = _xy(pvt, [cell])[0], np.array(h, np.int32)
            want, wrec = P.mask(g, xy, hd, pvt, W, e[0], e[1], e[2], c, _flags(u, mg))
            got, rec = m.ground_footprint_mask(xy, hd, e[0], e[1], e[2], c, u, mg)
            one = m.ground_footprints(xy.reshape(1, 1, 2), hd.reshape(1, 1, 2), e[0], e[1], e[2], c, u, mg)
            assert np.array_equal(got, want) and rec.tobytes() == wrec.tobytes() == one.tobytes(), (cell, h, e)
            ends.add(int(wrec["end"]))
            with torch.cuda.stream(st):
                dxy, dhd = torch.from_numpy(xy).to(dev), torch.from_numpy(hd).to(dev)
                dmask = torch.full((70 * 40 + 16,), 0x5a, dtype=torch.uint8, device=dev)
                drec = torch.full((64,), 0x5a, dtype=torch.uint8, device=dev)
                m.ground_footprint_mask_dev(dxy.data_ptr(), dhd.data_ptr(), dmask.data_ptr(), drec.data_ptr(), e[0], e[1], e[2], c, u, mg)
                m.ground_footprint_mask_dev(dxy.data_ptr(), dhd.data_ptr(), dmask.data_ptr(), 0, e[0], e[1], e[2], c, u, mg)      # rec may be NULL
            m.sync()
            o, r = dmask.cpu().numpy(), drec.cpu().numpy()
            assert o[:2800].tobytes() == want.tobytes() and o[2800:].tobytes() == P5A * 16 and r[:32].tobytes() == wrec.tobytes() and r[32:].tobytes() == P5A * 32
        assert ends == {0, 1, 2}
    finally:
        m.close()


def test_a_quarter_turn_turns_the_mask_on_a_square_field():
    size = (48, 48, 4)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((4, 48, 48), np.int8))
        _ground(m, size)
        c = (24, 24)                                            # a turn about c maps (x, y) to (c - (y - c), c + (x - c)) = (48 - y, x): rows and columns 1 .. 47
        for h in ((1, 0), (3, 1), (-2, 5), (32767, 1), (1, 1)):
            for e in ((100, 16, 25), (400, 0, 9), (7, 5, 3)):
                a, _ = m.ground_footprint_mask(_xy(pvt, [c])[0], h, e[0], e[1], e[2], 0, True)
                b, _ = m.ground_footprint_mask(_xy(pvt, [c])[0], (-h[1], h[0]), e[0], e[1], e[2], 0, True)
                assert a.sum() > 0 and not a[0].any() and not a[:, 0].any() and not b[0].any() and not b[:, 0].any()
                ys, xs = np.nonzero(a)
                turned = np.zeros_like(a)
                turned[xs, 48 - ys] = a[ys, xs]
                assert np.array_equal(b, turned), (h, e)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, t = _mapper(size), _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        f = m._f
        n, T = 4, 3
        host = np.frombuffer(P5A * 4096, np.uint8).copy()
        dbuf = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [[(3, 3), (4, 4), (5, 5)], [(9, 9), (9, 10), (9, 11)], [(20, 4), (21, 4), (22, 4)], [(1, 1), (1, 1), (1, 1)]])
        hd = np.ascontiguousarray(np.broadcast_to(np.array([1, 1], np.int32), (n, T, 2)))
        dxy, dhd = torch.from_numpy(xy).to("cuda:0"), torch.from_numpy(hd).to("cuda:0")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())

        def FP(**kw):
            p = _capi.GroundFootprintParam(1, 1, 1, 0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert host.tobytes() == P5A * host.size and bool((dbuf == 0x5a).all())

        def refused(h, who, p="default", n_=n, T_=T, a=True, b=True, out=True, masks=True):
            p = FP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_footprints"](h, ptr(xy) if a else None, ptr(hd) if b else None, n_, T_, pr, ptr(host) if out else None) == INVALID, who
            assert f["ground_footprints_dev"](h, C.c_void_p(dxy.data_ptr()) if a else None, C.c_void_p(dhd.data_ptr()) if b else None, n_, T_, pr,
                                              dp if out else None) == INVALID, who
            if masks:                                            # (n and T are not arguments of the mask forms; a NULL out is their NULL mask)
                assert f["ground_footprint_mask"](h, ptr(xy) if a else None, ptr(hd) if b else None, pr, ptr(host) if out else None, ptr(host[2048:])) == INVALID, who
                assert f["ground_footprint_mask_dev"](h, C.c_void_p(dxy.data_ptr()) if a else None, C.c_void_p(dhd.data_ptr()) if b else None, pr,
                                                      dp if out else None, C.c_void_p(dbuf.data_ptr() + 2048)) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            refused(h, who)
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper
        refused(t._h, "tiled")
        unwritten()
        z = pvt[2]
        m.ground_compute(z, z + 7)
        refused(m._h, "null param", None)
        big = P.MAX_SQ + 1
        bad = [FP(front_sq=-1), FP(front_sq=big), FP(back_sq=-1), FP(back_sq=big), FP(side_sq=-1), FP(side_sq=big), FP(side_sq=2 ** 31 - 1), FP(front_sq=-2 ** 31),
               FP(clearance_sq=-1), FP(clearance_sq=-2 ** 31), FP(flags=4), FP(flags=7), FP(flags=-2 ** 31), FP(flags=8)] + [FP(reserved=i) for i in range(3)]
        for p in bad:
            refused(m._h, (p.front_sq, p.back_sq, p.side_sq, p.clearance_sq, p.flags, list(p.reserved)), p)
        refused(m._h, "n < 0", n_=-1, masks=False)
        for bad_T in (0, -1, 4097, 2 ** 31 - 1):
            refused(m._h, "T", T_=bad_T, masks=False)
            refused(m._h, "T with n == 0", n_=0, T_=bad_T, masks=False)
        refused(m._h, "null xy", a=False)
        refused(m._h, "null heading", b=False)
        refused(m._h, "null out / null mask", out=False)
        unwritten()
        # (the same calls with good arguments work; n == 0 is valid with NULL arrays and writes nothing)
        assert f["ground_footprints"](m._h, None, None, 0, 1, C.byref(FP()), None) == 0 and f["ground_footprints_dev"](m._h, None, None, 0, 4096, C.byref(FP()), None) == 0
        unwritten()
        assert f["ground_footprints"](m._h, ptr(xy), ptr(hd), n, T, C.byref(FP(front_sq=P.MAX_SQ, flags=3)), ptr(host)) == 0
        rec = host[:32 * n].view(FD)
        assert rec["poses"].tolist() == [3] * 4 and rec["end"].tolist() == [0] * 4 and rec["min_dist_sq"].tolist() == [-1] * 4 and rec["min_at"].tolist() == [0] * 4
        assert host[32 * n:].tobytes() == P5A * (4096 - 32 * n)
        assert f["ground_footprints"](m._h, ptr(xy), ptr(hd), n, T, C.byref(FP(front_sq=P.MAX_SQ)), ptr(host)) == 0           # without the flag the outside blocks
        assert rec["poses"].tolist() == [0] * 4 and rec["end"].tolist() == [1] * 4 and rec["min_at"].tolist() == [-2] * 4
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 6. state
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
        cells, hd = _fan(g0, size, 20, np.random.default_rng(2), n=24)
        xy = _xy(pvt0, cells)
        r0 = m.ground_footprints(xy, hd, 9, 1, 4, 0, False, True)
        _same(r0, P.footprints(g0, xy, hd, pvt0, W, 9, 1, 4, 0, P.MARGIN), "before")
        assert len(set(r0["end"].tolist())) >= 2
        g0b = m.read_ground()
        assert all(np.array_equal(g0[k], g0b[k]) for k in g0)   # the calls wrote nothing of the ground field
        pvt1 = step(1)                                          # a map update between two calls changes no result
        assert tuple(pvt1) != tuple(pvt0)
        assert m.ground_footprints(xy, hd, 9, 1, 4, 0, False, True).tobytes() == r0.tobytes()
        g1 = _ground(m, size)                                   # a new ground field does: the next call sees it, at its pivot
        r1 = m.ground_footprints(xy, hd, 9, 1, 4, 0, False, True)
        _same(r1, P.footprints(g1, xy, hd, pvt1, W, 9, 1, 4, 0, P.MARGIN), "after")
        assert r1.tobytes() != r0.tobytes()
    finally:
        m.close()


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
        if phase == "fuse" and k % 2 == 0:                       # a new ground field and function every other frame, between fuse and merge
            field["pvt"] = scenes.local_pivot(pos, W, size)
            a.ground_compute(field["pvt"][2] + 2, field["pvt"][2] + 9, 2, k % 4 == 2)
            a.ground_nf1_compute(_xy(field["pvt"], [(24, 20)]), 0, True)
            field["nf"] = a.read_ground_nf1()
        if phase in ("fuse", "edt", "merge"):
            r = np.random.default_rng(k)
            arcs = [_arc(r.uniform(0, 40, 2), r.uniform(0, 6.28), r.uniform(0.3, 2.0), 0.05, 70) for _ in range(30)]
            xy, hd = _xy(field["pvt"], np.stack([p for p, _ in arcs])), np.ascontiguousarray(np.stack([h for _, h in arcs]))
            a.ground_footprints(xy, hd, 25, 4, 9, k % 3, k % 2 == 0, True)
            a.ground_footprint_mask(xy[0, 0], hd[0, 0], 25, 4, 9, k % 3, k % 2 == 0, True)
            assert np.array_equal(a.read_ground_nf1(), field["nf"])                   # nor of the ground navigation function

    stage_calls_change_nothing(size, (frame(k) for k in range(5)), _mapper, calls, n_probe=2000)


# ---------------------------------------------------------------------------------------------------------- 7. launches and profile
def test_profile_counts_under_ground_query():
    import torch
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.profile_enable(True)
        m.profile_read()
        xy = _xy(pvt, [[(3, 3), (20, 9)], [(5, 5), (6, 6)]])
        hd = np.ones((2, 2, 2), np.int32)
        m.ground_footprints(xy, hd, 4, 4, 4)
        prof = m.profile_read()
        assert prof["ground_query"][1] == 1 and prof["ground_query"][0] > 0
        m.ground_footprints(xy, hd, 4, 4, 4, 1, True, True)
        d = torch.zeros((256,), dtype=torch.uint8, device="cuda:0")
        dxy, dhd = torch.from_numpy(xy).to("cuda:0"), torch.from_numpy(hd).to("cuda:0")
        m.ground_footprints_dev(dxy.data_ptr(), dhd.data_ptr(), 2, 2, d.data_ptr(), 4, 4, 4)
        m.ground_footprint_mask(xy[0, 0], hd[0, 0], 4, 4, 4)
        m.ground_footprints(np.zeros((0, 2, 2), np.float32), np.zeros((0, 2, 2), np.int32), 4, 4, 4)        # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_query"][1] == 3 and prof["ground_query"][0] > 0
        assert all(v[1] == 0 for k, v in prof.items() if k != "ground_query")
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
xy = ((np.array([[(8, 8), (9, 9), (10, 9)], [(15, 15), (16, 16), (17, 17)]], np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(0.1)).astype(np.float32)
hd = np.ones((2, 3, 2), np.int32)
for margin in (False, True):
    sys.stderr.write("BEGIN\n"); sys.stderr.flush()
    r = m.ground_footprints(xy, hd, 9, 1, 4, 1, False, margin)
    sys.stderr.write("END\n"); sys.stderr.flush()
    assert r["poses"].tolist() == [3, 3]
sys.stderr.write("BEGIN\n"); sys.stderr.flush()
mask, rec = m.ground_footprint_mask(xy[0, 0], hd[0, 0], 9, 1, 4)
sys.stderr.write("END\n"); sys.stderr.flush()
assert rec["poses"] == 1 and mask.sum() > 0
sys.stderr.write("BEGIN\n"); sys.stderr.flush()
m.ground_footprints(xy[:0], hd[:0], 9, 1, 4)
sys.stderr.write("END\n"); sys.stderr.flush()
m.close()
"""


def test_a_call_is_two_launches():
    """the launches themselves, named by the test build's launch trace (a switch read once per process: a child process)"""
    import os
    import sys
    env = dict(os.environ, GIE_TRACE_LAUNCHES="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    res = subprocess.run([sys.executable, "-c", _TRACE_CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr)
    calls = [blk.split("END")[0] for blk in res.stderr.split("BEGIN\n")[1:]]
    names = [[ln.split("launch ")[1].strip() for ln in c.splitlines() if "launch " in ln] for c in calls]
    assert names == [["k_glos_prep", "k_ground_footprints<false>"], ["k_glos_prep", "k_ground_footprints<true>"],
                     ["k_glos_prep", "k_ground_footprints<false>"], []], names


# ---------------------------------------------------------------------------------------------------------- 8. host layer
def test_host_layer_ground_local_plan_footprint_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_footprint_plan_probe")
    size, w, cutoff, gmin, gmax, min_known, radius = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15
    yaw, dt, T, inflate, v_min, v_max, omega_max = 2.4, 0.25, 20, 0.45, 0.1, 0.8, 1.5
    fp = (0.35, 0.15, 0.2)                                      # metres: front, back, half width
    frames, fpath = lidar_frames(tmp_path)
    robot = np.asarray(frames[-1][0][:2], np.float32)
    goal = np.array([[robot[0] + 1.5, robot[1] - 1.0], [robot[0] - 1.4, robot[1] + 1.2]], np.float32)
    head = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), repr(gmin), repr(gmax), str(min_known), repr(radius)]
    tail = [repr(yaw), repr(dt), str(T), repr(inflate), repr(v_min), repr(v_max), repr(omega_max)] + [repr(float(x)) for x in goal.ravel()]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + head[:1] + [out] + head[2:] + ["[%r, %r, %r]" % fp] + tail, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 best " in res.stdout and "poses %d headings %d records 81 footprints 81" % (81 * T * 2, 81 * T * 2) in res.stdout, (res.stdout, res.stderr)
    v, omega = np.fromfile(out + ".v", np.float32), np.fromfile(out + ".omega", np.float32)
    poses = np.fromfile(out + ".poses", np.float32).reshape(81, T, 2)
    hd = np.fromfile(out + ".headings", np.int32).reshape(81, T, 2)
    rec, frec = np.fromfile(out + ".rec", gie.GROUND_ROLLOUT_DTYPE), np.fromfile(out + ".fp", FD)
    best, plain, csq, fsq, bsq, ssq = np.fromfile(out + ".info", np.int32).tolist()
    want_sq = [int(np.floor((np.float32(x) / np.float32(w)) * (np.float32(x) / np.float32(w)))) for x in fp]
    assert [fsq, bsq, ssq] == want_sq == [12, 2, 4] and csq == 4
    # ground_local_plan()'s results are what they were: the same poses and records, from the shared arcs
    assert np.fromfile(out + ".plain_poses", np.float32).tobytes() == poses.tobytes() and np.fromfile(out + ".plain_rec", np.uint8).tobytes() == rec.tobytes()
    # the headings: numpy's, of the poses' own theta
    th = np.float64(np.float32(yaw)) + omega.astype(np.float64)[:, None] * np.float64(np.float32(dt)) * np.arange(T)[None, :]
    want_hd = np.stack([np.rint(32767.0 * np.cos(th)), np.rint(32767.0 * np.sin(th))], 2)
    assert np.abs(hd - want_hd).max() <= 1 and (np.abs(hd) <= 32767).all()              # (a sum of T terms against a product: the last bit of theta)
    # the records: the Mapper's, on those poses and headings
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        assert m.ground_nf1_compute(goal, csq) >= 1
        isq = int(np.ceil(np.float32(inflate) / np.float32(w))) ** 2
        assert m.ground_rollouts(poses, csq, isq, False, True).tobytes() == rec.tobytes()
        got = m.ground_footprints(poses, hd, fsq, bsq, ssq, 0, False, True)
        _same(got, P.footprints(m.read_ground(), poses, hd, m.pivot(), w, fsq, bsq, ssq, 0, P.MARGIN), "the mapper against the reference")
    finally:
        m.close()
    assert frec.tobytes() == got.tobytes()
    # the indices: the stated rule
    def pick(ok):
        ok = np.flatnonzero(ok)
        return -1 if not len(ok) else int(ok[np.lexsort((ok, rec["cost"][ok], rec["nf1_min"][ok]))[0]])
    base = (rec["poses"] >= 2) & (rec["nf1_min"] >= 0)
    assert plain == pick(base) and best == pick(base & (frec["poses"] >= 2)) and best >= 0
    assert (frec["poses"] >= 2).sum() >= 10 and len(set(frec["poses"].tolist())) > 2
    out = str(tmp_path / "off")                                 # "ground/footprint" unset: the call refuses, ground_local_plan() does not
    res = subprocess.run([exe] + head[:1] + [out] + head[2:] + ["-"] + tail, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "best -1 plain %d poses 3 headings 3 records 2 footprints 2" % plain in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == P5A * 96 and np.fromfile(out + ".fp", np.uint8).tobytes() == P5A * 64
    assert np.fromfile(out + ".poses", np.float32).tolist() == [-7.0] * 3 and np.fromfile(out + ".headings", np.int32).tolist() == [-7] * 3
    assert np.fromfile(out + ".info", np.int32).tolist() == [-1, plain, 4, -1, -1, -1]          # ground_footprint_sq() says "unset"

"""Ground view gain on the device (include/gie.h "ground view gain", gie_ground_view.inc.h) against the numpy statement of
tests/ground_view_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is of bytes.  The fields
at the staging limit (1024 cells a side) are checked against closed forms, so that no slow reference runs there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gie
import ground_ref as R
import ground_view_ref as V
import los_ref
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, ground as _ground, xy as _xy, scene as _scene, same as _same
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries of a mapper without frontier clusters
SD = gie.VIEW_SCORE_DTYPE


def _view_points(size, pvt, g):
    """about 20 views of a case: corners, edges, the centre, cells either side of x = 63 | 64 and 127 | 128, inside an obstacle,
    outside, NaN, +-inf, ties of gie_pos2coord's rounding"""
    X, Y = size[0], size[1]
    cx = lambda x: min(max(x, 0), X - 1)                        # noqa: E731
    cells = [(0, 0), (X - 1, 0), (0, Y - 1), (X - 1, Y - 1), (X // 2, 0), (0, Y // 2), (X - 1, Y // 2), (X // 2, Y // 2),
             (cx(62), Y // 3), (cx(63), Y // 3), (cx(64), Y // 3), (cx(65), Y // 2), (cx(127), Y // 4), (cx(128), Y // 4)]
    occ = np.argwhere(np.asarray(g["type"]) == R.OCCUPIED)
    cells.append(tuple(int(v) for v in occ[len(occ) // 2][::-1]))             # inside an obstacle
    cells += [(-1, 0), (X, Y - 1), (cx(3), Y)]                                # outside
    xy = _xy(pvt, cells)
    ties = _xy(pvt, [(cx(10), Y // 2), (cx(63), 0), (X - 1, Y - 1)], 0.5)     # a point on the border between two cells (and beyond the last)
    odd = _xy(pvt, [(cx(5), 0)] * 3)
    odd[:, 0] = [np.nan, np.inf, -np.inf]
    odd2 = _xy(pvt, [(cx(5), 0)])
    odd2[:, 1] = 1e30
    return np.concatenate([xy, ties, odd, odd2])


def _normals(base, n):
    """n x n_planes x 2: the base normals for the even views, their negatives for the odd ones"""
    b = np.asarray(base, np.int32).reshape(1, -1, 2)
    sign = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int32).reshape(-1, 1, 1)
    return np.ascontiguousarray(b * sign)


# (r_min, r_max in cells; normals of the even views; unknown_opaque; union)
COMBOS = [(0.0, 0.0, None, False, False), (0.0, 1.5, None, False, False), (0.0, 1.5, [(1, 0)], True, False), (1.5, 7.0, None, True, False),
          (0.0, 7.0, [(0, 1)], False, False), (2.0, 7.0, [(3, -2)], False, False), (0.0, 7.0, [(1, 0), (0, 1)], False, False),
          (0.0, 7.0, [(1, 0), (0, 1)], False, True), (0.0, 20.0, None, False, False), (0.0, 20.0, None, True, False),
          (7.0, 20.0, [(-5, 2), (3, 7)], True, False), (0.0, 20.0, [(-5, 2), (3, 7)], True, True), (0.0, 20.0, [(0, 0)], False, False),
          (0.0, 20.0, [(32767, -32767), (0, 0)], False, False), (20.0, 20.0, None, False, False), (0.0, 200.0, None, False, False),
          (0.0, 200.0, None, True, False), (0.0, 200.0, [(-1, -3)], True, False), (1.5, 3e37, [(2, 1), (2, -1)], False, True)]


# ---------------------------------------------------------------------------------------------------------- 1. box scenes
@pytest.mark.parametrize("size", [(64, 24, 8), (65, 24, 8), (70, 24, 8), (130, 24, 8), (130, 1, 8), (1, 40, 8)])
def test_gain_and_mask_equal_the_reference(size):
    import torch
    line = min(size[0], size[1]) == 1                           # (on a line one box hides everything behind it: fewer of them)
    pos, lab = _scene(size, 100 + size[0] + size[1], n_boxes=5 if line else 14, unknown_slab=4 if size[0] > 8 else 0)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        assert ((g["type"] == R.UNKNOWN).any() or size[0] == 1) and (g["type"] == R.OCCUPIED).any()
        xy = _view_points(size, pvt, g)
        n = len(xy)
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        hidden = visible = 0
        invalid = None
        for k, (r0, r1, base, uo, un) in enumerate(COMBOS):
            npl = 0 if base is None else len(base)
            nr = None if base is None else _normals(base, n)
            flags = (V.UNKNOWN_OPAQUE if uo else 0) | (V.UNION if un else 0)
            r0, r1 = np.float32(r0) * np.float32(W), np.float32(r1) * np.float32(W)
            want, masks = V.gain(g, xy, pvt, r0, r1, W, nr, npl, flags, masks=True)
            got = m.ground_view_gain(xy, r0, r1, nr, npl, uo, un)
            assert got.dtype == SD
            _same(got, want, (size, k))
            hidden += sum(int((mk == 1).sum()) for mk in masks)
            visible += sum(int((mk == 2).sum()) for mk in masks)
            invalid = want["candidates"] == -1
            # the _dev form: the same bytes, nothing beyond them
            with torch.cuda.stream(st):
                dxy = torch.from_numpy(xy).to(dev)
                dnr = torch.from_numpy(nr).to(dev) if nr is not None else None
                dout = torch.full((n * 16 + 1,), 0x5a, dtype=torch.uint8, device=dev)
                m.ground_view_gain_dev(dxy.data_ptr(), dnr.data_ptr() if dnr is not None else 0, n, dout.data_ptr(), r0, r1, npl, uo, un)
            m.sync()
            o = dout.cpu().numpy()
            assert o[:-1].tobytes() == want.tobytes() and o[-1] == 0x5a, (size, k)
            if k % 3 == 1 or r1 > 100 * W:                      # the mask of every view, host and _dev forms
                for i in range(n):
                    mk, sc = m.ground_view_mask(xy[i], r0, r1, None if nr is None else nr[i], npl, uo, un)
                    assert np.array_equal(mk, masks[i]) and sc.tobytes() == want[i].tobytes(), (size, k, i)
                with torch.cuda.stream(st):
                    dmask = torch.full((n, size[0] * size[1] + 1), 0x5a, dtype=torch.uint8, device=dev)
                    dsc = torch.full((n * 16 + 1,), 0x5a, dtype=torch.uint8, device=dev)
                    for i in range(n):
                        m.ground_view_mask_dev(dxy.data_ptr() + 8 * i, dnr.data_ptr() + 8 * npl * i if dnr is not None else 0, dmask[i].data_ptr(),
                                               dsc.data_ptr() + 16 * i if i % 2 == 0 else 0, r0, r1, npl, uo, un)
                m.sync()
                dm, ds = dmask.cpu().numpy(), dsc.cpu().numpy()
                assert (dm[:, -1] == 0x5a).all() and ds[-1] == 0x5a
                for i in range(n):
                    assert dm[i, :-1].tobytes() == masks[i].tobytes(), (size, k, i)
                    assert ds[16 * i:16 * i + 16].tobytes() == (want[i].tobytes() if i % 2 == 0 else P5A * 16), (size, k, i)
        assert invalid.sum() >= 6 and (~invalid).sum() >= 12    # outside, NaN, +-inf, 1e30; everything else has a cell
        # both outcomes: at least a tenth of the candidates hidden and at least a tenth visible (the reference's numbers)
        print("candidates %d: hidden %d visible %d" % (hidden + visible, hidden, visible))
        assert hidden * 10 >= hidden + visible and visible * 10 >= hidden + visible
        # a normal component beyond +-32767: the host form refuses, the _dev form scores that view -1
        nr = _normals([(40000, 1)], n)
        nr[1::2] = (1, 1)
        nr[0] = (1, 1)
        with pytest.raises(Exception):
            m.ground_view_gain(xy, 0.0, 0.7, nr, 1)
        want = V.gain(g, xy, pvt, 0.0, np.float32(0.7), W, nr, 1, 0)
        assert (want["candidates"][2:14:2] == -1).all() and want["candidates"][0] > 0
        with torch.cuda.stream(st):
            dnr = torch.from_numpy(nr).to(dev)
            dout = torch.full((n * 16,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_view_gain_dev(dxy.data_ptr(), dnr.data_ptr(), n, dout.data_ptr(), 0.0, np.float32(0.7), 1)
        m.sync()
        assert dout.cpu().numpy().tobytes() == want.tobytes()
        assert len(m.ground_view_gain(np.zeros((0, 2), np.float32), 0.0, 1.0)) == 0              # n == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. the staging limits
def _flat(size, wall=None, ring=None):
    """labels [1][Y][X] of a free plane: wall = (axis, at): a full OCCUPIED line x = at (axis 0) or y = at (axis 1); ring = (cx, cy, r):
    a closed square ring of never-seen cells at max-norm r around (cx, cy)"""
    X, Y = size[0], size[1]
    lab = np.ones((1, Y, X), np.int8)
    if wall is not None:
        if wall[0] == 0:
            lab[0, :, wall[1]] = 2
        else:
            lab[0, wall[1], :] = 2
    if ring is not None:
        cx, cy, r = ring
        mx = np.maximum(np.abs(np.arange(X)[None] - cx), np.abs(np.arange(Y)[:, None] - cy))
        lab[0][mx == r] = 0
    return lab


def _wall_mask(size, p, wall):
    """the closed form behind a full wall: every cell on p's side is visible; a wall cell is seen iff the line's last step is not
    along the wall (|d| along the wall <= |d| across it); everything beyond is hidden"""
    X, Y = size[0], size[1]
    dx, dy = np.arange(X)[None] - p[0] + 0 * np.arange(Y)[:, None], np.arange(Y)[:, None] - p[1] + 0 * np.arange(X)[None]
    across, along = (dx, dy) if wall[0] == 0 else (dy, dx)
    side = wall[1] - p[wall[0]]                                 # signed distance of the wall from p, not 0
    s = np.sign(side)
    mask = np.where(across * s < abs(side), 2, np.where((across * s == abs(side)) & (np.abs(along) <= abs(side)), 2, 1)).astype(np.uint8)
    mask[p[1], p[0]] = 0
    return mask


def _ring_mask(size, p, r):
    """the closed form inside a closed ring around p: the inside and the ring are visible, everything outside is hidden"""
    X, Y = size[0], size[1]
    mx = np.maximum(np.abs(np.arange(X)[None] - p[0]), np.abs(np.arange(Y)[:, None] - p[1]))
    mask = np.where(mx <= r, 2, 1).astype(np.uint8)
    mask[p[1], p[0]] = 0
    return mask


def _counts(g, mask):
    t = np.asarray(g["type"])
    s = np.zeros(1, SD)
    s[0] = (((mask == 2) & (t == R.UNKNOWN)).sum(), ((mask == 2) & (t == R.FNT)).sum(), ((mask == 2) & (t == R.OCCUPIED)).sum(), (mask > 0).sum())
    return s


LIMIT_CASES = [((1024, 1024, 1), None, None), ((1024, 1024, 1), (1, 600), (300, 800, 5)), ((1024, 3, 1), None, None), ((1024, 3, 1), (0, 600), None),
               ((3, 1024, 1), None, None), ((3, 1024, 1), (1, 600), None)]


@pytest.mark.parametrize("size,wall,ring", LIMIT_CASES)
def test_fields_at_the_staging_limit_against_closed_forms(size, wall, ring):
    X, Y = size[0], size[1]
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pvt = _settle(m, _flat(size, wall, ring))
        g = _ground(m, size)
        t = g["type"]
        want_occ = np.zeros((Y, X), bool)
        if wall is not None:
            want_occ[(slice(None), wall[1]) if wall[0] == 0 else (wall[1], slice(None))] = True
        assert np.array_equal(t == R.OCCUPIED, want_occ)
        assert ((t == R.UNKNOWN).sum() == 40) if ring is not None else not (t == R.UNKNOWN).any()
        corners = [(0, 0), (X - 1, 0), (0, Y - 1), (X - 1, Y - 1)]          # the staged box is the whole plane
        views = corners + [(X // 2, Y // 2), (X // 3, min(100, Y - 1)), (min(700, X - 1), Y - 1)]
        xy = _xy(pvt, views)
        r_max = np.float32(3000.0)                              # beyond the field: every other cell is a candidate
        got = m.ground_view_gain(xy, 0.0, r_max)
        for i, p in enumerate(views):
            if wall is None:
                want = np.full((Y, X), 2, np.uint8)             # an empty field: every candidate is visible
                want[p[1], p[0]] = 0
            else:
                if p[wall[0]] == wall[1]:
                    continue
                want = _wall_mask(size, p, wall)
            mk, sc = m.ground_view_mask(xy[i], 0.0, r_max)
            assert np.array_equal(mk, want), (p, int((mk != want).sum()))
            ws = _counts(g, want)
            assert ws["candidates"][0] == X * Y - 1 and sc.tobytes() == ws.tobytes() and got[i].tobytes() == ws.tobytes(), p
            if wall is None:
                assert [int(sc[k]) for k in ("unknown", "frontier", "occupied")] == [int((t == c).sum()) - int(t[p[1], p[0]] == c) for c in (R.UNKNOWN, R.FNT, R.OCCUPIED)]
        if ring is not None:                                    # (with UNKNOWN transparent the ring has changed nothing above; opaque, it casts a shadow)
            assert (m.ground_view_mask(xy[2], 0.0, r_max, unknown_opaque=True)[0] == 1).sum() > (_wall_mask(size, views[2], wall) == 1).sum()
        if ring is not None:                                    # a closed ring around p, opaque by the flag
            p = ring[:2]
            mk, sc = m.ground_view_mask(_xy(pvt, [p])[0], 0.0, r_max, unknown_opaque=True)
            want = _ring_mask(size, p, ring[2])
            assert np.array_equal(mk, want), int((mk != want).sum())
            ws = _counts(g, want)
            assert sc.tobytes() == ws.tobytes() and ws["unknown"][0] == 40 and ws["candidates"][0] == X * Y - 1
            assert m.ground_view_gain(_xy(pvt, [p]), 0.0, r_max, unknown_opaque=True).tobytes() == ws.tobytes()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. a larger field
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
        cells = [(256, 256), (0, 0), (511, 300), (63, 64), (128, 127), (400, 90), (5, 500), (300, 511)]
        xy = _xy(pvt, cells)
        r = np.float32(100.0) * np.float32(W)
        nr = _normals([(3, 1), (-1, 2)], len(xy))
        for npl, uo, un, k in ((0, False, False, 8), (2, True, True, 3)):
            xy, nr = xy[:k], nr[:k]
            want, masks = V.gain(g, xy, pvt, 0.0, r, W, nr if npl else None, npl, (V.UNKNOWN_OPAQUE if uo else 0) | (V.UNION if un else 0), masks=True)
            got = m.ground_view_gain(xy, 0.0, r, nr if npl else None, npl, uo, un)
            _same(got, want, (npl, uo))
            assert (want["candidates"] > (5000 if npl == 0 else 1000)).all() and sum(int((mk == 1).sum()) for mk in masks) > 1000
            mk, sc = m.ground_view_mask(xy[0], 0.0, r, nr[0] if npl else None, npl, uo, un)
            assert np.array_equal(mk, masks[0]) and sc.tobytes() == want[0].tobytes()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. many views
def test_66000_views_in_one_call():
    import torch
    size = (64, 24, 8)
    pos, lab = _scene(size, 188)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        n = 66000                                               # beyond 65535: the views are not a grid dimension of their own
        rng = np.random.default_rng(66)
        cells = np.stack([rng.integers(-1, size[0] + 1, n), rng.integers(-1, size[1] + 1, n)], 1)
        xy = _xy(pvt, cells)
        r = np.float32(1.5) * np.float32(W)
        uniq, inv = np.unique(cells, axis=0, return_inverse=True)
        want = V.gain(g, _xy(pvt, uniq), pvt, 0.0, r, W, None, 0, V.UNKNOWN_OPAQUE)[inv.ravel()]
        got = m.ground_view_gain(xy, 0.0, r, unknown_opaque=True)
        _same(got, want, "host")
        assert (want["candidates"] == 8).sum() > 40000 and (want["candidates"] == -1).sum() > 1000 and (want["candidates"] == 3).any()
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(torch.cuda.ExternalStream(m.stream_handle(), device=dev)):
            dxy = torch.from_numpy(xy).to(dev)
            dout = torch.full((n * 16 + 1,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_view_gain_dev(dxy.data_ptr(), 0, n, dout.data_ptr(), 0.0, r, 0, True)
        m.sync()
        o = dout.cpu().numpy()
        assert o[:-1].tobytes() == want.tobytes() and o[-1] == 0x5a
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. against the 3-D section
def test_a_flat_volume_agrees_with_the_3d_view_gain():
    size = (70, 24, 1)
    pos, lab = _scene(size, 41, n_boxes=8)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        loc = m.read_local(dist_sq=False, coc=False)
        g = _ground(m, size)
        assert np.array_equal(g["type"], loc["type"][0])        # every column is its one voxel
        assert (g["type"] == R.UNKNOWN).any() and (g["type"] == R.OCCUPIED).any()
        xy = _view_points(size, pvt, g)
        n = len(xy)
        pos3 = np.concatenate([xy, np.full((n, 1), np.float32(pvt[2]) * np.float32(W), np.float32)], 1)
        for flag3 in (0, los_ref.UNKNOWN_OPAQUE):               # the 3-D flag corresponds to the ground flag
            m.los_prepare(0.0, flag3)
            for r0, r1 in ((0.0, 1.5), (0.0, 7.0), (2.0, 20.0), (0.0, 200.0)):
                r0, r1 = np.float32(r0) * np.float32(W), np.float32(r1) * np.float32(W)
                for base in (None, [(1, 0)], [(3, -2), (1, 5)]):
                    s3 = m.view_gain(gie.make_views(pos3, None if base is None else [(a, b, 0) for a, b in base]), r0, r1, -1.0)
                    nr = None if base is None else np.ascontiguousarray(np.broadcast_to(np.asarray(base, np.int32), (n, len(base), 2)))
                    s2 = m.ground_view_gain(xy, r0, r1, nr, 0 if base is None else len(base), bool(flag3))
                    _same(s2, s3, (flag3, float(r1), base))
                    _same(s2, V.gain(g, xy, pvt, r0, r1, W, nr, 0 if base is None else len(base), V.UNKNOWN_OPAQUE if flag3 else 0), "reference")
            assert (s2["candidates"] > 100).any() and (s2["candidates"] == -1).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. chained
def test_chained_behind_the_ground_field_and_its_clusters_with_one_sync():
    import torch
    size = (70, 40, 8)
    pos, lab = _scene(size, 91, n_boxes=10)
    m = _mapper(size)
    cap = 64
    try:
        pvt = _settle(m, lab, pos)
        z = pvt[2]
        dev = torch.device("cuda", 0)
        r0, r1 = np.float32(0.2), np.float32(1.5)
        with torch.cuda.stream(torch.cuda.ExternalStream(m.stream_handle(), device=dev)):
            dgoal = torch.full((cap, 2), 7.0, dtype=torch.float32, device=dev)
            dout = torch.full((cap * 16 + 1,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_compute_dev(z, z + size[2] - 1, 1, False, 0)
            m.ground_frontier_compute_dev(0, 2, 8, cap, 0)
            m.read_ground_frontier_clusters_dev(0, dgoal.data_ptr(), 0)
            m.ground_view_gain_dev(dgoal.data_ptr(), 0, cap, dout.data_ptr(), r0, r1, 0, True)
        m.sync()                                                # the only wait
        goal, o = dgoal.cpu().numpy(), dout.cpu().numpy()
        g = m.read_ground()
        have = int(np.isfinite(goal[:, 0]).sum())
        assert 1 <= have < cap and np.isnan(goal[have:]).all()
        want = V.gain(g, goal, pvt, r0, r1, W, None, 0, V.UNKNOWN_OPAQUE)
        assert o[:-1].tobytes() == want.tobytes() and o[-1] == 0x5a
        assert (want["candidates"][have:] == -1).all() and (want["candidates"][:have] > 0).all()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. refusals
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
        nr = np.ones((n, 2, 2), np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())

        def VP(**kw):
            p = _capi.GroundViewParam(0.0, 1.0, 0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert all(a.tobytes() == P5A * a.size for a in host) and bool((dbuf == 0x5a).all())

        def refused(h, who, p="default", n_=n, a=True, b=True, out=True, mask=True, host_only=False, nrm=None):
            p = VP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            hn = ptr(nr if nrm is None else nrm)
            assert f["ground_view_gain"](h, ptr(xy) if a else None, hn if b else None, n_, pr, ptr(host[0]) if out else None) == INVALID, who
            if not host_only:
                assert f["ground_view_gain_dev"](h, dp if a else None, dp if b else None, n_, pr, dp if out else None) == INVALID, who
            if n_ == n:                                         # (the mask forms have no n)
                assert f["ground_view_mask"](h, ptr(xy) if a else None, hn if b else None, pr, ptr(host[0]) if mask and out else None, ptr(host[1])) == INVALID, who
                if not host_only:
                    assert f["ground_view_mask_dev"](h, dp if a else None, dp if b else None, pr, dp if mask and out else None, dp) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            refused(h, who)
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper: all four refuse
        refused(t._h, "tiled")
        unwritten()
        z = pvt[2]
        m.ground_compute(z, z + 7)
        refused(m._h, "null param", None)
        bad = [VP(r_min=-0.5), VP(r_min=2.0), VP(r_min=float("nan")), VP(r_max=float("nan")), VP(r_max=float("inf")), VP(r_min=float("-inf")),
               VP(r_min=float("inf"), r_max=float("inf")), VP(n_planes=-1), VP(n_planes=3), VP(n_planes=2 ** 31 - 1), VP(flags=4), VP(flags=7), VP(flags=-2 ** 31),
               VP(flags=2), VP(flags=3, n_planes=1), VP(flags=2, n_planes=1)] + [VP(reserved=i) for i in range(4)] + [VP(n_planes=2, reserved=3)]
        for p in bad:
            refused(m._h, (p.r_min, p.r_max, p.n_planes, p.flags, list(p.reserved)), p)
        refused(m._h, "n < 0", n_=-1)
        refused(m._h, "null xy", a=False)
        refused(m._h, "null out / null mask", out=False)
        refused(m._h, "null normals with planes", VP(n_planes=1), b=False)
        refused(m._h, "null normals with two planes", VP(n_planes=2, flags=2), b=False)
        for v in (32768, -32768, 2 ** 31 - 1, -2 ** 31):       # the host forms read the normals
            far = nr.copy()
            far[0, 1, 1] = v
            refused(m._h, "normal %d" % v, VP(n_planes=2), host_only=True, nrm=far)
            far = nr.copy()
            far[0, 0, 0] = v
            refused(m._h, "normal %d" % v, VP(n_planes=1), host_only=True, nrm=far)
        unwritten()
        # (the same calls with good arguments work; n == 0 is valid with NULL arrays; a NULL score is fine)
        assert f["ground_view_gain"](m._h, None, None, 0, C.byref(VP()), None) == 0 and f["ground_view_gain_dev"](m._h, None, None, 0, C.byref(VP()), None) == 0
        unwritten()
        assert f["ground_view_gain"](m._h, ptr(xy), ptr(nr), n, C.byref(VP(n_planes=2, flags=2)), ptr(host[0])) == 0
        assert (host[0][:16 * n].view(SD)["candidates"] > 0).all() and host[0][16 * n:].tobytes() == P5A * (4096 - 16 * n)
        assert f["ground_view_mask"](m._h, ptr(xy), None, C.byref(VP()), ptr(host[1]), None) == 0
        assert host[1][:32 * 24].max() == 2 and host[1][32 * 24:].tobytes() == P5A * (4096 - 32 * 24)
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 8. nothing else is written
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
            xy = _xy(gp, r.integers(0, 40, (30, 2)))
            a.ground_view_gain(xy, 0.0, 1.2, _normals([(1, 2)], 30), 1, k % 2 == 0)
            a.ground_view_mask(xy[0], 0.3, 5.0)

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
        m.ground_nf1_compute(_xy(pvt0, [(30, 24)]), 1, False, True)
        nf0 = m.read_ground_nf1()
        xy = _xy(pvt0, [(5, 5), (60, 40), (33, 20), (50, 8), (0, 47), (63, 0)])
        r = np.float32(1.6)
        s0 = m.ground_view_gain(xy, 0.0, r)
        mk0, _ = m.ground_view_mask(xy[2], 0.0, r, unknown_opaque=True)
        _same(s0, V.gain(g0, xy, pvt0, 0.0, r, W), "before")
        # the calls wrote nothing of the ground field or of its navigation function
        g0b = m.read_ground()
        assert all(np.array_equal(g0[k], g0b[k]) for k in g0) and np.array_equal(m.read_ground_nf1(), nf0)
        # a map update between two calls changes no result: the field stays at its own pivot
        pvt1 = step(1)
        assert tuple(pvt1) != tuple(pvt0)
        assert m.ground_view_gain(xy, 0.0, r).tobytes() == s0.tobytes()
        assert np.array_equal(m.ground_view_mask(xy[2], 0.0, r, unknown_opaque=True)[0], mk0)
        # a new ground field does: later calls see it, at its pivot, with no prepare in between (and without a navigation function)
        g1 = _ground(m, size)
        s1 = m.ground_view_gain(xy, 0.0, r)
        _same(s1, V.gain(g1, xy, pvt1, 0.0, r, W), "after")
        assert s1.tobytes() != s0.tobytes()
        assert np.array_equal(m.ground_view_mask(xy[2], 0.0, r, unknown_opaque=True)[0], V.gain(g1, xy[2:3], pvt1, 0.0, r, W, None, 0, V.UNKNOWN_OPAQUE, masks=True)[1][0])
    finally:
        m.close()


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
        m.ground_view_gain(xy, 0.0, 0.5)
        m.ground_view_mask(xy[0], 0.0, 0.5)
        d = torch.zeros((256,), dtype=torch.uint8, device="cuda:0")
        dxy = torch.from_numpy(xy).to("cuda:0")
        m.ground_view_gain_dev(dxy.data_ptr(), 0, 2, d.data_ptr(), 0.0, 0.5)
        m.ground_view_gain(np.zeros((0, 2), np.float32), 0.0, 0.5)          # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_query"][1] == 3 and prof["ground_query"][0] > 0
        assert all(v[1] == 0 for k, v in prof.items() if k != "ground_query")
        assert list(prof) == NAMES
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 9. host layer
def test_host_layer_ground_exploration_gains_matches_the_mapper(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = build_host_probe(tmp_path, "ground_gains_probe", ["-DGIE_HOST_WITH_HIP", "-I" + os.path.join(rocm, "include"), "-Wno-unused-result",
                                                            "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    size, w, cutoff, gmin, gmax, min_known, radius, cap, min_size, r_min, r_max = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15, 24, 2, 0.25, 1.25
    frames, fpath = lidar_frames(tmp_path)
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        g = m.read_ground()
        pvt = m.pivot()
        csq = int(np.ceil(np.float32(radius) / np.float32(w))) ** 2
        assert csq == 4
        kept, cells = m.ground_frontier_compute(csq, min_size, 8, cap)
        rec, goal, _ = m.read_ground_frontier_clusters()
        have = len(rec)
        assert have == min(kept, cap) >= 1
        m.ground_nf1_compute(np.array([frames[-1][0][:2]], np.float32), csq)
        steps = m.ground_nf1_query(goal)
        scores = m.ground_view_gain(goal, r_min, r_max)
        _same(scores, V.gain(g, goal, pvt, r_min, r_max, w), "the mapper chain")
        assert (scores["candidates"][:have] > 0).all() and (scores["candidates"][have:] == -1).all()
    finally:
        m.close()
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), repr(radius), str(cap), str(min_size), repr(r_min), repr(r_max)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 clusters %d steps %d scores %d" % (have, have, have) in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == rec.tobytes()
    assert np.fromfile(out + ".steps", np.int32).tolist() == steps[:have].tolist()
    assert np.fromfile(out + ".scores", np.uint8).tobytes() == scores[:have].tobytes()
    assert np.fromfile(out + ".info", np.int32).tolist() == [kept, cells, csq]
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", repr(radius), str(cap), str(min_size), repr(r_min), repr(r_max)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 clusters 2 steps 3 scores 4" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == P5A * 128 and np.fromfile(out + ".steps", np.uint8).tobytes() == P5A * 12
    assert np.fromfile(out + ".scores", np.uint8).tobytes() == P5A * 64 and np.fromfile(out + ".info", np.int32).tolist() == [0, 0, csq]

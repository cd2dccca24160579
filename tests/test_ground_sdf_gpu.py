"""The ground signed distance field on the device (include/gie.h "ground signed distance", gie_ground_sdf.inc.h) against the numpy
statement of tests/ground_sdf_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is of bytes:
no tolerance, no cell or point left out."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gie
import ground_ref as R
import ground_sdf_ref as S
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, ground as _ground, xy as _xy, plane as _plane, arc
from stage_common import W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
NAMES = ["ogm_classify", "ray_register", "ray_free", "ray_finalize", "block_alloc", "fuse", "edt_pass_y", "edt_pass_x", "edt_pass_z", "mark",
         "frontiers", "wave_a", "wave_b", "waves", "commit", "edt_prep", "mark_commit", "ground_nf1", "ground", "ground_query", "cloud", "los",
         "los_query", "sdf", "sdf_query"]                       # gie_profile_read's entries of a mapper without frontier clusters
RD = gie.GROUND_SDF_ROLLOUT_DTYPE


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Field:
    """a mapper settled on a [Y][X] label plane (0 never seen, 1 free, 2 occupied) with its ground field: m, pvt, g = read_ground()"""

    def __init__(self, size, lab2d, blocks=False, pos=(0.0, 0.0, 0.0)):
        self.size, self.blocks = size, blocks
        self.m = _mapper(size)
        try:
            self.pvt = _settle(self.m, _plane(size, lab2d), pos)
            self.g = _ground(self.m, size, blocks=blocks)
        except Exception:
            self.m.close()
            raise
        self.f = S.field(self.g, size, blocks)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.m.close()


def _check_planes(fd, what):
    """read_ground_sdf against the reference, both planes, bytes; returns the reference"""
    got = fd.m.read_ground_sdf()
    f = fd.f
    assert np.array_equal(got["inside_dist_sq"], f["inside_dist_sq"]), (what, np.argwhere(got["inside_dist_sq"] != f["inside_dist_sq"])[:5].tolist())
    assert got["inside_dist_sq"].dtype == np.int32 and got["sdf"].dtype == np.float32
    assert np.array_equal(u32(got["sdf"]), u32(f["sdf"])), what
    assert list(fd.m.read_ground_sdf(sdf=False)) == ["inside_dist_sq"] and list(fd.m.read_ground_sdf(inside_dist_sq=False)) == ["sdf"]
    return f


def _same_records(got, want, what):
    """two record arrays: field by field (the failing field is named; floats by their bits, a NaN equals itself), then byte for byte"""
    for key in want.dtype.names:
        a, b = (u32(got[key]), u32(want[key])) if want.dtype[key].base == np.float32 else (got[key], want[key])
        assert np.array_equal(a, b), (what, key, got[key].tolist(), want[key].tolist())
    assert got.tobytes() == want.tobytes(), what


def _phantom(obs):
    """inside_dist_sq if the padding bits of the last word were free columns at x >= X"""
    Y, X = obs.shape
    pad = (-X) % 64
    if not pad:
        return S.inside_dist_sq(obs)
    return S.inside_dist_sq(np.concatenate([obs, np.zeros((Y, pad), bool)], 1))[:, :X]


# ---------------------------------------------------------------------------------------------------------- 1. inside distances and gsdf
@pytest.mark.parametrize("X", [1, 2, 63, 64, 65, 70, 128, 130])
def test_inside_distances_over_x(X):
    import torch
    Y = 24
    size = (X, Y, 1)
    right = np.ones((Y, X), np.int8)
    right[3:21, (X // 2 if X > 2 else 0):] = 2                  # a solid block reaching the right edge: the nearest free column of a row lies only to the left (X <= 2: above and below)
    cross = np.ones((Y, X), np.int8)
    cross[8:15, :] = 2                                          # a block through all four edges
    cross[:, max(X // 2 - 3, 0):X // 2 + 4] = 2
    labs = [("right edge", right), ("all four edges", cross)]
    if X > 64:
        word = np.ones((Y, X), np.int8)
        word[4:19, 57:min(71, X)] = 2                           # a block over the word boundary at 63 | 64
        labs.append(("word boundary", word))
    for what, lab in labs:
        with Field(size, lab) as fd:
            assert np.array_equal(fd.f["obs"], lab == 2), what  # the scene is the one that was drawn
            f = _check_planes(fd, (X, what))
            if what == "right edge" and X % 64:
                # on the CPU side: a free bit at x >= X would shorten distances of this scene
                ph = _phantom(f["obs"])
                assert (ph != f["inside_dist_sq"]).sum() >= 4 and (ph <= f["inside_dist_sq"])[f["obs"]].all(), X
            if what == "right edge" and X >= 63:
                assert f["inside_dist_sq"].max() >= 9 * 9
            if what == "word boundary":
                assert f["inside_dist_sq"][11, 63] > 25 and f["inside_dist_sq"][11, 64] > 25
            if what == "all four edges":
                ds = torch.full((X * Y + 1,), -5.0, dtype=torch.float32, device="cuda:0")
                di = torch.full((X * Y + 1,), -5, dtype=torch.int32, device="cuda:0")
                st = torch.cuda.ExternalStream(fd.m.stream_handle(), device=torch.device("cuda", 0))
                with torch.cuda.stream(st):
                    fd.m.read_ground_sdf_dev(ds.data_ptr(), di.data_ptr())
                fd.m.sync()
                assert np.array_equal(u32(ds.cpu().numpy()[:-1]), u32(f["sdf"]).ravel()) and np.array_equal(di.cpu().numpy()[:-1], f["inside_dist_sq"].ravel())
                assert ds[-1].item() == -5.0 and di[-1].item() == -5


@pytest.mark.parametrize("Y", [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_inside_distances_over_y(Y):
    X = 16
    lab = np.ones((Y, X), np.int8)
    y0 = Y // 5
    y1 = y0 + max(int(round(0.45 * Y)), 1) if Y > 1 else 1
    lab[y0:y1, :] = 2                                           # 45 % of the rows, all of x: the nearest free column lies along y only
    if Y > 1:
        lab[y0 + (y1 - y0) // 3, 5] = 1                         # and one free cell inside it
    with Field((X, Y, 1), lab) as fd:
        f = _check_planes(fd, Y)
        if Y >= 64:
            assert f["inside_dist_sq"].max() >= (Y // 12) ** 2   # distances of a twelfth of the line and more
        if Y == 1024:
            assert f["inside_dist_sq"].max() > 100 * 100
        if Y == 1:
            assert (f["inside_dist_sq"] == -1).all()


def test_the_gate():
    size = (70, 24, 1)
    thin = np.ones((24, 70), np.int8)
    thin[2, 3:60] = 2                                           # walls one and two cells thick
    thin[5:20, 10] = 2
    thin[8:10, 20:38] = 2                                       # (they neither cross nor meet in a corner: a crossing has interior cells)
    thin[4:22, 40:42] = 2
    thin[0, 5:60] = 2
    thin[12:20, 69] = 2
    with Field(size, thin) as fd:
        f = _check_planes(fd, "thin walls")
        assert S.interior(f["obs"]).sum() == 0 and f["obs"].sum() > 200
        assert set(np.unique(f["inside_dist_sq"]).tolist()) == {0, 1}
    block = np.ones((24, 70), np.int8)
    block[10:13, 62:65] = 2                                     # one 3 x 3 block, over the word boundary
    with Field(size, block) as fd:
        f = _check_planes(fd, "3 x 3")
        assert S.interior(f["obs"]).sum() == 1 and (f["inside_dist_sq"] == 4).sum() == 1 and f["inside_dist_sq"][11, 63] == 4 and f["inside_dist_sq"].max() == 4


@pytest.mark.parametrize("size", [(70, 24, 2), (64, 9, 1)])
def test_all_obstacles_no_obstacle_and_one_free_cell(size):
    X, Y = size[0], size[1]
    far = np.float32(size[0] ** 2 + size[1] ** 2 + size[2] ** 2)
    with Field(size, np.full((Y, X), 2, np.int8)) as fd:
        f = _check_planes(fd, "all obstacles")
        got = fd.m.read_ground_sdf()
        assert (got["inside_dist_sq"] == -1).all() and (got["sdf"] == -far).all()
    with Field(size, np.ones((Y, X), np.int8)) as fd:
        f = _check_planes(fd, "no obstacle")
        got = fd.m.read_ground_sdf()
        assert (got["inside_dist_sq"] == 0).all() and (got["sdf"] == far).all() and (fd.g["dist_sq"] == -1).all()
    yy, xx = np.indices((Y, X))
    for cx, cy in ((0, 0), (X - 1, 0), (0, Y - 1), (X - 1, Y - 1)):
        lab = np.full((Y, X), 2, np.int8)
        lab[cy, cx] = 1
        with Field(size, lab) as fd:
            _check_planes(fd, (cx, cy))
            got = fd.m.read_ground_sdf()
            closed = ((xx - cx) ** 2 + (yy - cy) ** 2).astype(np.int32)
            assert np.array_equal(got["inside_dist_sq"], closed), (cx, cy)
            want = np.where(closed <= 1, np.float32(0), np.float32(1) - np.sqrt(closed.astype(np.float32))).astype(np.float32)
            want[cy, cx] = np.float32(1)                        # the free cell: one cell from its neighbours
            assert np.array_equal(u32(got["sdf"]), u32(want)), (cx, cy)


def test_unknown_blocks_with_and_without():
    size = (70, 30, 2)
    lab = np.ones((30, 70), np.int8)
    lab[0, :] = lab[-1, :] = 2                                  # a room
    lab[:, 0] = lab[:, -1] = 2
    lab[6:20, 50:68] = 0                                        # with a never-seen slab
    res = {}
    for blocks in (False, True):
        with Field(size, lab, blocks) as fd:
            f = _check_planes(fd, blocks)
            assert (fd.g["type"] == R.UNKNOWN).sum() == 14 * 18
            res[blocks] = f["inside_dist_sq"]
    # without the flag the room's four corners alone are deeper than 1 (two walls and twice the outside around them: 2 to the cell inside)
    assert res[False].max() == 2 and (res[False] > 1).sum() == 4 and res[True].max() == 49 and (res[True][6:20, 50:68] >= 1).all()


# ---------------------------------------------------------------------------------------------------------- 2. the cache
def test_the_cache_follows_the_ground_field_and_nothing_else():
    size = (64, 48, 8)
    rng = np.random.default_rng(7)
    boxes = []
    for _ in range(40):
        s = rng.integers(4, 12, size=3)
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
        step(0)
        g0 = _ground(m, size)
        a = m.read_ground_sdf()
        f0 = S.field(g0, size)
        assert np.array_equal(a["inside_dist_sq"], f0["inside_dist_sq"]) and np.array_equal(u32(a["sdf"]), u32(f0["sdf"])) and f0["inside_dist_sq"].max() > 4
        b = m.read_ground_sdf()                                 # two reads without a compute between them
        assert a["sdf"].tobytes() == b["sdf"].tobytes() and a["inside_dist_sq"].tobytes() == b["inside_dist_sq"].tobytes()
        m.profile_enable(True)
        m.profile_read()
        m.read_ground_sdf()
        assert m.profile_read()["ground"][1] == 1               # the export alone: the plane is reused
        step(1)                                                 # a map update without a new compute: the field stays, as the ground field does
        c = m.read_ground_sdf()
        assert m.profile_read()["ground"][1] == 1
        assert a["sdf"].tobytes() == c["sdf"].tobytes() and a["inside_dist_sq"].tobytes() == c["inside_dist_sq"].tobytes()
        gb = m.read_ground()
        assert all(np.array_equal(g0[k], gb[k]) for k in g0)
        g1 = _ground(m, size)                                   # a new compute: the field follows the map
        m.profile_read()
        d = m.read_ground_sdf()
        assert m.profile_read()["ground"][1] == 2               # the inside pass and the export
        m.profile_enable(False)
        f1 = S.field(g1, size)
        assert np.array_equal(d["inside_dist_sq"], f1["inside_dist_sq"]) and np.array_equal(u32(d["sdf"]), u32(f1["sdf"]))
        assert not np.array_equal(f1["inside_dist_sq"], f0["inside_dist_sq"])
        m.ground_compute(m.pivot()[2], m.pivot()[2] + 7, 9, True)       # and its flags: no column has nine known voxels, every UNKNOWN one blocks
        e = m.read_ground_sdf()
        f2 = S.field(m.read_ground(), size, True)
        assert np.array_equal(e["inside_dist_sq"], f2["inside_dist_sq"]) and np.array_equal(u32(e["sdf"]), u32(f2["sdf"])) and (e["inside_dist_sq"] == -1).all()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. queries
def _query_scene(size):
    """a 12 x 12 block clipped by the rectangle, placed so that a free cell remains; (2, 2): three obstacle cells around one free one"""
    X, Y = size[0], size[1]
    lab = np.ones((Y, X), np.int8)
    if (X, Y) == (2, 2):
        lab[:] = 2
        lab[0, 0] = 1
        return lab
    x0, y0 = (X // 3 if X > 1 else 0), (Y // 3 if Y > 1 else 0)
    lab[y0:y0 + 12, x0:x0 + 12] = 2
    if X > 30:
        lab[min(2, Y - 1), X - 9:X - 2] = 0                                 # never-seen cells: flag bit 1
    return lab


def _query_points(size, rng, n=20000):
    """local coordinates (cells, fractions): around the block and over the rectangle and a cell beyond it, the exact faces, both ends of a
    flat axis's interval, gie_pos2coord's ties; the values that are no point come in _special"""
    X, Y = size[0], size[1]
    x0, y0 = (X // 3 if X > 1 else 0), (Y // 3 if Y > 1 else 0)
    lo, hi = np.array([-1.0 if X > 1 else -0.7, -1.0 if Y > 1 else -0.7]), np.array([X if X > 1 else 0.7, Y if Y > 1 else 0.7])
    a = rng.uniform(lo, hi, (n // 2, 2))
    b = rng.uniform(np.maximum([x0 - 2, y0 - 2], 0), np.minimum([x0 + 14, y0 + 14], [max(X - 1, 0), max(Y - 1, 0)]), (n - n // 2 - 400, 2))
    if X == 1:
        a[:, 0], b[:, 0] = rng.uniform(-0.6, 0.6, len(a)), rng.uniform(-0.45, 0.45, len(b))
    if Y == 1:
        a[:, 1], b[:, 1] = rng.uniform(-0.6, 0.6, len(a)), rng.uniform(-0.45, 0.45, len(b))
    faces = np.array([(x, y) for x in (0, X - 1, -0.5, 0.5, X - 0.5, 0.4999999, -0.5000001) for y in (0, Y - 1, -0.5, 0.5, Y - 0.5, 0.4999999, -0.5000001)], np.float64)
    ties = np.floor(rng.uniform(lo, hi, (400 - len(faces) - 16, 2))) + 0.5
    ints = np.floor(rng.uniform([0, 0], [X, Y], (16, 2)))
    return np.concatenate([a, b, faces, ties, ints])


def _special(xy, rng):
    k = rng.choice(len(xy), 60, replace=False)
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38]
    for j, i in enumerate(k):
        xy[i, j % 2] = vals[(j // 2) % len(vals)]
    xy[k[-1]] = np.nan
    return xy


@pytest.mark.parametrize("size", [(1, 40, 1), (40, 1, 1), (2, 2, 1), (65, 20, 2), (130, 70, 2)])
def test_queries_equal_the_reference(size):
    import torch
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    pos = (-3.0, -2.0, 0.0)                                     # a negative pivot
    with Field(size, _query_scene(size), pos=pos) as fd:
        m, pvt, f, g = fd.m, fd.pvt, fd.f, fd.g
        assert pvt[0] < 0 and pvt[1] < 0
        assert (f["inside_dist_sq"] > 1).any()
        xy = _special(_xy(pvt, _query_points(size, rng)), rng)
        n = len(xy)
        assert n == 20000
        dist, grad, flags = S.query(f, g, pvt, W, xy)
        # on the CPU side: the samples are worth it
        inside = (flags & 1) == 1
        deep = np.zeros(n, bool)
        for i in np.flatnonzero(inside):
            u = [np.float32(xy[i, k]) / np.float32(W) - np.float32(pvt[k]) for k in range(2)]
            ix = min(int(np.floor(u[0])), size[0] - 2) if size[0] > 1 else 0
            iy = min(int(np.floor(u[1])), size[1] - 2) if size[1] > 1 else 0
            deep[i] = (f["inside_dist_sq"][iy:iy + 2, ix:ix + 2] > 1).any()
        assert inside.sum() > n // 2 and (~inside).sum() > 100 and deep.sum() * 10 >= inside.sum(), (inside.sum(), deep.sum())
        assert (dist[inside] < 0).any() and (dist[inside] > 0).any()
        for k in range(2):
            if size[k] == 1:
                assert (grad[:, k] == 0).all() and (u32(grad[:, k]) == 0).all()     # a flat axis: exactly 0
        got = m.ground_query_sdf(xy)
        assert np.array_equal(u32(got[0]), u32(dist)), np.flatnonzero(u32(got[0]) != u32(dist))[:5].tolist()
        assert np.array_equal(u32(got[1]), u32(grad)), np.argwhere(u32(got[1]) != u32(grad))[:5].tolist()
        assert np.array_equal(got[2], flags)
        # each of the three outputs NULL in turn
        for drop in range(3):
            want = [k != drop for k in range(3)]
            part = m.ground_query_sdf(xy, *want)
            assert part[drop] is None
            for k, ref in enumerate((dist, grad, flags)):
                if k != drop:
                    assert part[k].tobytes() == ref.tobytes()
        # the _dev form through torch on the mapper's stream, with poisoned tails
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            dxy = torch.from_numpy(xy).to(dev)
            dd = torch.full((n + 1,), -5.0, dtype=torch.float32, device=dev)
            dg = torch.full((2 * n + 2,), -5.0, dtype=torch.float32, device=dev)
            df = torch.full((n + 1,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_query_sdf_dev(dxy.data_ptr(), n, dd.data_ptr(), dg.data_ptr(), df.data_ptr())
        m.sync()
        assert dd.cpu().numpy()[:n].tobytes() == got[0].tobytes() and dg.cpu().numpy()[:2 * n].tobytes() == got[1].tobytes() and df.cpu().numpy()[:n].tobytes() == got[2].tobytes()
        assert dd[n].item() == -5.0 and dg[2 * n].item() == -5.0 and dg[2 * n + 1].item() == -5.0 and df[n].item() == 0x5a
        assert m.ground_query_sdf(np.zeros((0, 2), np.float32))[0].shape == (0,)                # n == 0


# ---------------------------------------------------------------------------------------------------------- 4. rollouts
def _rollout_scene():
    lab = np.ones((70, 130), np.int8)
    lab[20:40, 30:60] = 2
    lab[50:56, 60:70] = 2
    lab[5:9, 100:125] = 2
    lab[60:66, 5:20] = 0
    return lab


def _fan(T, rng, n=257):
    """n trajectories of T points (cells, fractions) on the 130 x 70 field: the first rows are the special ones, the rest lines, arcs and
    jitter around the blocks, a quarter of them leaving the field"""
    out = np.zeros((n, T, 2))
    for i in range(n):
        start = rng.uniform([2, 2], [127, 67])
        out[i] = arc(start, rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 1.0) * min(1.0, 150.0 / T), rng.uniform(-0.05, 0.05) * min(1.0, 60.0 / T), T)[0]
    out = np.clip(out, -3.0, [132.0, 72.0])
    far, deep, mid = (110.0, 40.0), (45.0, 30.0), (32.3, 30.0)  # far from every obstacle; the middle of the large block; two cells inside it
    # row 0: the minimum tied between a point of the first chunk and one of the second: the first must win
    out[0] = far
    out[0, min(5, T - 1)] = deep
    if T > 70:
        out[0, 69] = deep
    # row 1: first_below and first_in in an earlier chunk than argmin
    out[1] = far
    out[1, min(3, T - 1)] = mid
    if T > 100:
        out[1, 100] = deep
    # rows 2 .. 7: prefixes ending at k = 0, 63, 64 and T - 1, by one point outside the field (the points behind it are answered all the same)
    for r, k in ((2, 0), (3, 63), (4, 64), (5, T - 1)):
        if k < T:
            out[r] = np.clip(out[r], 1.0, [128.0, 68.0])
            out[r, k] = (-5.0, 10.0)
    out[6] = np.clip(out[6], 1.0, [128.0, 68.0])                # complete: the prefix ends at T
    out[7] = np.clip(out[7], 1.0, [128.0, 68.0])
    return out


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 4096])
def test_rollouts_equal_the_reference(T):
    import torch
    size = (130, 70, 1)
    rng = np.random.default_rng(T)
    with Field(size, _rollout_scene()) as fd:
        m, pvt, f, g = fd.m, fd.pvt, fd.f, fd.g
        assert f["inside_dist_sq"].max() >= 100
        xy = _xy(pvt, _fan(T, rng))
        if T > 2:
            xy[7, T // 2:] = np.nan                             # a NaN tail: a shorter trajectory
        if T == 4096:
            cut = rng.integers(0, T, len(xy))                   # (most of the long ones are cut short: the reference is a Python loop)
            for i in range(8, len(xy)):
                if i % 8:
                    xy[i, cut[i]:] = np.nan
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        seen = set()
        for margin in (0.0, 0.35):
            want, wd, wg = S.rollouts(f, g, pvt, W, xy, margin)
            # the special rows are what they were built to be
            if margin > 0:
                assert want["argmin"][0] == min(5, T - 1) and want["min_dist"][0] < -0.5 and want["points"][0] == T
                if T > 100:
                    assert 0 <= want["first_below"][1] < 64 <= want["argmin"][1] and want["first_in"][1] == want["first_below"][1]
                assert [int(want["points"][r]) for r, k in ((2, 0), (3, 63), (4, 64), (5, T - 1)) if k < T] == [k for k in (0, 63, 64, T - 1) if k < T]
                assert want["points"][6] == T and (want["n_below"] > 0).sum() > 20 and (want["first_in"] >= 0).sum() > 10
            else:
                assert (want["n_below"] <= (wd <= 0).sum(axis=1)).all() and ((want["first_below"] >= 0) == (want["n_below"] > 0)).all()
            for n in (1, 3, 257):
                for r0 in (range(0, 8) if n == 1 else range(0, 9, 3) if n == 3 else (0,)):
                    sub = np.ascontiguousarray(xy[r0:r0 + n])
                    rec, dist, grad = m.ground_sdf_rollouts(sub, margin, True, True)
                    assert rec.dtype == RD
                    _same_records(rec, want[r0:r0 + n], (T, n, r0, margin))
                    assert np.array_equal(u32(dist), u32(wd[r0:r0 + n])) and np.array_equal(u32(grad), u32(wg[r0:r0 + n]))
                    seen.add(n)
            # the per-point outputs are the query's on the same points, NaN patterns included
            qd, qg, qf = m.ground_query_sdf(xy.reshape(-1, 2))
            rec, dist, grad = m.ground_sdf_rollouts(xy, margin, True, True)
            assert np.array_equal(u32(dist).ravel(), u32(qd)) and np.array_equal(u32(grad).reshape(-1, 2), u32(qg))
            # the optional outputs NULL in turn, and both
            for d_on, g_on in ((False, True), (True, False), (False, False)):
                r2, d2, g2 = m.ground_sdf_rollouts(xy, margin, d_on, g_on)
                assert r2.tobytes() == want.tobytes() and (d2 is None) == (not d_on) and (g2 is None) == (not g_on)
                assert (d2 is None or d2.tobytes() == wd.tobytes()) and (g2 is None or g2.tobytes() == wg.tobytes())
            # the _dev form, with poisoned tails
            n = len(xy)
            with torch.cuda.stream(st):
                dxy = torch.from_numpy(xy).to(dev)
                dout = torch.full(((n + 1) * 32,), 0x5a, dtype=torch.uint8, device=dev)
                dd = torch.full((n * T + 1,), -5.0, dtype=torch.float32, device=dev)
                dg = torch.full((2 * n * T + 1,), -5.0, dtype=torch.float32, device=dev)
                m.ground_sdf_rollouts_dev(dxy.data_ptr(), n, T, dout.data_ptr(), dd.data_ptr(), dg.data_ptr(), margin)
            m.sync()
            o = dout.cpu().numpy()
            assert o[:n * 32].tobytes() == want.tobytes() and o[n * 32:].tobytes() == P5A * 32
            assert dd.cpu().numpy()[:-1].tobytes() == wd.tobytes() and dg.cpu().numpy()[:-1].tobytes() == wg.tobytes() and dd[-1].item() == -5.0 and dg[-1].item() == -5.0
        assert seen == {1, 3, 257}
        ends = want["points"]
        assert (ends == T).sum() >= 10 and ((ends > 0) & (ends < T)).sum() >= (10 if T > 1 else 0) and (ends == 0).sum() >= 1
        assert len(m.ground_sdf_rollouts(np.zeros((0, 5, 2), np.float32))[0]) == 0                # n == 0
        with pytest.raises(Exception):
            m.ground_sdf_rollouts(np.zeros((1, 4097, 2), np.float32))


# ---------------------------------------------------------------------------------------------------------- 5. nothing else is written
def test_section_calls_change_nothing():
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
            field["blocks"] = k % 4 == 2
            a.ground_compute(field["pvt"][2] + 2, field["pvt"][2] + 9, 2, field["blocks"])
            a.ground_nf1_compute(_xy(field["pvt"], [(24, 20)]), 0, True)
        if phase in ("fuse", "edt", "merge"):
            r = np.random.default_rng(k)
            xy = _xy(field["pvt"], np.stack([arc(r.uniform(0, 40, 2), r.uniform(0, 6.28), r.uniform(0.3, 2.0), 0.05, 70)[0] for _ in range(30)]))
            before = (a.read_ground(), a.read_ground_nf1(), a.ground_rollouts(xy, 1, 16, False, True))
            sdf = a.read_ground_sdf()
            dist, grad, flags = a.ground_query_sdf(xy.reshape(-1, 2))
            rec, d2, g2 = a.ground_sdf_rollouts(xy, 0.2, True, True)
            f = S.field(before[0], size, field["blocks"])
            assert np.array_equal(sdf["inside_dist_sq"], f["inside_dist_sq"]) and rec.tobytes() == S.rollouts(f, before[0], field["pvt"], W, xy, 0.2)[0].tobytes()
            after = (a.read_ground(), a.read_ground_nf1(), a.ground_rollouts(xy, 1, 16, False, True))
            assert all(np.array_equal(before[0][key], after[0][key]) for key in before[0])
            assert np.array_equal(before[1], after[1]) and before[2].tobytes() == after[2].tobytes()

    stage_calls_change_nothing(size, (frame(k) for k in range(5)), _mapper, calls, n_probe=2000)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
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
        hp = lambda off=0: C.c_void_p(host.ctypes.data + off)   # noqa: E731
        dp = lambda off=0: C.c_void_p(dbuf.data_ptr() + off)    # noqa: E731
        xp = xy.ctypes.data_as(C.c_void_p)

        def RP(margin=0.0, flags=0, reserved=None):
            p = _capi.GroundSdfRolloutParam()
            p.margin, p.flags = margin, flags
            if reserved is not None:
                p.reserved[reserved] = 1
            return p

        def unwritten():
            m.sync()
            assert host.tobytes() == P5A * host.size and bool((dbuf == 0x5a).all())

        def read_refused(h, who, outs=True):
            assert f["read_ground_sdf"](h, hp() if outs else None, hp(2048) if outs else None) == INVALID, who
            assert f["read_ground_sdf_dev"](h, dp() if outs else None, dp(2048) if outs else None) == INVALID, who

        def query_refused(h, who, n_=n * T, a=True, outs=True):
            assert f["ground_query_sdf"](h, xp if a else None, n_, hp() if outs else None, hp(1024) if outs else None, hp(2048) if outs else None) == INVALID, who
            assert f["ground_query_sdf_dev"](h, dp(3072) if a else None, n_, dp() if outs else None, dp(1024) if outs else None, dp(2048) if outs else None) == INVALID, who

        def rollouts_refused(h, who, p="default", n_=n, T_=T, a=True, out=True):
            p = RP() if p == "default" else p
            pr = None if p is None else C.byref(p)
            assert f["ground_sdf_rollouts"](h, xp if a else None, n_, T_, pr, hp() if out else None, hp(1024), hp(2048)) == INVALID, who
            assert f["ground_sdf_rollouts_dev"](h, dp(3072) if a else None, n_, T_, pr, dp() if out else None, dp(1024), dp(2048)) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "no ground field yet")):
            read_refused(h, who)
            query_refused(h, who)
            rollouts_refused(h, who)
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 8))                      # a tiled mapper
        read_refused(t._h, "tiled")
        query_refused(t._h, "tiled")
        rollouts_refused(t._h, "tiled")
        unwritten()
        z = pvt[2]
        m.ground_compute(z, z + 7)
        read_refused(m._h, "both outputs null", outs=False)
        query_refused(m._h, "all outputs null", outs=False)
        query_refused(m._h, "all outputs null with n == 0", n_=0, outs=False)
        query_refused(m._h, "n < 0", n_=-1)
        query_refused(m._h, "null xy", a=False)
        rollouts_refused(m._h, "null param", None)
        rollouts_refused(m._h, "null param with n == 0", None, n_=0)
        bad = [RP(-1.0), RP(-1e-30), RP(float("nan")), RP(float("inf")), RP(-float("inf")), RP(flags=1), RP(flags=-2 ** 31)] + [RP(reserved=i) for i in range(6)]
        for p in bad:
            rollouts_refused(m._h, (p.margin, p.flags, list(p.reserved)), p)
        rollouts_refused(m._h, "n < 0", n_=-1)
        for bad_T in (0, -1, 4097, 2 ** 31 - 1):
            rollouts_refused(m._h, "T", T_=bad_T)
            rollouts_refused(m._h, "T with n == 0", n_=0, T_=bad_T)
        rollouts_refused(m._h, "null xy", a=False)
        rollouts_refused(m._h, "null records", out=False)
        unwritten()
        assert "gie_ground_sdf_rollouts_dev" in m._err(), m._err()               # the message names the entry
        # (the same calls with good arguments work; n == 0 is valid with NULL arrays)
        assert f["ground_sdf_rollouts"](m._h, None, 0, 1, C.byref(RP()), None, None, None) == 0
        assert f["ground_sdf_rollouts_dev"](m._h, None, 0, 4096, C.byref(RP()), None, None, None) == 0
        assert f["ground_query_sdf"](m._h, None, 0, hp(), None, None) == 0 and f["ground_query_sdf_dev"](m._h, None, 0, None, None, dp()) == 0
        unwritten()
        assert f["ground_sdf_rollouts"](m._h, xp, n, T, C.byref(RP(1e30)), hp(), None, None) == 0
        rec = host[:32 * n].view(RD)
        assert rec["points"].tolist() == [3] * 4 and rec["n_below"].tolist() == [3] * 4 and rec["first_in"].tolist() == [-1] * 4 and rec["argmin"].tolist() == [0] * 4
        assert host[32 * n:].tobytes() == P5A * (4096 - 32 * n)
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 7. profile
def test_profile_counts_under_ground_and_ground_query():
    import torch
    size = (32, 24, 8)
    lab = np.ones((8, 24, 32), np.int8)
    lab[:, 5:15, 8:20] = 2
    m = _mapper(size)
    try:
        pvt = _settle(m, lab)
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.profile_enable(True)
        m.profile_read()
        xy = _xy(pvt, [[(3, 3), (20, 9)], [(5, 5), (6, 6)]])

        def only(prof, ground, query):
            assert prof["ground"][1] == ground and prof["ground_query"][1] == query, prof
            assert (prof["ground"][0] > 0) == (ground > 0) and (prof["ground_query"][0] > 0) == (query > 0)
            assert all(v[1] == 0 for k, v in prof.items() if k not in ("ground", "ground_query")) and list(prof) == NAMES

        m.ground_query_sdf(xy.reshape(-1, 2))                   # the first call of the section: the inside pass, then the query
        only(m.profile_read(), 1, 1)
        m.ground_query_sdf(xy.reshape(-1, 2))
        m.ground_sdf_rollouts(xy, 0.1, True, True)
        only(m.profile_read(), 0, 2)
        m.read_ground_sdf()
        only(m.profile_read(), 1, 0)
        d = torch.zeros((32 * 24 * 4,), dtype=torch.uint8, device="cuda:0")
        dxy = torch.from_numpy(xy).to("cuda:0")
        m.ground_sdf_rollouts_dev(dxy.data_ptr(), 2, 2, d.data_ptr())
        m.ground_query_sdf_dev(dxy.data_ptr(), 4, d.data_ptr(), 0, 0)
        m.read_ground_sdf_dev(0, d.data_ptr())
        only(m.profile_read(), 1, 2)
        m.ground_sdf_rollouts(np.zeros((0, 2, 2), np.float32))  # n == 0 launches nothing
        m.ground_query_sdf(np.zeros((0, 2), np.float32))
        only(m.profile_read(), 0, 0)
        m.ground_compute(pvt[2], pvt[2] + 7)                    # a compute marks the plane stale: one more inside pass at the next call
        m.profile_read()
        m.ground_sdf_rollouts(xy)
        only(m.profile_read(), 1, 1)
        m.profile_enable(False)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. host layer
def test_host_layer_ground_distance_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_distance_probe")
    size, w, cutoff, gmin, gmax, min_known = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2
    frames, fpath = lidar_frames(tmp_path)
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        m.ground_compute(scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w), min_known)
        pvt = m.pivot()
        rng = np.random.default_rng(8)
        xy = _xy(pvt, rng.uniform(-1.0, [49.0, 41.0], (500, 2)))
        xy[7] = np.nan
        dist, grad, flags = m.ground_query_sdf(xy)
        g = m.read_ground()
        want = S.query(S.field(g, size), g, pvt, w, xy)
        assert np.array_equal(u32(dist), u32(want[0])) and np.array_equal(u32(grad), u32(want[1])) and np.array_equal(flags, want[2])
        assert (flags & 1).sum() > 400 and (flags & 4).sum() > 0 and (flags == 0).sum() > 5
    finally:
        m.close()
    ppath = str(tmp_path / "points.f32")
    xy.tofile(ppath)
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), ppath], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 1 ok 1 points 500 dist 500 grad 1000" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".dist", np.uint8).tobytes() == dist.tobytes() and np.fromfile(out + ".grad", np.uint8).tobytes() == grad.tobytes()
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", ppath], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 ok 0 points 500 dist 3 grad 5" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".dist", np.float32).tolist() == [-7.0] * 3 and np.fromfile(out + ".grad", np.float32).tolist() == [-7.0] * 5

"""The NF1 navigation function on the device (include/gie.h gie_nf1_* / gie_read_nf1* / gie_read_costmap_nf1*) against the numpy
statement of tests/nf1_ref.py, computed from read_local's type and edt at the same point of the mapper's stream."""
import ctypes as C

import numpy as np
import pytest

import nf1_ref
import planner_scenes as ps
from gie import scenes
from gie._capi import CostMapHdr
from stage_common import BoxDrive as _BoxDrive, box_labels as _box_labels, mapper as _mapper, random_boxes as _random_boxes
from stage_common import serpentine_labels, stage_calls_change_nothing, update as _update, world as _world

pytestmark = pytest.mark.gpu


def _flags(unknown, frontiers):
    return (nf1_ref.UNKNOWN_TRAVERSABLE if unknown else 0) | (nf1_ref.FROM_FRONTIERS if frontiers else 0)


def _goals(m, size, rng, k=4):
    """k goals inside the volume, one outside it, one not finite"""
    v = rng.integers(0, np.array(size), size=(k, 3))
    pts = _world(m, v, rng.uniform(-0.4, 0.4, (k, 3)))
    out = _world(m, [[-6, 0, 0], [0, 0, 0]])
    out[1, 0] = np.nan
    return np.concatenate([pts, out])


def _check(m, goals=(), clearance=0.0, unknown=False, frontiers=False, loc=None, exact=True):
    """nf1_compute (clearance in metres) + read_nf1 against the reference on read_local's planes: (field, trav, src, loc)"""
    if loc is None:
        loc = m.read_local(dist_sq=False, coc=False)
    ns = m.nf1_compute(goals, clearance, unknown, frontiers)
    f = m.read_nf1()
    fl = _flags(unknown, frontiers)
    cv = np.float32(clearance) / np.float32(m.cfg.voxel_width)
    trav = nf1_ref.traversable(loc["type"], loc["edt"], cv, fl)
    src = nf1_ref.sources(loc["type"], trav, goals, m.cfg.voxel_width, m.pivot(), fl)
    assert ns == int(src.sum())
    if exact:
        ref = nf1_ref.bfs(trav, src)
        assert np.array_equal(f, ref), int((f != ref).sum())
    else:
        assert nf1_ref.certificate(f, trav, src) == ""
    return f, trav, src, loc


@pytest.mark.parametrize("size", [(96, 80, 72), (97, 61, 45), (77, 53, 1)])
def test_exact_on_random_boxes(size):
    rng = np.random.default_rng(sum(size))
    boxes = _random_boxes(rng, 10, 40, 4, 30)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = _box_labels(scenes.local_pivot(pos, 0.1, size), size, 0, boxes, unknown_slab=5)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        assert (loc["type"] == nf1_ref.FNT).any() and (loc["type"] == nf1_ref.OCCUPIED).any()
        goals = _goals(m, size, rng)
        occ = np.argwhere(loc["type"] == nf1_ref.OCCUPIED)[:1, ::-1]
        goals = np.concatenate([goals, _world(m, occ)])                  # a goal inside an obstacle
        deep = 0
        for cl in (0.0, 0.15, 0.3):                                       # 0, 1.5 and 3 voxels
            for unknown in (False, True):
                for frontiers, g in ((False, goals), (True, ()), (True, goals)):
                    f, _, src, _ = _check(m, g, cl, unknown, frontiers, loc=loc)
                    deep = max(deep, int(f.max()))
        assert deep >= 20
        f, *_ = _check(m, (), 0.0, loc=loc)                               # n == 0 without frontiers: no source
        assert (f == -1).all()
    finally:
        m.close()


@pytest.mark.parametrize("size", ps.RIDER_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_exact_on_solid_scenes_at_flat_thin_and_long_shapes(size):
    """X = 1, Y = 1, a partial last word of the bit rows, 16 words per row, 128 tiles along y or z: the solid scene of
    planner_scenes (never-seen slab, blocks and specks in its free space)"""
    rng = np.random.default_rng(sum(size))
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = ps.solid_labels(size, 12)                              # (a seed at which the reference keeps two clusters or more at every shape)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        assert (loc["type"] == nf1_ref.FNT).any() and (loc["type"] == nf1_ref.OCCUPIED).any() and (loc["type"] == 0).any()
        goals = _goals(m, size, rng)
        reached = 0
        for cl in (0.0, 0.15):                                            # 0 and 1.5 voxels
            for unknown in (False, True):
                for frontiers, g in ((False, goals), (True, ()), (True, goals)):
                    f, _, src, _ = _check(m, g, cl, unknown, frontiers, loc=loc)
                    reached = max(reached, int((f > 0).sum()))
        assert reached > 0
        ax = int(np.argmax(size))
        trav = nf1_ref.traversable(loc["type"], loc["edt"], 0.0, _flags(True, False))
        cells = np.argwhere(trav)[:, ::-1]
        goal = _world(m, cells[np.argsort(cells[:, ax], kind="stable")[:1]])     # ONE goal at the low end of the longest axis
        f, trav, src, _ = _check(m, goal, 0.0, True, False, loc=loc)
        assert src.sum() == 1
        if size[ax] >= 1000:
            assert f.max() >= 500                                         # the field crosses all 16 words / 128 tiles
        reach = np.argwhere(f > 0)[:, ::-1]
        starts = _world(m, reach[rng.choice(len(reach), 20, replace=False)], rng.uniform(-0.3, 0.3, (20, 3)))
        for max_len in (7, int(f.max()) + 2):
            got, glen = m.nf1_path(starts, max_len)
            ref, rlen = nf1_ref.paths(f, starts, m.cfg.voxel_width, m.pivot(), max_len)
            assert np.array_equal(glen, rlen)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b)
        assert (rlen > 0).all()
    finally:
        m.close()


def test_serpentine_maze_thousands_of_levels():
    size, w = (150, 36, 20), 0.125                # corridors cross the 64-voxel words in x and the 8-voxel tiles in y and z
    m = _mapper(size, voxel=w)
    try:
        pos, q = scenes.pose(0, w, delta_vox=0, yaw_deg=0.0)
        lab, cells = serpentine_labels(size)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        goal = _world(m, cells[:1])
        f, trav, src, _ = _check(m, goal, 0.0, loc=loc)
        assert src.sum() == 1 and f.max() >= 20000
        along = f[cells[:, 2], cells[:, 1], cells[:, 0]]
        assert (along >= 0).mean() > 0.99
        f2, *_ = _check(m, goal, 0.15, loc=loc)                           # 1.5 voxels: the corridor is too narrow
        assert (f2 == -1).all()
        f, *_ = _check(m, goal, 0.0, loc=loc)
        starts = _world(m, cells[[-1, len(cells) // 2, 5000]])
        for max_len in (1000, int(f.max()) + 3):
            got, glen = m.nf1_path(starts, max_len)
            ref, rlen = nf1_ref.paths(f, starts, w, m.pivot(), max_len)
            assert np.array_equal(glen, rlen) and rlen[0] > 20000
            for a, b in zip(got, ref):
                assert np.array_equal(a, b)
    finally:
        m.close()


def test_multi_update_drive():
    size = (96, 80, 64)
    d = _BoxDrive(size)
    m = _mapper(size)
    rng = np.random.default_rng(9)
    try:
        for k in range(24):
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
            _check(m, _goals(m, size, rng), (0.0, 0.15, 0.3)[k % 3], k % 2 == 1, k % 4 >= 2)
    finally:
        m.close()


@pytest.mark.parametrize("n", [256, 512])
def test_c5_world(n):
    size, w = (n, n, n), 0.05
    m = _mapper(size, voxel=w, cutoff_dist=2.0)
    try:
        for k in range(2):
            pos, q = scenes.pose(k, w, delta_vox=8, yaw_deg=2.0)
            pvt = scenes.local_pivot(pos, w, size)
            _update(m, pos, q, scenes.hash_world_labels(pvt, size, k).astype(np.int8))
        loc = m.read_local(dist_sq=False, coc=False)
        cv = np.float32(0.1) / np.float32(w)
        trav = nf1_ref.traversable(loc["type"], loc["edt"], cv)
        c = np.array([n // 2] * 3)
        free = np.argwhere(trav[c[2] - 4:c[2] + 4, c[1] - 4:c[1] + 4, c[0] - 4:c[0] + 4])
        assert len(free)
        goal = _world(m, (free[0][::-1] + c - 4)[None, :])
        f, _, src, _ = _check(m, goal, 0.1, loc=loc, exact=n <= 256)
        assert src.sum() == 1 and (f >= 0).mean() > 0.3
    finally:
        m.close()


def _starts(m, f, trav, rng, k=60):
    """k start points at reached voxels, jittered within the voxel, plus an unreachable traversable voxel, an obstacle voxel
    and a point outside the volume"""
    reach = np.argwhere(f > 0)[:, ::-1]
    pick = reach[rng.choice(len(reach), k, replace=False)]
    extra = [np.argwhere(~trav)[:1, ::-1]]
    un = np.argwhere(trav & (f < 0))[:1, ::-1]
    if len(un):
        extra.append(un)
    pts = _world(m, pick, rng.uniform(-0.3, 0.3, (k, 3)))
    return np.concatenate([pts] + [_world(m, e) for e in extra] + [_world(m, [[0, -3, 0]])])


def test_paths_step_for_step():
    size = (96, 80, 72)
    rng = np.random.default_rng(4)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = _box_labels(scenes.local_pivot(pos, 0.1, size), size, 0, _random_boxes(rng, 12, 40, 4, 30))
        for _ in range(2):
            _update(m, pos, q, lab)
        f, trav, _, _ = _check(m, _goals(m, size, rng, 2), 0.15)
        starts = _starts(m, f, trav, rng)
        for max_len in (0, 1, 7, int(f.max()) + 2):
            got, glen = m.nf1_path(starts, max_len)
            ref, rlen = nf1_ref.paths(f, starts, m.cfg.voxel_width, m.pivot(), max_len)
            assert np.array_equal(glen, rlen)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b)
        assert (rlen > 7).any() and (rlen == 0).sum() >= 2
    finally:
        m.close()


def test_costmap_and_the_field_is_kept():
    size = (80, 72, 64)
    d = _BoxDrive(size, seed=4)
    rng = np.random.default_rng(5)
    m = _mapper(size)
    try:
        pos, q, lab = d.frame(0)
        _update(m, pos, q, lab)
        f, trav, _, loc = _check(m, _goals(m, size, rng), 0.15, False, True)
        pay, hdr = m.read_costmap_nf1()
        _, ch = m.read_costmap()
        assert hdr.type == 2 and ch.type == 1
        for k in ("x_size", "y_size", "z_size", "x_origin", "y_origin", "z_origin", "width"):
            assert getattr(hdr, k) == getattr(ch, k), k
        want = np.where(f >= 0, f.astype(np.float32), np.float32(-1.0))
        assert np.array_equal(pay["d"].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(pay["o"], (loc["type"] != 0).astype(np.uint8))
        assert (pay["s"] == 0).all() and (pay["pad"] == 0).all()
        starts = _starts(m, f, trav, rng, 20)
        p0 = m.nf1_path(starts, 60)
        pv = m.pivot()
        for k in range(1, 4):                                             # the map moves and changes; the field stays
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
        assert m.pivot() != pv
        assert np.array_equal(m.read_nf1(), f)
        pay2, hdr2 = m.read_costmap_nf1()
        assert bytes(hdr2) == bytes(hdr) and np.array_equal(pay2.view(np.uint8), pay.view(np.uint8))
        p1 = m.nf1_path(starts, 60)
        assert np.array_equal(p0[1], p1[1]) and all(np.array_equal(a, b) for a, b in zip(p0[0], p1[0]))
    finally:
        m.close()


def test_dev_forms_through_torch():
    import torch
    size = (72, 64, 48)
    d = _BoxDrive(size, seed=6)
    rng = np.random.default_rng(6)
    m = _mapper(size)
    try:
        for k in range(2):
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
        goals = _goals(m, size, rng)
        ns = m.nf1_compute(goals, 0.15, True, True)
        f = m.read_nf1()
        pay, hdr = m.read_costmap_nf1()
        starts = _starts(m, f, f >= 0, rng, 16)
        ph, lh = m.nf1_path(starts, 40)
        assert m.nf1_compute((), 0.0) == 0                                # another field in between
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            dg = torch.from_numpy(goals).to(dev)
            dn = torch.full((1,), -7, dtype=torch.int32, device=dev)
            m.nf1_compute_dev(dg.data_ptr(), len(goals), 0.15, True, True, dn.data_ptr())
            df = torch.empty(size[::-1], dtype=torch.int32, device=dev)
            m.read_nf1_dev(df.data_ptr())
            ds = torch.from_numpy(starts).to(dev)
            dp = torch.zeros((len(starts), 40, 3), dtype=torch.int32, device=dev)
            dl = torch.zeros(len(starts), dtype=torch.int32, device=dev)
            m.nf1_path_dev(ds.data_ptr(), len(starts), 40, dp.data_ptr(), dl.data_ptr())
            dc = torch.empty(int(np.prod(size)) * 8, dtype=torch.uint8, device=dev)
            hd = m.read_costmap_nf1_dev(dc.data_ptr())
        m.sync()
        assert int(dn.cpu().item()) == ns
        assert np.array_equal(df.cpu().numpy(), f)
        assert np.array_equal(dl.cpu().numpy(), lh)
        dpn = dp.cpu().numpy()
        for i, a in enumerate(ph):
            assert np.array_equal(dpn[i, :len(a)], a)
        assert np.array_equal(dc.cpu().numpy(), pay.view(np.uint8).ravel()) and bytes(hd) == bytes(hdr)
    finally:
        m.close()


def test_refusals():
    size = (32, 32, 16)
    m, t = _mapper(size), _mapper(size)
    try:
        f, h = m._f, m._h
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
        out = np.zeros(m.n, np.int32)
        xyz = np.zeros((2, 3), np.float32)
        ln = np.zeros(2, np.int32)
        path = np.zeros((2, 4, 3), np.int32)
        pay = np.zeros(m.n * 8, np.uint8)
        hdr = CostMapHdr()
        # before the first compute
        assert f["read_nf1"](h, ptr(out)) == 1
        assert f["read_nf1_dev"](h, ptr(out)) == 1
        assert f["nf1_path"](h, ptr(xyz), 2, 4, ptr(path), ptr(ln)) == 1
        assert f["nf1_path_dev"](h, None, 0, 0, None, None) == 1
        assert f["read_costmap_nf1"](h, ptr(pay), C.byref(hdr)) == 1
        assert f["read_costmap_nf1_dev"](h, None, None) == 1
        pos, q = scenes.pose(0, 0.1, delta_vox=0, yaw_deg=0.0)
        _update(m, pos, q, np.ones((size[2], size[1], size[0]), np.int8))
        p = m.nf1_param(0.0)
        for bad in (-1.0, float("nan"), float("inf"), -1e-4):
            b = m.nf1_param(0.0)
            b.clearance = bad
            assert f["nf1_compute"](h, None, 0, C.byref(b), None) == 1
        b = m.nf1_param(0.0)
        b.flags = 4
        assert f["nf1_compute"](h, None, 0, C.byref(b), None) == 1
        assert f["nf1_compute"](h, None, -1, C.byref(p), None) == 1
        assert f["nf1_compute"](h, None, 3, C.byref(p), None) == 1
        assert f["nf1_compute"](h, None, 0, None, None) == 1
        assert f["nf1_compute"](None, None, 0, C.byref(p), None) == 1
        assert f["nf1_compute_dev"](h, None, 2, C.byref(p), None) == 1
        assert f["read_nf1"](h, ptr(out)) == 1                            # (nothing refused has made a field)
        assert m.nf1_compute((), 0.0) == 0 and (m.read_nf1() == -1).all()
        assert f["nf1_path"](h, ptr(xyz), -1, 4, ptr(path), ptr(ln)) == 1
        assert f["nf1_path"](h, ptr(xyz), 2, -1, ptr(path), ptr(ln)) == 1
        assert f["nf1_path"](h, ptr(xyz), 2, 4, None, ptr(ln)) == 1
        assert f["nf1_path"](h, ptr(xyz), 0, 4, None, None) == 0
        assert f["read_nf1_dev"](h, None) == 1
        t.set_tile((8, 0, 0), (64, 32, 16))
        th = t._h
        assert f["nf1_compute"](th, None, 0, C.byref(p), None) == 1
        assert f["nf1_compute_dev"](th, None, 0, C.byref(p), None) == 1
        assert f["read_nf1"](th, ptr(out)) == 1
        assert f["nf1_path"](th, ptr(xyz), 2, 4, ptr(path), ptr(ln)) == 1
        assert f["read_costmap_nf1"](th, ptr(pay), C.byref(hdr)) == 1
    finally:
        m.close()
        t.close()


def test_nf1_calls_change_nothing_of_the_map_update():
    size = (80, 64, 64)
    d = _BoxDrive(size, seed=5)

    def calls(a, k, phase, pos):
        if phase == "labels":
            a.nf1_compute(np.array([pos], np.float32), 0.1, k % 2 == 0, True)
        elif phase == "fuse":
            a.nf1_path(np.array([pos], np.float32), 20)
            a.read_costmap_nf1()
        elif phase == "edt":
            a.nf1_compute(np.zeros((3, 3), np.float32), 0.0)
        else:
            a.read_nf1()
    stage_calls_change_nothing(size, (d.frame(k) for k in range(12)), _mapper, calls)


def test_compute_dev_and_another_mappers_updates_on_one_device():
    """the propagation is a grid-barrier launch like the waves: it joins the device's chain of such launches, so one mapper's
    asynchronous compute and another mapper's map updates are never resident half and half (both with a grid of every compute
    unit here): the updates stay exact and nothing times out"""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    msize, w = (150, 36, 20), 0.125
    size = (96, 80, 64)
    d = _BoxDrive(size, seed=8)
    a = _mapper(msize, voxel=w, wave_workgroups=ncu)
    b, c = _mapper(size, wave_workgroups=ncu), _mapper(size)
    try:
        pos, q = scenes.pose(0, w, delta_vox=0, yaw_deg=0.0)
        lab, cells = serpentine_labels(msize)
        for _ in range(2):
            _update(a, pos, q, lab)
        goal = _world(a, cells[:1])
        a.nf1_compute(goal, 0.0)
        want = a.read_nf1()
        assert want.max() >= 20000                                          # (thousands of barrier rounds per compute)
        dev = torch.device("cuda", 0)
        dg = torch.from_numpy(goal).to(dev)
        torch.cuda.synchronize()
        for k in range(6):
            a.nf1_compute_dev(dg.data_ptr(), 1, 0.0)                        # enqueued, not waited for
            pos_k, q_k, lab_k = d.frame(k)
            for m in (b, c):
                _update(m, pos_k, q_k, lab_k)
            lb, lc = b.read_local(), c.read_local()
            for key in lb:
                assert np.array_equal(lb[key], lc[key]), (k, key)
            assert b.stats() == c.stats()
        a.sync()
        assert np.array_equal(a.read_nf1(), want)
    finally:
        a.close()
        b.close()
        c.close()

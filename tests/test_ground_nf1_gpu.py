"""The ground navigation function on the device (include/gie.h "ground navigation function", gie_ground_nf1.inc.h) against the numpy
statement of tests/ground_nf1_ref.py, evaluated on the planes the same mapper's read_ground() returns.  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ground_nf1_ref as N
import ground_ref as R
from gie import _capi, scenes
from ground_common import INVALID, POISON, settle as _settle, ground as _ground, xy as _xy, plane as _plane, serpentine as _serpentine, scene as _scene
from stage_common import ROOT, W, box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
CLEARANCES = (0, 1, 2, 4, 5, 9)
HDR_FIELDS = ("x_size", "y_size", "z_size", "x_origin", "y_origin", "z_origin", "width", "type")
LDS_BUDGET = 144 * 1024                                         # bytes of the three bit planes the propagation keeps in LDS


def _flags(ut, ff):
    return (N.UNKNOWN_TRAVERSABLE if ut else 0) | (N.FROM_FRONTIERS if ff else 0)


def _check(m, g, pvt, goals, csq=0, ut=False, ff=False):
    """compute + read against the reference on the planes g; returns (the field, the number of sources)"""
    goals = np.asarray(goals, np.float32).reshape(-1, 2)
    n = m.ground_nf1_compute(goals, csq, ut, ff)
    nf = m.read_ground_nf1()
    want, n_want = N.field(g, goals, pvt, W, csq, _flags(ut, ff))
    assert n == n_want, (csq, ut, ff, n, n_want)
    assert np.array_equal(nf, want), (csq, ut, ff, int((nf != want).sum()))
    return nf, n


# ---------------------------------------------------------------------------------------------------------- 1. word boundaries
@pytest.mark.parametrize("X", [1, 63, 64, 65, 130])
def test_carries_across_word_boundaries_and_padding_bits(X):
    """corridors along x between walls, the last column a wall: a source at the low end of one and at the high end of another
    (carries in both directions); the corridors without a source stay -1 (a padding bit beyond X that was open or frontier would
    join the rows behind the wall)"""
    size = (X, 9, 2)
    lab = np.full((9, X), 2, np.int8)
    lab[1:8:2, :X - 1] = 1
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        nf, n = _check(m, g, pvt, _xy(pvt, [(0, 1), (max(X - 2, 0), 5)]))
        if X == 1:
            assert n == 0 and (nf == -1).all()
        else:
            assert n == 2 and nf[1, :X - 1].tolist() == list(range(X - 1)) and nf[5, :X - 1].tolist() == list(range(X - 2, -1, -1))
            assert (nf[[0, 2, 3, 4, 6, 7, 8]] == -1).all() and (nf[:, X - 1] == -1).all()
        _check(m, g, pvt, _xy(pvt, [(X // 2, 3), (X // 2, 7)]))         # from the middle: both directions at once
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. depth
def test_a_serpentine_maze_of_thousands_of_levels():
    size = (130, 129, 2)
    lab, cells = _serpentine(size[0], size[1], 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        nf, n = _check(m, g, pvt, _xy(pvt, [cells[0]]))
        assert n == 1 and nf.max() == len(cells) - 1 and len(cells) > 8000
        assert np.array_equal(nf[cells[:, 1], cells[:, 0]], np.arange(len(cells)))
        nf, _ = _check(m, g, pvt, _xy(pvt, [cells[-1], cells[len(cells) // 3]]))
        assert nf.max() == len(cells) // 3
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. clearance
def test_clearances_against_a_pillar_and_a_wall():
    size = (72, 48, 6)
    lab = np.ones((size[2], size[1], size[0]), np.int8)
    lab[1:5, 20:24, 30:34] = 2                                  # a pillar
    lab[:, 8:40, 52] = 2                                        # a wall with a way round either end
    lab[:, :, :5] = 0                                           # never seen
    lab[:, 40:, 60:] = 0
    m = _mapper(size)
    try:
        pvt = _settle(m, lab)
        seen = set()
        for blocks in (False, True):
            g = _ground(m, size, blocks=blocks)
            assert (g["type"] == R.UNKNOWN).any() and (g["type"] == R.FNT).any() and (g["type"] == R.OCCUPIED).any()
            for ut in (False, True):
                for csq in CLEARANCES:
                    nf, n = _check(m, g, pvt, _xy(pvt, [(12, 24), (2, 2)]), csq, ut)
                    seen.add((blocks, ut, csq, n, int((nf >= 0).sum())))
                    if blocks and ut and csq > 0:
                        assert (nf[g["type"] == R.UNKNOWN] == -1).all()       # an UNKNOWN column at distance 0
        reach = {k[:3]: k[4] for k in seen}
        r = [reach[(False, False, c)] for c in CLEARANCES]
        assert r[0] == r[1] > r[2] > r[3] > r[4] > r[5] > 0     # every cell that is not an obstacle is at least 1 away; each larger clearance takes cells
        assert reach[(False, True, 0)] > reach[(False, False, 0)]
    finally:
        m.close()


def test_a_field_without_an_obstacle_column_passes_every_clearance():
    size = (40, 30, 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((2, 30, 40), np.int8))
        g = _ground(m, size)
        assert (g["dist_sq"] == -1).all()
        for csq in (0, 9, 2 ** 31 - 1):
            nf, n = _check(m, g, pvt, _xy(pvt, [(20, 15)]), csq)
            assert n == 1 and nf.min() == 0 and nf.max() == 20 + 15
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. sources
def test_sources():
    import torch
    size = (64, 40, 4)
    pos, lab = _scene(size, 64)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        rng = np.random.default_rng(4)
        cells = np.stack([rng.integers(-3, size[0] + 3, 60), rng.integers(-3, size[1] + 3, 60)], 1)
        occ = np.argwhere(g["type"] == R.OCCUPIED)[:5, ::-1]
        assert len(occ) == 5
        odd = np.array([[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [1e30, 0.0], [0.0, -3e9], [3e9, 3e9]], np.float32)
        sets = {"centres": _xy(pvt, cells), "ties": _xy(pvt, cells, 0.5), "outside": _xy(pvt, [(-1, 0), (size[0], 3), (5, -1), (5, size[1])]),
                "odd": odd, "in obstacles": _xy(pvt, occ), "none": np.zeros((0, 2), np.float32)}
        sets["all"] = np.concatenate(list(sets.values()))
        counts = {}
        for name, xy in sets.items():
            counts[name] = _check(m, g, pvt, xy)[1]
            _check(m, g, pvt, xy, 1, True, True)
        assert counts["centres"] > 10 and counts["ties"] > 10 and counts["all"] > counts["centres"]
        assert counts["outside"] == counts["odd"] == counts["in obstacles"] == counts["none"] == 0
        nf, n_fnt = _check(m, g, pvt, sets["none"], 0, False, True)                  # FROM_FRONTIERS alone
        assert n_fnt == int((g["type"] == R.FNT).sum()) > 0 and (nf[g["type"] == R.FNT] == 0).all()
        # n_sources of the _dev form; a NULL count in both forms
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            d_xy = torch.from_numpy(sets["all"]).to(dev)
            d_n = torch.full((1,), 77, dtype=torch.int32, device=dev)
            d_nf = torch.full((size[0] * size[1],), 77, dtype=torch.int32, device=dev)
            m.ground_nf1_compute_dev(d_xy.data_ptr(), len(sets["all"]), 0, False, False, d_n.data_ptr())
            m.read_ground_nf1_dev(d_nf.data_ptr())
            m.ground_nf1_compute_dev(d_xy.data_ptr(), len(sets["all"]), 0, False, False, 0)
        m.sync()
        assert d_n.item() == counts["all"]
        assert np.array_equal(d_nf.cpu().numpy().reshape(size[1], size[0]), N.field(g, sets["all"], pvt, W)[0])
        p = m.ground_nf1_param()
        assert m._f["ground_nf1_compute"](m._h, None, 0, C.byref(p), None) == 0 and (m.read_ground_nf1() == -1).all()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. paths
def _check_steps(path, ln, nf, pvt, max_len):
    for p, n in zip(path, ln):
        k = min(int(n), max_len)
        c = p[:k] - np.array(pvt[:2])
        if k == 0:
            continue
        v = nf[c[:, 1], c[:, 0]]
        assert v[0] == n - 1 and np.array_equal(v, v[0] - np.arange(k))
        assert (np.abs(np.diff(c, axis=0)).sum(axis=1) == 1).all()
        if n <= max_len:
            assert v[-1] == 0


def test_paths():
    import torch
    size = (64, 40, 4)
    pos, lab = _scene(size, 65)
    m, plain = _mapper(size), _mapper((40, 30, 2))
    try:
        # a plateau: nf = x + (29 - y) from the source (0, 29); from (5, 5) both -x and +y hold the value one less: -x first
        pv = _settle(plain, np.ones((2, 30, 40), np.int8))
        gp = _ground(plain, (40, 30, 2))
        nf, _ = _check(plain, gp, pv, _xy(pv, [(0, 29)]))
        path, ln = plain.ground_nf1_path(_xy(pv, [(5, 5)]), 64)
        assert ln.tolist() == [5 + 24 + 1]
        assert (path[0, :6] - np.array(pv[:2])).tolist() == [[5, 5], [4, 5], [3, 5], [2, 5], [1, 5], [0, 5]] and (path[0, 6] - np.array(pv[:2])).tolist() == [0, 6]
        want, wl = N.path(nf, _xy(pv, [(5, 5)]), pv, W, 64)
        assert np.array_equal(path, want) and np.array_equal(ln, wl)
        # a scene of boxes: random starts, some outside, some in obstacles, some not finite
        pvt = _settle(m, lab, pos)
        g = _ground(m, size)
        nf, n = _check(m, g, pvt, _xy(pvt, [(40, 20), (10, 30)]), 1)
        assert n >= 1 and nf.max() > 20 and (nf == -1).any()
        rng = np.random.default_rng(5)
        cells = np.stack([rng.integers(-3, size[0] + 3, 200), rng.integers(-3, size[1] + 3, 200)], 1)
        starts = np.concatenate([_xy(pvt, cells), _xy(pvt, cells[:50], 0.5), np.array([[np.nan, 0.0], [0.0, np.inf], [1e30, 0.0]], np.float32)])
        for max_len in (1, 4, 128):
            poisoned = np.full((len(starts), max_len, 2), POISON, np.int32)
            path, ln = m.ground_nf1_path(starts, max_len, poisoned.copy())
            want, wl = N.path(nf, starts, pvt, W, max_len, fill=POISON)
            assert np.array_equal(ln, wl) and np.array_equal(path, want)              # beyond min(len, max_len) the poison is intact
            _check_steps(path, ln, nf, pvt, max_len)
            assert (ln == 0).sum() > 10 and (max_len == 128 or (ln > max_len).sum() > 50)
            dev = torch.device("cuda", 0)
            st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
            with torch.cuda.stream(st):
                d_s = torch.from_numpy(starts).to(dev)
                d_p = torch.from_numpy(poisoned).to(dev)
                d_l = torch.full((len(starts),), 77, dtype=torch.int32, device=dev)
                m.ground_nf1_path_dev(d_s.data_ptr(), len(starts), max_len, d_p.data_ptr(), d_l.data_ptr())
            m.sync()
            assert d_p.cpu().numpy().tobytes() == path.tobytes() and d_l.cpu().numpy().tobytes() == ln.tobytes()
        assert m._f["ground_nf1_path"](m._h, None, 0, 4, None, None) == 0 and m._f["ground_nf1_path_dev"](m._h, None, 0, 4, None, None) == 0
    finally:
        m.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------- 6. CostMap
def test_costmap_payload_and_header():
    size = (64, 40, 8)
    pos, lab = _scene(size, 66)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        z_lo, z_hi = pvt[2] + 1, pvt[2] + 5
        m.ground_compute(z_lo, z_hi, 2)
        g = m.read_ground()
        _, ghdr = m.read_costmap_ground()
        nf, _ = _check(m, g, pvt, _xy(pvt, [(40, 20)]), 1)
        pay, hdr = m.read_costmap_ground_nf1()
        want, whdr = N.costmap(nf, g, size, pvt, m.cfg.voxel_width, z_lo)
        assert pay.tobytes() == want.tobytes() and (pay["d"] == -1.0).any() and (pay["o"] == 0).any()
        assert [getattr(hdr, k) for k in HDR_FIELDS] == [whdr[k] for k in HDR_FIELDS] and list(hdr.pad) == [0, 0, 0]
        assert hdr.type == 2 and hdr.z_size == 1
        assert [getattr(hdr, k) for k in HDR_FIELDS[:-1]] == [getattr(ghdr, k) for k in HDR_FIELDS[:-1]]      # the ground CostMap's, but the type
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. lifetime
def test_lifetime_across_map_updates_and_ground_computes():
    import torch
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
        goal = _xy(pvt0, [(30, 24), (50, 10)])
        nf0, _ = _check(m, g0, pvt0, goal, 1, False, True)
        starts = _xy(pvt0, [(5, 5), (60, 40), (33, 20)])
        path0, len0 = m.ground_nf1_path(starts, 96)
        pay0 = m.read_costmap_ground_nf1()[0]
        pvt1 = step(1)
        assert tuple(pvt1) != tuple(pvt0)                        # the update moved the pivot: the field stays at its own
        assert np.array_equal(m.read_ground_nf1(), nf0)
        path1, len1 = m.ground_nf1_path(starts, 96)
        assert np.array_equal(path1, path0) and np.array_equal(len1, len0) and m.read_costmap_ground_nf1()[0].tobytes() == pay0.tobytes()
        # a new ground field invalidates it: every reader refuses and writes nothing
        g1 = _ground(m, size)
        n = size[0] * size[1]
        f = m._f
        host = np.full(8 * n, 0x5a, np.uint8)
        dbuf = torch.full((8 * n,), 0x5a, dtype=torch.uint8, device="cuda:0")
        hdr = _capi.CostMapHdr.from_buffer_copy(bytes([0x5a]) * C.sizeof(_capi.CostMapHdr))
        hp, dp = host.ctypes.data_as(C.c_void_p), C.c_void_p(dbuf.data_ptr())
        sp = starts.ctypes.data_as(C.c_void_p)
        assert f["read_ground_nf1"](m._h, hp) == INVALID and f["read_ground_nf1_dev"](m._h, dp) == INVALID
        assert f["ground_nf1_path"](m._h, sp, 3, 4, hp, hp) == INVALID and f["ground_nf1_path_dev"](m._h, dp, 3, 4, dp, dp) == INVALID
        assert f["read_costmap_ground_nf1"](m._h, hp, C.byref(hdr)) == INVALID and f["read_costmap_ground_nf1_dev"](m._h, dp, C.byref(hdr)) == INVALID
        m.sync()
        assert (host == 0x5a).all() and bool((dbuf == 0x5a).all()) and bytes(hdr) == bytes([0x5a]) * C.sizeof(_capi.CostMapHdr)
        # the next compute follows the new map at the new pivot
        nf1, _ = _check(m, g1, pvt1, goal, 1, False, True)
        assert not np.array_equal(nf1, nf0)
        path2, len2 = m.ground_nf1_path(starts, 96)
        want, wl = N.path(nf1, starts, pvt1, W, 96)
        assert np.array_equal(path2, want) and np.array_equal(len2, wl)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. both storage forms
@pytest.mark.parametrize("size,in_lds", [((512, 768, 1), True), ((512, 769, 1), False)])
def test_a_maze_in_each_storage_form(size, in_lds):
    """three bit planes of 8 * ceil(X / 64) * Y bytes: exactly the LDS budget DESIGN.md 20 states, and one row more"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_ground_nf1.inc.h")).read()
    assert "GIE_GNF1_LDS_BYTES = 144 KiB" in design and re.search(r"#define GIE_GNF1_LDS_BYTES \(144 \* 1024\)", src)
    assert (3 * 8 * ((size[0] + 63) // 64) * size[1] <= LDS_BUDGET) == in_lds
    lab, cells = _serpentine(size[0], size[1], 24)
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        nf, n = _check(m, g, pvt, _xy(pvt, [cells[0]]))
        assert n == 1 and nf.max() == len(cells) - 1 and len(cells) > 16000
        nf, n = _check(m, g, pvt, _xy(pvt, [cells[-1], cells[5000]]))
        assert n == 2
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 9. one stream, one sync
def test_dev_forms_back_to_back_on_the_stream():
    import torch
    size = (64, 40, 8)
    pos, lab = _scene(size, 67)
    m = _mapper(size)
    try:
        pvt = _settle(m, lab, pos)
        z = pvt[2]
        goals = _xy(pvt, [(40, 20), (8, 8)])
        starts = _xy(pvt, np.stack([np.arange(0, 64, 3), np.arange(0, 64, 3) % 40], 1))
        m.ground_compute(z + 1, z + 5, 2, True)
        g = m.read_ground()
        n_host = m.ground_nf1_compute(goals, 2, True, True)
        nf_host = m.read_ground_nf1()
        assert np.array_equal(nf_host, N.field(g, goals, pvt, W, 2, 3)[0])
        path_host, len_host = m.ground_nf1_path(starts, 50)
        pay_host, hdr_host = m.read_costmap_ground_nf1()
        n = size[0] * size[1]
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            d_goals, d_starts = torch.from_numpy(goals).to(dev), torch.from_numpy(starts).to(dev)
            d_n = torch.full((1,), 77, dtype=torch.int32, device=dev)
            d_path = torch.zeros((len(starts) * 50 * 2,), dtype=torch.int32, device=dev)
            d_len = torch.full((len(starts),), 77, dtype=torch.int32, device=dev)
            d_pay = torch.full((8 * n,), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_compute_dev(z + 1, z + 5, 2, True, 0)
            m.ground_nf1_compute_dev(d_goals.data_ptr(), len(goals), 2, True, True, d_n.data_ptr())
            m.ground_nf1_path_dev(d_starts.data_ptr(), len(starts), 50, d_path.data_ptr(), d_len.data_ptr())
            hdr = m.read_costmap_ground_nf1_dev(d_pay.data_ptr())
        m.sync()                                                # the only wait
        assert d_n.item() == n_host and d_len.cpu().numpy().tobytes() == len_host.tobytes()
        assert d_path.cpu().numpy().tobytes() == path_host.tobytes()
        assert d_pay.cpu().numpy().tobytes() == pay_host.tobytes() and bytes(hdr) == bytes(hdr_host)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 10. the update does not notice
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

    def calls(a, k, phase, pos):
        pvt = scenes.local_pivot(pos, W, size)
        goals = _xy(pvt, [(24, 20), (5, 35)])
        if phase == "fuse":                                      # between fuse and merge
            a.ground_compute(pvt[2] + 2, pvt[2] + 9, 2, k % 2 == 1)
            a.ground_nf1_compute(goals, k % 3, True, k % 2 == 0)
            a.read_ground_nf1()
            a.ground_nf1_path(goals[::-1], 40)
        elif phase == "merge":
            a.ground_compute(pvt[2], pvt[2] + 15)
            a.ground_nf1_compute(goals, 4, False, True)
            a.read_costmap_ground_nf1()
            a.ground_nf1_path(_xy(pvt, [(40, 3)]), 200)
    stage_calls_change_nothing(size, (frame(k) for k in range(6)), _mapper, calls, n_probe=2000)


# ---------------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, fresh, t = _mapper(size), _mapper(size), _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        f = m._f
        n = size[0] * size[1]
        P5A = bytes([0x5a])
        host = [np.frombuffer(P5A * (8 * n), np.uint8).copy() for _ in range(3)]
        hdr = _capi.CostMapHdr.from_buffer_copy(P5A * C.sizeof(_capi.CostMapHdr))
        dbuf = torch.full((8 * n,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [(3, 3), (9, 9)])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())
        ns = np.frombuffer(P5A * 4, np.int32).copy()

        def P(**kw):
            p = _capi.GroundNf1Param(0, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert all(a.tobytes() == P5A * a.size for a in host) and ns.tobytes() == P5A * 4
            assert bytes(hdr) == P5A * C.sizeof(_capi.CostMapHdr) and bool((dbuf == 0x5a).all())

        def computes(h, who, p=None):
            p = P() if p is None else p
            assert f["ground_nf1_compute"](h, ptr(xy), 2, C.byref(p), ptr(ns)) == INVALID, who
            assert f["ground_nf1_compute_dev"](h, dp, 2, C.byref(p), dp) == INVALID, who

        def readers(h, who):
            assert f["read_ground_nf1"](h, ptr(host[0])) == INVALID and f["read_ground_nf1_dev"](h, dp) == INVALID, who
            assert f["ground_nf1_path"](h, ptr(xy), 2, 4, ptr(host[1]), ptr(host[2])) == INVALID, who
            assert f["ground_nf1_path_dev"](h, dp, 2, 4, dp, dp) == INVALID, who
            assert f["read_costmap_ground_nf1"](h, ptr(host[0]), C.byref(hdr)) == INVALID, who
            assert f["read_costmap_ground_nf1_dev"](h, dp, C.byref(hdr)) == INVALID, who

        computes(None, "null handle")
        readers(None, "null handle")
        computes(m._h, "before a ground field exists")
        computes(fresh._h, "fresh")
        readers(m._h, "before a ground field exists")
        z = pvt[2]
        m.ground_compute(z, z + 7)
        readers(m._h, "before the first compute")
        for p in [P(clearance_sq=-1), P(clearance_sq=-2 ** 31), P(flags=4), P(flags=7), P(flags=-2 ** 31)] + [P(reserved=i) for i in range(6)]:
            computes(m._h, (p.clearance_sq, p.flags, list(p.reserved)), p)
        assert f["ground_nf1_compute"](m._h, ptr(xy), 2, None, ptr(ns)) == INVALID and f["ground_nf1_compute_dev"](m._h, dp, 2, None, dp) == INVALID
        for name, pts in (("ground_nf1_compute", ptr(xy)), ("ground_nf1_compute_dev", dp)):
            out = ptr(ns) if name == "ground_nf1_compute" else dp
            assert f[name](m._h, pts, -1, C.byref(P()), out) == INVALID and f[name](m._h, None, 2, C.byref(P()), out) == INVALID
        readers(m._h, "every compute so far was refused")
        unwritten()
        # a tiled mapper: all eight refuse
        t.set_tile((8, 0, 0), (64, 24, 8))
        computes(t._h, "tiled")
        readers(t._h, "tiled")
        unwritten()
        # after a compute: max_len < 1, n < 0, NULL arrays, a NULL device payload or field
        assert f["ground_nf1_compute"](m._h, ptr(xy), 2, C.byref(P()), None) == 0
        for name in ("ground_nf1_path", "ground_nf1_path_dev"):
            s, pa, le = (ptr(xy), ptr(host[1]), ptr(host[2])) if name == "ground_nf1_path" else (dp, dp, dp)
            for bad in ((s, 2, 0, pa, le), (s, 2, -3, pa, le), (s, -1, 4, pa, le), (None, 2, 4, pa, le), (s, 2, 4, None, le), (s, 2, 4, pa, None)):
                assert f[name](m._h, *bad) == INVALID, (name, bad[1:3])
        assert f["read_costmap_ground_nf1_dev"](m._h, None, C.byref(hdr)) == INVALID and f["read_ground_nf1_dev"](m._h, None) == INVALID
        unwritten()
        assert f["ground_nf1_path"](m._h, ptr(xy), 2, 4, ptr(host[1]), ptr(host[2])) == 0          # (the same call with good arguments works)
        assert host[2].view(np.int32)[:2].tolist() == [1, 1]     # (both starts are sources of that compute)
    finally:
        for x in (m, fresh, t):
            x.close()


# ---------------------------------------------------------------------------------------------------------- 12. profile
def test_profile_entry():
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        pvt = _settle(m, np.ones((8, 24, 32), np.int8))
        m.profile_enable(True)
        m.profile_read()
        m.ground_compute(pvt[2], pvt[2] + 7)
        m.ground_nf1_compute(_xy(pvt, [(3, 3)]))
        m.read_ground_nf1()                                     # (the host reader is a copy of the plane: no launch, no bracket)
        import torch
        d = torch.zeros((8 * size[0] * size[1],), dtype=torch.uint8, device="cuda:0")
        m.read_ground_nf1_dev(d.data_ptr())
        m.read_costmap_ground_nf1()
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_nf1"][1] == 3 and prof["ground_nf1"][0] > 0 and prof["ground"][1] == 1
        names = list(prof)
        assert names.index("ground_nf1") == names.index("ground") - 1
        assert names.index("ground") == names.index("cloud") - 2 and names[0] == "ogm_classify" and names[-2:] == ["sdf", "sdf_query"]
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 13. at size
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
        nf, n = _check(m, g, pvt, _xy(pvt, [goal]), 9)
        assert n == 1 and nf.max() > 400 and (nf >= 0).sum() > 100000 and (nf == -1).sum() > 5000
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 14. host layer
def test_host_layer_ground_plan_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_plan_probe")
    size, w, cutoff, gmin, gmax, min_known, radius, max_len = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15, 24
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
            nf, n = _check(m, g, pvt, goal, csq, False, bool(ff))
            path, ln = m.ground_nf1_path(start, max_len)
            results[ff] = (path[0, :min(int(ln[0]), max_len)], int(ln[0]), n)
    finally:
        m.close()
    assert results[0][1] > 1 and results[1][2] > results[0][2] >= 1
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    gs = [repr(float(v)) for v in goal.ravel()]
    for ff in (0, 1):
        out = str(tmp_path / ("on%d" % ff))
        res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), repr(radius), str(ff), str(max_len)] + gs,
                             capture_output=True, text=True, timeout=120)
        path, ln, n = results[ff]
        assert res.returncode == 0 and "made 4 points %d" % len(path) in res.stdout, (res.stdout, res.stderr)
        assert np.fromfile(out + ".path", np.int32).tobytes() == path.tobytes()
        assert np.fromfile(out + ".info", np.int32).tolist() == [ln, n, csq]
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", repr(radius), "1", str(max_len)] + gs, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 points 3" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".path", np.int32).tolist() == [POISON] * 6 and np.fromfile(out + ".info", np.int32).tolist() == [0, 0, csq]

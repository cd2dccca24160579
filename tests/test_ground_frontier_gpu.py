"""The ground frontier clusters and the gather of the ground navigation function on the device (include/gie.h "ground frontier
clusters", gie_ground_frontier.inc.h) against the numpy / scipy statement of tests/ground_frontier_ref.py, evaluated on the planes
the same mapper's read_ground() returns.  Every comparison is exact.

FNT cells cannot be written: they come out of the map update (a FREE voxel with an UNKNOWN face neighbour and an obstacle within the
cut-off), so a scene is a label plane, the same on every layer.  In a volume of one or two layers every layer touches the never-seen
space outside the volume: there every free column near an obstacle is FNT, and a scene draws its FNT runs as free cells between walls
(never-seen lines between them join nothing).  With three layers and the band on the middle one only the neighbours in the plane
count: a never-seen cell in free space gives the four-cell ring around it, a never-seen line an arc on either side.  Every scene
asserts FROM THE REFERENCE ALONE that it holds the members, kept and dropped components its case is about before the device is
compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frontier_ref
import ground_frontier_ref as F
import ground_nf1_ref as N
import ground_ref as R
import gie
from gie import _capi, scenes
from ground_common import INVALID, P5A, settle as _settle, plane as _plane, ground as _ground, xy as _xy, framed as _framed, serpentine as _serpentine, chain_scene as _chain_scene
from stage_common import W, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing, update as _update

pytestmark = pytest.mark.gpu
CLEARANCES = (0, 1, 2, 4, 5, 9)
DT = gie.GROUND_FRONTIER_CLUSTER_DTYPE


def _same(got, want):
    """(records, goals, n) of read_ground_frontier_clusters against the reference's dict"""
    rec, goals, n = got
    assert n == want["n_clusters"]
    assert rec.dtype == DT and rec.tobytes() == want["records"].tobytes(), (rec, want["records"])
    assert goals.shape == want["goals"].shape and np.array_equal(goals, want["goals"], equal_nan=True)


def _check(m, g, pvt, csq=0, conn=8, min_size=1, cap=256, members=1, kept=0, dropped=0):
    """the reference's own conditions, then compute + the readers against it; returns the reference's dict"""
    want = F.clusters(g, csq, conn, min_size, cap, pvt, W)
    assert want["n_members"] >= members and want["n_clusters"] >= kept and want["n_dropped"] >= dropped, \
        (csq, conn, min_size, want["n_members"], want["n_clusters"], want["n_dropped"])
    n, cells = m.ground_frontier_compute(csq, min_size, conn, cap)
    assert (n, cells) == (want["n_clusters"], want["n_cells"]), (csq, conn, min_size, cap, n, cells, want["n_clusters"], want["n_cells"])
    labels = m.read_ground_frontier_labels()
    assert np.array_equal(labels, want["labels"]), (csq, conn, min_size, int((labels != want["labels"]).sum()))
    _same(m.read_ground_frontier_clusters(), want)
    return want


# ---------------------------------------------------------------------------------------------------------- 1. word boundaries
def _corridors(X):
    """walls with free rows: row 1 all but the last column (a run across every word boundary); rows 3 and 5 up to the LAST column,
    a wall row between them (set padding bits beyond X would join them); row 7 single cells, one in the last column; rows 2 and 6
    partly never seen"""
    lab = np.full((9, X), 2, np.int8)
    lab[1, :max(X - 1, 1)] = 1
    lab[3, X // 2:] = 1
    lab[5, :] = 1
    lab[5, 40:min(63, X - 1)] = 2                               # (a run that ends at bit 63 or at the last column, another before it)
    lab[7, [min(5, X - 1), X - 1]] = 1
    lab[2, :X // 3] = 0
    lab[6, X // 2:] = 0
    return lab


@pytest.mark.parametrize("X", [1, 63, 64, 65, 130])
def test_runs_across_word_boundaries_and_padding_bits(X):
    size = (X, 9, 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _corridors(X)))
        g = _ground(m, size)
        assert (g["type"][:, X - 1] == R.FNT).sum() >= 3        # FNT cells in the last column
        for conn in (4, 8):
            want = _check(m, g, pvt, 0, conn, 1, 16, members=4, kept=4)
            lab = want["labels"]
            assert lab[3, X - 1] >= 0 and lab[5, X - 1] >= 0 and lab[3, X - 1] != lab[5, X - 1]     # not joined behind the wall
            assert lab[1, 0] == X and lab[1, max(X - 2, 0)] == X                                   # one label all along row 1
            if X > 1:
                assert (lab[1, :X - 1] == X).all() and lab[1, X - 1] == -1
                _check(m, g, pvt, 0, conn, 2, 16, kept=3, dropped=1)
                _check(m, g, pvt, 1, conn, X // 2, 16, kept=2, dropped=1)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. connectivity
def _contacts(X=130, Y=33):
    """in walls: diagonal-only contacts across x = 63 / 64 in both directions; a comb; two arcs one cell apart"""
    lab = np.full((Y, X), 2, np.int8)
    lab[2, 50:64] = 1; lab[3, 64:80] = 1                       # \ across the boundary
    lab[6, 64:80] = 1; lab[7, 50:64] = 1                       # / across the boundary
    lab[10, 63] = 1; lab[11, 64] = 1; lab[12, 63] = 1          # single cells, corner to corner
    lab[15, 3:127] = 1                                          # the comb's spine and its teeth
    lab[16:20, 4:127:2] = 1
    lab[23, 20:110] = 1; lab[25, 20:110] = 1                   # two arcs, a wall row between them
    lab[24, 20] = 0                                             # (never seen: joins nothing)
    return lab


def test_connectivity_across_the_word_boundary():
    size = (130, 33, 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _contacts()))
        g = _ground(m, size)
        w8 = _check(m, g, pvt, 0, 8, 1, 32, kept=5)
        w4 = _check(m, g, pvt, 0, 4, 1, 32, kept=10)
        assert w8["n_clusters"] == 6 and w4["n_clusters"] == 10 and w8["n_cells"] == w4["n_cells"]
        l8, l4 = w8["labels"], w4["labels"]
        assert l8[2, 50] == l8[3, 79] and l4[2, 50] != l4[3, 79]
        assert l8[6, 79] == l8[7, 50] == 6 * 130 + 64 and l4[7, 50] == 7 * 130 + 50
        assert l8[10, 63] == l8[11, 64] == l8[12, 63] and len({l4[10, 63], l4[11, 64], l4[12, 63]}) == 3
        comb = 124 + 4 * 62
        assert (l8[15:20][l8[15:20] >= 0] == 15 * 130 + 3).all() and comb in w8["sizes"].tolist() and comb in w4["sizes"].tolist()
        assert l8[23, 20] != l8[25, 20] and l4[23, 109] != l4[25, 109]
        _check(m, g, pvt, 0, 4, 2, 32, kept=7, dropped=3)
    finally:
        m.close()


def test_one_serpentine_arc_through_every_word_column():
    size = (130, 33, 2)
    lab, cells = _serpentine(size[0], size[1], 2)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        for conn in (4, 8):
            want = _check(m, g, pvt, 0, conn, 1, 4, members=2000, kept=1)
            assert want["n_clusters"] == 1 and want["records"]["size"].tolist() == [len(cells)] and want["records"]["label"].tolist() == [131]
            assert (want["labels"][cells[:, 1], cells[:, 0]] == 131).all()
        _check(m, g, pvt, 0, 8, len(cells) + 1, 4, dropped=1)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. parameter sweep
def _noise_scene(X, Y, seed, slab=5):
    """boxes in free space on the right, random walls / free / never-seen cells on the left, a never-seen slab, a wall frame"""
    rng = np.random.default_rng(seed)
    lab = _framed(X, Y)
    half = X // 2
    lab[1:-1, 1:half] = rng.choice(np.array([1, 2, 0], np.int8), size=(Y - 2, half - 1), p=[0.62, 0.3, 0.08])
    for _ in range(max(4, X * Y // 700)):
        x, y = int(rng.integers(half, X - 6)), int(rng.integers(1, Y - 6))
        lab[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 6))] = 2
    lab[1:-1, half + 6:half + 6 + slab] = 0
    return lab


@pytest.mark.parametrize("size,band", [((48, 40, 4), (1, 2)), ((130, 129, 2), None)])
def test_parameter_sweep(size, band):
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _noise_scene(size[0], size[1], size[0])))
        rich = 0
        for blocks in (False, True):
            g = _ground(m, size, band, blocks)
            assert (g["type"] == R.UNKNOWN).any() and (g["type"] == R.FNT).sum() > 50
            for csq in CLEARANCES:
                for conn in (4, 8):
                    for min_size in (1, 3, 8):
                        want = _check(m, g, pvt, csq, conn, min_size, 64, members=1 if csq <= 1 else 0)     # (with UNKNOWN_BLOCKS an FNT cell is 1 from an obstacle)
                        rich += want["n_clusters"] >= 2 and want["n_dropped"] >= 1
        assert rich >= 20
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. specks
def _specks(X, Y, pitch=4):
    lab = _framed(X, Y)
    lab[2:Y - 2:pitch, 2:X - 2:pitch] = 0
    return lab


def test_specks_far_beyond_the_capacity():
    import torch
    size = (66, 34, 3)
    lab = _specks(size[0], size[1])
    n_specks = int((lab == 0).sum())
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size, (1, 1))
        full = _check(m, g, pvt, 0, 8, 1, 1024, members=4 * n_specks, kept=n_specks)
        assert n_specks > 100 and full["n_clusters"] == n_specks and set(full["sizes"].tolist()) == {4}
        assert _check(m, g, pvt, 0, 4, 1, 1024)["n_clusters"] == 4 * n_specks
        assert _check(m, g, pvt, 0, 8, 5, 8, dropped=n_specks)["n_clusters"] == 0
        f = m._f
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        for cap in (0, 1, n_specks, n_specks + 3):
            want = _check(m, g, pvt, 0, 8, 1, cap)
            have = min(cap, n_specks)
            rec = np.frombuffer(P5A * (64 * (cap + 2)), DT).copy()
            goal = np.frombuffer(P5A * (8 * (cap + 2)), np.float32).copy()
            n = C.c_int32(-7)
            assert f["read_ground_frontier_clusters"](m._h, rec.ctypes.data_as(C.c_void_p), goal.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
            assert n.value == n_specks and rec[:have].tobytes() == full["records"][:have].tobytes()
            assert rec[have:].tobytes() == P5A * (64 * (cap + 2 - have))            # entries beyond the produced ones: as they were
            assert np.array_equal(goal[:2 * cap].reshape(-1, 2), want["goals"], equal_nan=True) and np.isnan(goal[2 * have:2 * cap]).all()
            assert goal[2 * cap:].tobytes() == P5A * 16
            with torch.cuda.stream(st):
                d_rec = torch.full((64 * (cap + 2),), 0x5a, dtype=torch.uint8, device=dev)
                d_goal = torch.full((8 * (cap + 2),), 0x5a, dtype=torch.uint8, device=dev)
                d_n = torch.full((3,), 77, dtype=torch.int32, device=dev)
                m.ground_frontier_compute_dev(0, 1, 8, cap, d_n.data_ptr() + 4)
                m.read_ground_frontier_clusters_dev(d_rec.data_ptr(), d_goal.data_ptr(), d_n.data_ptr())
            m.sync()
            assert d_n.cpu().tolist() == [n_specks, n_specks, 4 * n_specks]
            assert d_rec.cpu().numpy().tobytes() == rec.tobytes() and d_goal.cpu().numpy().tobytes() == goal.tobytes()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. a large component
def _rooms(X, Y, pitch=24):
    """free space with closed 5 x 5 rooms `pitch` apart: ONE large component outside them and a 3 x 3 one inside each"""
    lab = _framed(X, Y)
    for y in range(8, Y - 8, pitch):
        for x in range(8, X - 8, pitch):
            lab[y:y + 5, x:x + 5] = 2
            lab[y + 1:y + 4, x + 1:x + 4] = 1
    return lab


def test_one_large_component_and_hundreds_of_small_ones():
    size = (512, 512, 2)
    lab = _rooms(size[0], size[1])
    m = _mapper(size, cutoff_dist=2.0)
    try:
        pvt = _settle(m, _plane(size, lab))
        g = _ground(m, size)
        want = _check(m, g, pvt, 0, 8, 1, 1024, members=200000, kept=300)
        assert want["sizes"].max() > 200000 and (want["sizes"] == 9).sum() >= 300 and len(want["records"]) == want["n_clusters"]
        _check(m, g, pvt, 0, 4, 10, 1024, kept=1, dropped=300)
        _check(m, g, pvt, 2, 4, 1, 1024, members=100000, kept=300)
        # bit-identical from run to run
        a = m.read_ground_frontier_clusters()[0].tobytes()
        m.ground_frontier_compute(2, 1, 4, 1024)
        assert m.read_ground_frontier_clusters()[0].tobytes() == a
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. the 3-D stage agrees
def test_a_flat_volume_agrees_with_the_3d_frontier_clusters():
    size = (70, 33, 1)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _noise_scene(size[0], size[1], 7)))
        g = _ground(m, size)
        loc = m.read_local(dist_sq=False, coc=False)
        assert np.array_equal(loc["type"][0], g["type"]) and (g["type"] == R.FNT).sum() > 100
        for c2, c3 in ((8, 26), (4, 6)):
            want = _check(m, g, pvt, 0, c2, 2, 256, kept=2, dropped=1)
            n3, v3 = m.frontier_compute(0.0, 2, c3, 256)
            rec3, goal3, _ = m.read_frontier_clusters()
            rec2, goal2, _ = m.read_ground_frontier_clusters()
            assert (n3, v3) == (want["n_clusters"], want["n_cells"]) and len(rec3) == len(rec2) == want["n_clusters"]
            assert np.array_equal(m.read_frontier_labels()[0], m.read_ground_frontier_labels())
            for k in ("label", "size"):
                assert np.array_equal(rec3[k], rec2[k]), k
            for k in ("lo", "hi", "rep", "sum", "centroid"):
                assert rec3[k][:, :2].tobytes() == rec2[k].tobytes(), k
            assert np.array_equal(goal3[:, :2], goal2, equal_nan=True)
            ref3 = frontier_ref.clusters(loc["type"] == R.FNT, c3, 2, 256, pvt, W)
            assert np.array_equal(ref3["labels"][0], want["labels"])
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. the device chain
def test_the_device_chain_with_one_sync():
    import torch
    size = (64, 40, 3)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _chain_scene()))
        g = _ground(m, size, (1, 1))
        cap, csq = 12, 1
        want = F.clusters(g, csq, 8, 2, cap, pvt, W)
        have = want["n_clusters"]
        assert 4 <= have < cap and want["n_dropped"] == 0
        sealed = [i for i, q in enumerate(want["records"]) if 41 <= q["rep"][0] - pvt[0] <= 50 and 6 <= q["rep"][1] - pvt[1] <= 12]
        assert len(sealed) == 1
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        for robot, blocked in (((24, 20), False), ((40, 8), True), ((3, 3), False)):       # free space; inside a wall; free space
            robot_xy = _xy(pvt, [robot])
            steps_want = F.route_steps(g, robot_xy, want["goals"], pvt, W, csq)
            assert (steps_want[have:] == -1).all() and steps_want[sealed[0]] == -1
            assert (steps_want == -1).all() if blocked else (steps_want[:have] >= 0).sum() == have - 1
            with torch.cuda.stream(st):
                d_robot = torch.from_numpy(robot_xy).to(dev)
                d_rec = torch.zeros((64 * cap,), dtype=torch.uint8, device=dev)
                d_goal = torch.zeros((2 * cap,), dtype=torch.float32, device=dev)
                d_cnt = torch.full((4,), 77, dtype=torch.int32, device=dev)        # n_clusters, n_cells, the reader's count, n_sources
                d_zero = torch.full((size[0] * size[1],), 77, dtype=torch.int32, device=dev)
                d_steps = torch.full((cap + 1,), 77, dtype=torch.int32, device=dev)
                m.ground_frontier_compute_dev(csq, 2, 8, cap, d_cnt.data_ptr())
                m.read_ground_frontier_clusters_dev(d_rec.data_ptr(), d_goal.data_ptr(), d_cnt.data_ptr() + 8)
                m.ground_nf1_compute_dev(d_goal.data_ptr(), cap, csq, False, False, d_cnt.data_ptr() + 12)      # the goal array as it is
                m.read_ground_nf1_dev(d_zero.data_ptr())
                m.ground_nf1_compute_dev(d_robot.data_ptr(), 1, csq)
                m.ground_nf1_query_dev(d_goal.data_ptr(), cap, d_steps.data_ptr())
            m.sync()                                            # the only wait
            assert d_cnt.cpu().tolist() == [have, want["n_cells"], have, have]
            assert d_rec.cpu().numpy()[:64 * have].tobytes() == want["records"].tobytes()
            assert np.array_equal(d_goal.cpu().numpy().reshape(-1, 2), want["goals"], equal_nan=True)
            zero = np.argwhere(d_zero.cpu().numpy().reshape(size[1], size[0]) == 0)[:, ::-1] + np.array(pvt[:2])
            assert sorted(map(tuple, zero.tolist())) == sorted(map(tuple, want["records"]["rep"].tolist()))
            steps = d_steps.cpu().numpy()
            assert steps[cap] == 77 and np.array_equal(steps[:cap], steps_want), (steps, steps_want)
            assert np.array_equal(m.ground_nf1_query(want["goals"]), steps_want)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. the gather's inputs
def test_ground_nf1_query_inputs():
    import torch
    size = (64, 40, 3)
    m = _mapper(size)
    try:
        pvt = _settle(m, _plane(size, _chain_scene()))
        g = _ground(m, size, (1, 1))
        m.ground_nf1_compute(_xy(pvt, [(24, 20)]), 1)
        nf = m.read_ground_nf1()
        rng = np.random.default_rng(8)
        cells = np.stack([rng.integers(-3, size[0] + 3, 80), rng.integers(-3, size[1] + 3, 80)], 1)
        odd = np.array([[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [1e30, 0.0], [0.0, -3e9], [3e9, 3e9]], np.float32)
        sets = {"centres": _xy(pvt, cells), "ties": _xy(pvt, cells, 0.5), "outside": _xy(pvt, [(-1, 0), (size[0], 3), (5, -1), (5, size[1])]),
                "odd": odd, "none": np.zeros((0, 2), np.float32)}
        sets["all"] = np.concatenate(list(sets.values()))
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        for name, xy in sets.items():
            want = F.gather(nf, xy, pvt, W)
            host = m.ground_nf1_query(xy)
            assert np.array_equal(host, want), name
            with torch.cuda.stream(st):
                d_xy = torch.from_numpy(np.concatenate([xy, np.zeros((1, 2), np.float32)])).to(dev)
                d_out = torch.full((len(xy) + 1,), 77, dtype=torch.int32, device=dev)
                m.ground_nf1_query_dev(d_xy.data_ptr(), len(xy), d_out.data_ptr())
            m.sync()
            got = d_out.cpu().numpy()
            assert got[:len(xy)].tobytes() == host.tobytes() and got[len(xy)] == 77, name
        assert (F.gather(nf, sets["centres"], pvt, W) >= 0).sum() > 20 and (F.gather(nf, sets["ties"], pvt, W) >= 0).sum() > 20
        assert (F.gather(nf, sets["outside"], pvt, W) == -1).all() and (F.gather(nf, sets["odd"], pvt, W) == -1).all()
        assert m._f["ground_nf1_query"](m._h, None, 0, None) == 0 and m._f["ground_nf1_query_dev"](m._h, None, 0, None) == 0
        assert g["type"].shape == nf.shape
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 9. lifetime
def test_lifetime_invalidation_and_twin_mappers():
    size = (64, 40, 3)
    a, b = _mapper(size), _mapper(size)
    try:
        lab = _plane(size, _chain_scene())
        out = []
        for m in (a, b):
            pvt = _settle(m, lab)
            g = _ground(m, size, (1, 1))
            want = _check(m, g, pvt, 1, 8, 2, 16, kept=4)
            first = (m.read_ground_frontier_labels().tobytes(), m.read_ground_frontier_clusters()[0].tobytes())
            # a map update that moves the pivot does not touch the result
            pos, q = scenes.pose(3, W, delta_vox=4, yaw_deg=0.0)
            _update(m, pos, q, lab)
            assert tuple(m.pivot()) != tuple(pvt)
            assert (m.read_ground_frontier_labels().tobytes(), m.read_ground_frontier_clusters()[0].tobytes()) == first
            _same(m.read_ground_frontier_clusters(), want)
            # two computes in a row on the same ground field: the second one counts
            m.ground_frontier_compute(0, 1, 4, 3)
            _check(m, g, pvt, 0, 4, 1, 16, kept=4)
            # a new ground field invalidates: the three readers refuse until the next compute
            g2 = _ground(m, size, (1, 1))
            pvt2 = m.pivot()
            f, n = m._f, C.c_int32(-7)
            buf = np.frombuffer(P5A * (4 * size[0] * size[1]), np.uint8).copy()
            p = buf.ctypes.data_as(C.c_void_p)
            assert f["read_ground_frontier_labels"](m._h, p) == INVALID and f["read_ground_frontier_clusters"](m._h, p, p, C.byref(n)) == INVALID
            assert f["read_ground_frontier_labels_dev"](m._h, p) == INVALID and f["read_ground_frontier_clusters_dev"](m._h, p, p, p) == INVALID
            assert buf.tobytes() == P5A * buf.size and n.value == -7
            again = _check(m, g2, pvt2, 1, 8, 2, 16, kept=1)
            out.append((first, again["records"].tobytes(), m.read_ground_frontier_labels().tobytes()))
        assert out[0] == out[1]
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------- 10. the update does not notice
def test_section_calls_change_nothing_of_the_map_update():
    from stage_common import box_labels
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

    seen = []

    def calls(a, k, phase, pos):
        pvt = scenes.local_pivot(pos, W, size)
        if phase == "fuse":                                      # between fuse and merge
            a.ground_compute(pvt[2] + 2, pvt[2] + 9, 2, k % 2 == 1)
            n, _ = a.ground_frontier_compute(k % 3, 1 + k % 2, 8 if k % 2 else 4, 32)
            seen.append(n)
            a.read_ground_frontier_labels()
            _, goals, _ = a.read_ground_frontier_clusters()
            a.ground_nf1_compute(_xy(pvt, [(24, 20)]), k % 3)
            a.ground_nf1_query(goals)
        elif phase == "merge":
            a.ground_compute(pvt[2] + 1, pvt[2] + 14)
            seen.append(a.ground_frontier_compute(4, 3, 8, 8)[0])
            a.read_ground_frontier_clusters()
            a.ground_nf1_compute(_xy(pvt, [(40, 3)]), 4)
            a.ground_nf1_query(_xy(pvt, [(5, 35), (24, 20)]))
    stage_calls_change_nothing(size, (frame(k) for k in range(6)), _mapper, calls, n_probe=2000)
    assert len(seen) == 12 and sum(n > 0 for n in seen) >= 6


# ---------------------------------------------------------------------------------------------------------- 11. refusals, profile
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 3)
    m, fresh, t = _mapper(size), _mapper(size), _mapper(size)
    try:
        lab = _framed(size[0], size[1])
        lab[10, 10] = 0
        pvt = _settle(m, _plane(size, lab))
        f = m._f
        n = size[0] * size[1]
        host = [np.frombuffer(P5A * (64 * n), np.uint8).copy() for _ in range(3)]
        dbuf = torch.full((64 * n,), 0x5a, dtype=torch.uint8, device="cuda:0")
        xy = _xy(pvt, [(3, 3), (9, 9)])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())
        cnt = np.frombuffer(P5A * 8, np.int32).copy()
        c0, c1 = C.c_void_p(cnt.ctypes.data), C.c_void_p(cnt.ctypes.data + 4)

        def P(**kw):
            p = _capi.GroundFrontierParam(0, 1, 8, 4)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert all(a.tobytes() == P5A * a.size for a in host) and cnt.tobytes() == P5A * 8 and bool((dbuf == 0x5a).all())

        def computes(h, who, p=None):
            p = P() if p is None else p
            assert f["ground_frontier_compute"](h, C.byref(p), c0, c1) == INVALID, who
            assert f["ground_frontier_compute_dev"](h, C.byref(p), dp) == INVALID, who

        def readers(h, who):
            assert f["read_ground_frontier_clusters"](h, ptr(host[0]), ptr(host[1]), c0) == INVALID, who
            assert f["read_ground_frontier_clusters_dev"](h, dp, dp, dp) == INVALID, who
            assert f["read_ground_frontier_labels"](h, ptr(host[2])) == INVALID and f["read_ground_frontier_labels_dev"](h, dp) == INVALID, who

        def queries(h, who):
            assert f["ground_nf1_query"](h, ptr(xy), 2, ptr(host[0])) == INVALID and f["ground_nf1_query_dev"](h, dp, 2, dp) == INVALID, who

        for h, who in ((None, "null handle"), (m._h, "before a ground field exists"), (fresh._h, "fresh")):
            computes(h, who)
            readers(h, who)
            queries(h, who)
        z = pvt[2]
        m.ground_compute(z + 1, z + 1)
        readers(m._h, "before the first compute")
        queries(m._h, "before the first ground NF1")
        bad = [P(clearance_sq=-1), P(clearance_sq=-2 ** 31), P(min_size=0), P(min_size=-3), P(connectivity=6), P(connectivity=0), P(connectivity=26),
               P(max_clusters=-1), P(flags=1), P(flags=-2 ** 31)] + [P(reserved=i) for i in range(3)]
        for p in bad:
            computes(m._h, (p.clearance_sq, p.min_size, p.connectivity, p.max_clusters, p.flags, list(p.reserved)), p)
        assert f["ground_frontier_compute"](m._h, None, c0, c1) == INVALID and f["ground_frontier_compute_dev"](m._h, None, dp) == INVALID
        readers(m._h, "every compute so far was refused")
        unwritten()
        t.set_tile((8, 0, 0), (64, 24, 3))                      # a tiled mapper: all eight refuse
        computes(t._h, "tiled")
        readers(t._h, "tiled")
        queries(t._h, "tiled")
        unwritten()
        # after a compute: both cluster outputs NULL, a NULL label plane; after a ground NF1: n < 0, NULL arrays
        assert f["ground_frontier_compute"](m._h, C.byref(P()), None, None) == 0
        assert f["read_ground_frontier_clusters"](m._h, None, None, c0) == INVALID and f["read_ground_frontier_clusters_dev"](m._h, None, None, dp) == INVALID
        assert f["read_ground_frontier_labels"](m._h, None) == INVALID and f["read_ground_frontier_labels_dev"](m._h, None) == INVALID
        m.ground_nf1_compute(xy)
        for name, a, o in (("ground_nf1_query", ptr(xy), ptr(host[0])), ("ground_nf1_query_dev", dp, dp)):
            assert f[name](m._h, a, -1, o) == INVALID and f[name](m._h, None, 2, o) == INVALID and f[name](m._h, a, 2, None) == INVALID, name
        unwritten()
        m.ground_compute(z + 1, z + 1)                          # the ground NF1 field and the clusters are of the planes just overwritten
        readers(m._h, "invalidated")
        queries(m._h, "invalidated")
        unwritten()
        # the same calls with good arguments work, a NULL record array or goal array alone is fine
        assert f["ground_frontier_compute"](m._h, C.byref(P()), c0, c1) == 0 and cnt.tolist() == [1, 4]
        assert f["read_ground_frontier_clusters"](m._h, ptr(host[0]), None, None) == 0 and f["read_ground_frontier_clusters"](m._h, None, ptr(host[1]), None) == 0
        rec = host[0][:64].view(DT)[0]
        assert rec["size"] == 4 and rec["label"] == 9 * 32 + 10 and host[0][64:].tobytes() == P5A * (host[0].size - 64)
        assert np.array_equal(host[1][:8].view(np.float32), (rec["rep"].astype(np.float32) * np.float32(W))) and np.isnan(host[1][8:32].view(np.float32)).all()
    finally:
        for x in (m, fresh, t):
            x.close()


def test_profile_entry_and_its_place():
    import torch
    size = (32, 24, 3)
    m = _mapper(size)
    try:
        lab = _framed(size[0], size[1])
        lab[10, 10] = 0
        pvt = _settle(m, _plane(size, lab))
        m.profile_enable(True)
        before = list(m.profile_read())
        assert "ground_frontier" not in before                  # a mapper that has not called the section: the list as it was
        m.ground_compute(pvt[2] + 1, pvt[2] + 1)
        assert m.ground_frontier_compute(0, 1, 8, 4) == (1, 4)
        m.read_ground_frontier_labels()
        m.read_ground_frontier_clusters()
        with torch.cuda.stream(torch.cuda.ExternalStream(m.stream_handle(), device=torch.device("cuda", 0))):
            d = torch.zeros((4 * size[0] * size[1],), dtype=torch.uint8, device="cuda:0")
            m.read_ground_frontier_labels_dev(d.data_ptr())
        m.ground_nf1_compute(_xy(pvt, [(3, 3)]))
        m.ground_nf1_query(_xy(pvt, [(5, 5)]))
        m.ground_nf1_query(np.zeros((0, 2), np.float32))       # n == 0 launches nothing
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground_frontier"][1] == 4 and prof["ground_frontier"][0] > 0
        assert prof["ground_nf1"][1] == 2 and prof["ground"][1] == 1
        names = list(prof)
        assert names.index("ground_frontier") == names.index("ground_nf1") - 1 == names.index("ground") - 2
        assert names[0] == "ogm_classify" and names[-2:] == ["sdf", "sdf_query"]
        assert [x for x in names if x != "ground_frontier"] == before
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 12. host layer
def test_host_layer_ground_exploration_goals_matches_the_mapper(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = build_host_probe(tmp_path, "ground_explore_probe", ["-DGIE_HOST_WITH_HIP", "-I" + os.path.join(rocm, "include"), "-Wno-unused-result",
                                                              "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    size, w, cutoff, gmin, gmax, min_known, radius, cap, min_size = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2, 0.15, 24, 2
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
        want = _check(m, g, pvt, csq, 8, min_size, cap, kept=2)
        robot = np.array([frames[-1][0][:2]], np.float32)
        steps_want = F.route_steps(g, robot, want["goals"], pvt, w, csq)
        m.ground_nf1_compute(robot, csq)
        steps = m.ground_nf1_query(want["goals"])
        assert np.array_equal(steps, steps_want) and (steps >= 0).any()
        have = len(want["records"])
    finally:
        m.close()
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known), repr(radius), str(cap), str(min_size)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 clusters %d steps %d" % (have, have) in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == want["records"].tobytes()
    assert np.fromfile(out + ".steps", np.int32).tolist() == steps[:have].tolist()
    assert np.fromfile(out + ".info", np.int32).tolist() == [want["n_clusters"], want["n_cells"], csq]
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1", repr(radius), str(cap), str(min_size)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 clusters 2 steps 3" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".rec", np.uint8).tobytes() == P5A * 128 and np.fromfile(out + ".steps", np.uint8).tobytes() == P5A * 12
    assert np.fromfile(out + ".info", np.int32).tolist() == [0, 0, csq]

"""The frontier clusters on the device (include/gie.h gie_frontier_compute* / gie_read_frontier_*) against the numpy / scipy
statement of tests/frontier_ref.py.  The members are computed by the reference from read_local's type and edt taken at the same
point of the mapper's stream; every comparison is bit for bit: the label plane, the counts, every field of every record, the goal
array.  The C5 hash world is compared whole at 256^3 and at 512^3 (no slab stand-in was needed)."""
import ctypes as C

import numpy as np
import pytest

import frontier_ref as fr
import planner_scenes as ps
from gie import scenes
from stage_common import BoxDrive as _BoxDrive, bits as _bits, box_labels as _box_labels, mapper as _mapper, random_boxes as _random_boxes
from stage_common import serpentine_cells, stage_calls_change_nothing, update as _update

pytestmark = pytest.mark.gpu


def _pocket(lab, x0, y0, z0, inner, unknown):
    """a closed room (local voxels): occupied walls one voxel thick around `inner` free voxels, `unknown` never-seen voxels in its
    middle; clipped to the volume (a flat volume has no floor and ceiling to clip)"""
    Z, Y, X = lab.shape
    ix, iy, iz = inner
    z1 = min(z0 + iz + 2, Z)
    lab[z0:z1, y0:y0 + iy + 2, x0:x0 + ix + 2] = 2
    zi0, zi1 = (z0 + 1, z0 + 1 + iz) if Z > 1 else (0, 1)
    lab[zi0:zi1, y0 + 1:y0 + 1 + iy, x0 + 1:x0 + 1 + ix] = 1
    ux, uy, uz = unknown
    cx, cy, cz = x0 + 1 + (ix - ux) // 2, y0 + 1 + (iy - uy) // 2, zi0 + (zi1 - zi0 - min(uz, zi1 - zi0)) // 2
    lab[cz:cz + min(uz, zi1 - zi0), cy:cy + uy, cx:cx + ux] = 0


def _check(m, clearance=0.0, conn=26, min_size=1, cap=256, loc=None):
    """frontier_compute (clearance in metres) + the readers against the reference on read_local's planes: the reference's result"""
    if loc is None:
        loc = m.read_local(dist_sq=False, coc=False)
    nc, nv = m.frontier_compute(clearance, min_size, conn, cap)
    labels = m.read_frontier_labels()
    rec, goal, n = m.read_frontier_clusters()
    cv = np.float32(clearance) / np.float32(m.cfg.voxel_width)
    ref = fr.clusters(fr.members(loc["type"], loc["edt"], cv), conn, min_size, cap, m.pivot(), m.cfg.voxel_width)
    assert np.array_equal(labels, ref["labels"]), int((labels != ref["labels"]).sum())
    assert (nc, nv, n) == (ref["n_clusters"], ref["n_voxels"], ref["n_clusters"])
    assert rec.dtype == fr.CLUSTER_DTYPE and len(rec) == len(ref["records"])
    for k in rec.dtype.names:
        assert np.array_equal(_bits(rec[k]), _bits(ref["records"][k])), k
    assert rec.tobytes() == ref["records"].tobytes()
    assert goal.shape == ref["goals"].shape and np.array_equal(_bits(goal), _bits(ref["goals"]))
    return ref


@pytest.mark.parametrize("size", [(96, 80, 72), (97, 61, 45), (77, 53, 1), (48, 40, 33)])
def test_exact_on_random_boxes(size):
    rng = np.random.default_rng(sum(size))
    boxes = _random_boxes(rng, 10, 40, 4, 30)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = _box_labels(scenes.local_pivot(pos, 0.1, size), size, 0, boxes, unknown_slab=5)
        zc = max(size[2] // 2 - 5, 0)
        _pocket(lab, 18, 18, zc, (7, 7, 7), (3, 3, 3))                   # a large frontier shell in a closed room: kept
        _pocket(lab, 34, 8, zc, (3, 1, 1), (1, 1, 1))                    # two single frontier voxels in a closed room: noise
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        scene = fr.clusters(fr.members(loc["type"], loc["edt"], 0.0), 26, 8, 0)
        assert scene["n_clusters"] >= 2 and (scene["labels"] == -2).any()      # >= 2 kept and >= 1 filtered: not an empty set
        kept = 0
        for cl in (0.0, 0.15, 0.3):                                       # 0, 1.5 and 3 voxels
            for conn in (6, 26):
                for min_size in (1, 8, 200):
                    kept += _check(m, cl, conn, min_size, 64, loc=loc)["n_clusters"]
        assert kept >= 4
    finally:
        m.close()


@pytest.mark.parametrize("size", ps.RIDER_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_exact_on_solid_scenes_at_flat_thin_and_long_shapes(size):
    """X = 1, Y = 1, a partial last word of the bit rows, 16 words per row, 128 tiles along y or z: the solid scene of
    planner_scenes, whose never-seen slab and blocks of side 3 give clusters of more than eight voxels at either connectivity"""
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = ps.solid_labels(size, 12)                              # (a seed at which the reference keeps two clusters or more at every shape)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        for conn in (6, 26):
            for min_size in (1, 8):
                assert _check(m, 0.0, conn, min_size, 64, loc=loc)["n_clusters"] >= 2      # (never two empty sets)
        _check(m, 0.15, 26, 1, 3, loc=loc)
    finally:
        m.close()


def _free_space(size):
    """labels of a free volume with a lattice of single occupied voxels (z and y multiples of 4, x of 8): obtainFrontiers marks a
    free voxel FNT only when its closest obstacle lies inside the volume, so free space needs obstacles within the cutoff; the
    never-seen shapes of the tests below sit at coordinates that are 2 modulo 4, two voxels away from every post"""
    lab = np.ones(size[::-1], np.int8)
    lab[0::4, 0::4, 0::8] = 2
    return lab


def _shape_scene(m, size, w, unknown_cells=None, lab=None):
    pos, q = scenes.pose(0, w, delta_vox=0, yaw_deg=0.0)
    if lab is None:
        lab = _free_space(size)
        lab[unknown_cells[:, 2], unknown_cells[:, 1], unknown_cells[:, 0]] = 0
    for _ in range(2):
        _update(m, pos, q, lab)
    return m.read_local(dist_sq=False, coc=False)


def test_serpentine_tube_is_one_component_across_every_border():
    size, w = (128, 128, 24), 0.125
    m = _mapper(size, voxel=w)
    try:
        cells = serpentine_cells(size, 4, 2)
        loc = _shape_scene(m, size, w, cells)
        assert (loc["type"][cells[:, 2], cells[:, 1], cells[:, 0]] == fr.UNKNOWN).all()
        ref = _check(m, 0.0, 26, 1, 16, loc=loc)
        assert ref["records"]["size"].max() >= 2 * len(cells) and len(cells) > 15000     # the tube's shell
        side = loc["type"][cells[:, 2], cells[:, 1] + 1, cells[:, 0]] == fr.FNT          # (not where the tube itself turns into +y)
        shell = ref["labels"][cells[side, 2], cells[side, 1] + 1, cells[side, 0]]
        assert side.mean() > 0.9 and (shell == shell[0]).all() and shell[0] >= 0         # ONE label all along the tube
        for conn, min_size in ((6, 1), (6, 50), (26, 100000)):
            _check(m, 0.0, conn, min_size, 16, loc=loc)
    finally:
        m.close()


def test_comb_sheets_and_edge_contacts():
    size, w = (136, 72, 40), 0.1
    m = _mapper(size, voxel=w)
    try:
        lab = _free_space(size)
        lab[20, 6, 4:132] = 0                                            # the comb: a spine along x ...
        for x in range(6, 130, 4):
            lab[20, 7:60, x] = 0                                         # ... and a tooth every fourth column
        lab[4:16, 4:30, 60:69] = 2                                       # a solid block around x = 63 / 64 ...
        lab[5:15, 5:29, 61:68] = 1                                       # ... hollow ...
        lab[6:14, 6:28, 64] = 0                                          # ... with a never-seen plate across it: two sheets one voxel apart
        lab[5:15, 5:29, 64][lab[5:15, 5:29, 64] == 1] = 2                # (the plate's rim is wall: the sheets do not meet around it)
        lab[30, 10, 10] = lab[30, 12, 12] = 0                            # two never-seen voxels whose shells touch by edges only
        loc = _shape_scene(m, size, w, lab=lab)
        r26 = _check(m, 0.0, 26, 1, 64, loc=loc)
        r6 = _check(m, 0.0, 6, 1, 64, loc=loc)
        for r in (r26, r6):
            a, b = r["labels"][8, 10, 63], r["labels"][8, 10, 65]
            assert a >= 0 and b >= 0 and a != b                          # the two sheets: separate at 6 and at 26
        assert r26["labels"][30, 10, 11] == r26["labels"][30, 11, 12] >= 0       # edge contact: one component at 26 ...
        assert r6["labels"][30, 10, 11] != r6["labels"][30, 11, 12]              # ... two at 6
        _check(m, 0.0, 26, 30, 3, loc=loc)
        _check(m, 0.1, 6, 2, 64, loc=loc)
    finally:
        m.close()


def test_checkerboard_of_tens_of_thousands_of_components():
    size, w = (192, 160, 64), 0.1
    m = _mapper(size, voxel=w)
    try:
        lab = _free_space(size)
        lab[2:-2:4, 2:-2:4, 2:-2:4] = 0
        loc = _shape_scene(m, size, w, lab=lab)
        ref = _check(m, 0.0, 26, 1, 100, loc=loc)
        assert ref["n_clusters"] >= 20000 and len(ref["records"]) == 100          # (15 x 39 x 47 specks, less those by the faces)
        assert _check(m, 0.0, 26, 6, 7, loc=loc)["n_clusters"] >= 20000
        assert _check(m, 0.0, 6, 1, 1000, loc=loc)["n_clusters"] >= 120000        # six single voxels per speck
        _check(m, 0.0, 26, 7, 100, loc=loc)
    finally:
        m.close()


def test_capacity():
    size = (80, 72, 40)
    m = _mapper(size)
    try:
        pos, q, lab = _BoxDrive(size, seed=7).frame(0)
        lab[10:30:4, 10:60:4, 10:70:4] = 0                               # never-seen specks: many small components
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        full = _check(m, 0.0, 26, 2, 4096, loc=loc)
        kept = full["n_clusters"]
        assert kept >= 8
        for cap in (0, 1, kept - 1, kept, kept + 5):
            ref = _check(m, 0.0, 26, 2, cap, loc=loc)
            assert ref["n_clusters"] == kept and ref["n_voxels"] == full["n_voxels"]
            assert ref["records"].tobytes() == full["records"][:cap].tobytes()
            assert np.isnan(ref["goals"][kept:]).all() and ref["goals"].shape == (cap, 3)
    finally:
        m.close()


def test_multi_update_drive():
    size = (96, 80, 64)
    d = _BoxDrive(size)
    m = _mapper(size)
    try:
        total = 0
        for k in range(24):
            pos, q, lab = d.frame(k)
            lab[8:56:8, 8:72:8, 12 + k:90:8] = 0                          # specks that move through the volume
            _update(m, pos, q, lab)
            total += _check(m, (0.0, 0.15, 0.3)[k % 3], (26, 6)[k % 2], (1, 4, 30)[k % 3], (64, 3, 500)[k % 3])["n_clusters"]
        assert total >= 48
    finally:
        m.close()


def test_stream_enabled_update_and_ray_cast_update():
    size = (80, 72, 64)
    d = _BoxDrive(size, seed=4)
    m = _mapper(size)
    try:
        m.stream_enable(True)
        pos, q, lab = d.frame(0)
        _update(m, pos, q, lab)
        assert _check(m, 0.0, 26, 1, 64)["n_clusters"] >= 1
        m.stream_changed()
        # a ray-cast update: a point cloud of a solid block ahead of the sensor (sensor frame = world axes, yaw 0)
        g = np.arange(0.0, 1.2, 0.05, dtype=np.float32)
        blk = np.stack(np.meshgrid(g + 1.5, g - 0.6, g - 0.6, indexing="ij"), -1).reshape(-1, 3)
        m.set_pose(pos, q)
        m.ogm_pointcloud(blk)
        m.step()
        assert _check(m, 0.0, 26, 2, 64)["n_clusters"] >= 1
        _check(m, 0.1, 6, 1, 64)
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
        assert (loc["type"] == fr.FNT).any()
        _check(m, 0.0, 26, 8, 256, loc=loc)
        _check(m, 0.1, 26, 8, 256, loc=loc)                                # 2 voxels
        if n <= 256:
            _check(m, 0.0, 6, 1, 1000, loc=loc)
    finally:
        m.close()


def test_chain_to_nf1_on_the_device():
    import torch
    size, cap = (96, 80, 64), 40
    d = _BoxDrive(size, seed=6)
    m = _mapper(size)
    try:
        pos, q, lab = d.frame(0)
        lab[8:56:8, 8:72:8, 12:90:8] = 0                                  # never-seen specks (the same voxels in both updates)
        for _ in range(2):
            _update(m, pos, q, lab)
        for cl, kw in ((0.0, {}), (0.15, {}), (0.15, dict(from_frontiers=True))):
            dev = torch.device("cuda", 0)
            st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
            with torch.cuda.stream(st):
                dg = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
                dn = torch.full((1,), -7, dtype=torch.int32, device=dev)
                m.frontier_compute_dev(cl, 3, 26, cap)
                m.read_frontier_clusters_dev(0, dg.data_ptr(), 0)
                m.nf1_compute_dev(dg.data_ptr(), cap, cl, d_n_sources=dn.data_ptr(), **kw)
            m.sync()
            rec, goal, n = m.read_frontier_clusters()
            f = m.read_nf1()
            assert 3 <= len(rec) <= cap and np.array_equal(_bits(dg.cpu().numpy()), _bits(goal))
            rep = np.unique(rec["rep"], axis=0) - np.array(m.pivot())
            zero = np.zeros(f.shape, bool)
            zero[rep[:, 2], rep[:, 1], rep[:, 0]] = True
            if kw:
                loc = m.read_local(dist_sq=False, coc=False)
                zero |= fr.members(loc["type"], loc["edt"], np.float32(cl) / np.float32(m.cfg.voxel_width))
            assert int(dn.cpu().item()) == int(zero.sum())
            assert np.array_equal(f == 0, zero)
    finally:
        m.close()


def test_result_stays_with_its_pivot_and_two_computes_in_a_row():
    size = (80, 72, 64)
    d = _BoxDrive(size, seed=4)
    m = _mapper(size)
    try:
        pos, q, lab = d.frame(0)
        lab[8:56:8, 8:64:8, 12:70:8] = 0
        _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        big = _check(m, 0.0, 26, 1, 512, loc=loc)                         # many records, many sizes ...
        ref = _check(m, 0.15, 6, 5, 7, loc=loc)                           # ... must leave nothing behind for this one
        assert big["n_clusters"] > ref["n_clusters"]
        labels = m.read_frontier_labels()
        rec, goal, n = m.read_frontier_clusters()
        pv = m.pivot()
        for k in range(1, 4):                                             # the map moves and changes; the result stays
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
        assert m.pivot() != pv
        assert np.array_equal(m.read_frontier_labels(), labels)
        rec2, goal2, n2 = m.read_frontier_clusters()
        assert n2 == n and rec2.tobytes() == rec.tobytes() and np.array_equal(_bits(goal2), _bits(goal))
        assert rec2.tobytes() == ref["records"].tobytes()                 # (global coordinates of the compute's pivot)
        _check(m, 0.0, 26, 1, 512)
    finally:
        m.close()


def test_frontier_calls_change_nothing_of_the_map_update():
    size = (80, 64, 64)
    d = _BoxDrive(size, seed=5)

    def calls(a, k, phase, pos):
        if phase == "labels":
            a.frontier_compute(0.1, 2, 26, 16)
        elif phase == "fuse":
            a.read_frontier_clusters()
            a.frontier_compute(0.0, 1, 6, 300)
        elif phase == "edt":
            a.read_frontier_labels()
        else:
            a.frontier_compute(0.2, 8, 26, 0)
    stage_calls_change_nothing(size, (d.frame(k) for k in range(12)), _mapper, calls)


def test_dev_forms_through_torch():
    import torch
    size, cap = (72, 64, 48), 10
    d = _BoxDrive(size, seed=6)
    m = _mapper(size)
    try:
        pos, q, lab = d.frame(0)
        lab[8:40:8, 8:56:8, 12:66:8] = 0                                  # never-seen specks (the same voxels in both updates)
        for _ in range(2):
            _update(m, pos, q, lab)
        ref = _check(m, 0.15, 26, 2, cap)
        labels = m.read_frontier_labels()
        rec, goal, n = m.read_frontier_clusters()
        assert n > cap
        m.frontier_compute(0.0, 1, 6, 3)                                  # another result in between
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            dc = torch.full((2,), -7, dtype=torch.int32, device=dev)
            m.frontier_compute_dev(0.15, 2, 26, cap, dc.data_ptr())
            dl = torch.empty(size[::-1], dtype=torch.int32, device=dev)
            m.read_frontier_labels_dev(dl.data_ptr())
            dr = torch.zeros(cap * 80, dtype=torch.uint8, device=dev)
            dg = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
            dn = torch.full((1,), -7, dtype=torch.int32, device=dev)
            m.read_frontier_clusters_dev(dr.data_ptr(), dg.data_ptr(), dn.data_ptr())
        m.sync()
        assert dc.cpu().tolist() == [ref["n_clusters"], ref["n_voxels"]] and int(dn.cpu().item()) == n
        assert np.array_equal(dl.cpu().numpy(), labels)
        assert dr.cpu().numpy().tobytes() == rec.tobytes()
        assert np.array_equal(_bits(dg.cpu().numpy()), _bits(goal))
    finally:
        m.close()


def test_refusals():
    size = (32, 32, 16)
    m, t = _mapper(size), _mapper(size)
    try:
        f, h = m._f, m._h
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
        out = np.zeros(m.n, np.int32)
        rec = np.zeros(8, fr.CLUSTER_DTYPE)
        goal = np.zeros((8, 3), np.float32)
        n = C.c_int32(0)
        # before the first compute
        assert f["read_frontier_labels"](h, ptr(out)) == 1
        assert f["read_frontier_labels_dev"](h, ptr(out)) == 1
        assert f["read_frontier_clusters"](h, ptr(rec), ptr(goal), C.byref(n)) == 1
        assert f["read_frontier_clusters_dev"](h, None, None, None) == 1
        pos, q = scenes.pose(0, 0.1, delta_vox=0, yaw_deg=0.0)
        _update(m, pos, q, np.ones((size[2], size[1], size[0]), np.int8))
        good = m.frontier_param(0.0, 1, 26, 8)

        def bad(**kw):
            p = m.frontier_param(0.0, 1, 26, 8)
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        for p in (bad(connectivity=18), bad(connectivity=0), bad(min_size=0), bad(min_size=-3), bad(clearance=-1.0),
                  bad(clearance=-1e-4), bad(clearance=float("nan")), bad(clearance=float("inf")), bad(max_clusters=-1)):
            assert f["frontier_compute"](h, C.byref(p), None, None) == 1
            assert f["frontier_compute_dev"](h, C.byref(p), None) == 1
        assert f["frontier_compute"](h, None, None, None) == 1
        assert f["frontier_compute_dev"](h, None, None) == 1
        assert f["frontier_compute"](None, C.byref(good), None, None) == 1
        assert f["read_frontier_labels"](h, ptr(out)) == 1                # (nothing refused has made a result)
        nc, nv = m.frontier_compute(0.0, 1, 26, 8)
        lab = m.read_frontier_labels()
        assert nv == int((lab >= 0).sum()) and f["read_frontier_clusters"](h, ptr(rec), ptr(goal), C.byref(n)) == 0 and n.value == nc
        assert f["read_frontier_labels_dev"](h, None) == 1
        assert f["read_frontier_clusters"](h, None, None, None) == 0
        t.set_tile((8, 0, 0), (64, 32, 16))
        th = t._h
        assert f["frontier_compute"](th, C.byref(good), None, None) == 1
        assert f["frontier_compute_dev"](th, C.byref(good), None) == 1
        assert f["read_frontier_labels"](th, ptr(out)) == 1
        assert f["read_frontier_clusters"](th, ptr(rec), ptr(goal), C.byref(n)) == 1
    finally:
        m.close()
        t.close()

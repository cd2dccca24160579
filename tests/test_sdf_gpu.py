"""The signed distance field on the device (include/gie.h gie_read_sdf / gie_query_sdf and their _dev forms) against the numpy
statement of tests/sdf_ref.py, on what read_local returns at the same point of the mapper's stream."""
import numpy as np
import pytest

import planner_scenes as ps
import sdf_ref
from gie import scenes
from stage_common import BoxDrive, box_labels as _box_labels, mapper as _mapper, random_boxes as _random_boxes
from stage_common import stage_calls_change_nothing, update as _update

pytestmark = pytest.mark.gpu


def _check(m, size, loc=None, ids=None):
    """read_sdf against the reference computed from read_local's types (`ids`: inside_dist_sq of those types by another reference
    than scipy's); returns (sdf, ids, loc)"""
    if loc is None:
        loc = m.read_local(dist_sq=False, coc=False)
    r = m.read_sdf()
    if ids is None:
        ids = sdf_ref.inside_dist_sq(loc["type"])
    assert np.array_equal(r["inside_dist_sq"], ids), int((r["inside_dist_sq"] != ids).sum())
    shallow = (ids >= 0) & (ids <= 1)
    assert np.array_equal(r["sdf"][shallow].view(np.uint32), loc["edt"][shallow].view(np.uint32))
    assert np.allclose(r["sdf"], sdf_ref.sdf(ids, loc["edt"], size), rtol=1e-6, atol=0)
    return r["sdf"], ids, loc


@pytest.mark.parametrize("size", [(96, 80, 72), (97, 61, 45), (77, 53, 1)])
def test_exact_on_solid_boxes(size):
    rng = np.random.default_rng(sum(size))
    boxes = _random_boxes(rng, 10, 40, 4, 30)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, 0.1, size)
        lab = _box_labels(pvt, size, 0, boxes, unknown_slab=5)
        for _ in range(2):
            _update(m, pos, q, lab)
            _, ids, loc = _check(m, size)
        assert ids.max() >= (4 if size[2] > 1 else 2)      # interior voxels exist: the exact pass ran
    finally:
        m.close()


def test_exact_with_external_boxes_and_fence():
    size, w = (96, 88, 64), 0.1
    m = _mapper(size, voxel=w)
    try:
        pos, q = scenes.pose(0, w, delta_vox=4, yaw_deg=0.0)
        pvt = np.array(scenes.local_pivot(pos, w, size))
        lo_v, hi_v = pvt + 20, pvt + np.array(size) - 25          # the fence leaves occupied slabs 20 - 25 voxels thick
        ll = [lo_v * w, (pvt + [40, 30, 10]) * w]
        ur = [hi_v * w, (pvt + [60, 55, 40]) * w]
        m.set_ext_boxes(np.array(ll, np.float32), np.array(ur, np.float32), np.array([1, 1], np.uint8))
        lab = np.ones((size[2], size[1], size[0]), np.int8)
        for _ in range(3):
            _update(m, pos, q, lab)
        _, ids, loc = _check(m, size)
        assert (loc["type"] == 2).mean() > 0.3 and ids.max() >= 300
    finally:
        m.close()


def test_all_occupied_volume():
    size = (40, 36, 20)
    m = _mapper(size)
    try:
        pos, q = scenes.pose(0, 0.1, delta_vox=4, yaw_deg=0.0)
        lab = np.full((size[2], size[1], size[0]), 2, np.int8)
        for _ in range(3):
            _update(m, pos, q, lab)
        s, ids, loc = _check(m, size)
        assert (loc["type"] == 2).all() and (ids == -1).all()
        assert (s == -np.float32(sum(v * v for v in size))).all()
    finally:
        m.close()


@pytest.mark.parametrize("n", [256, 512])
def test_c5_hash_world(n):
    size, w = (n, n, n), 0.05
    m = _mapper(size, voxel=w, cutoff_dist=2.0)
    try:
        for k in range(2):
            pos, q = scenes.pose(k, w, delta_vox=8, yaw_deg=2.0)
            pvt = scenes.local_pivot(pos, w, size)
            _update(m, pos, q, scenes.hash_world_labels(pvt, size, k).astype(np.int8))
        loc = m.read_local(dist_sq=False, coc=False)
        r = m.read_sdf()
        occ = loc["type"] == 2
        assert not ps.interior(occ).any()                      # the device-gated skip of the exact pass
        ids = occ.astype(np.int32)
        if n <= 256:
            assert np.array_equal(ids, sdf_ref.inside_dist_sq(loc["type"]))
        assert np.array_equal(r["inside_dist_sq"], ids)
        assert np.array_equal(r["sdf"].view(np.uint32), loc["edt"].view(np.uint32))   # no voxel deeper than the surface
    finally:
        m.close()


def test_drive_moving_toggling_boxes():
    size = (96, 80, 64)
    d = BoxDrive(size, unknown_slab=0)
    m = _mapper(size)
    try:
        deep = 0
        for k in range(32):
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
            _, ids, _ = _check(m, size)
            deep = max(deep, int(ids.max()))
        assert deep >= 9
    finally:
        m.close()


def test_stream_enabled_update_and_ray_cast_update():
    size = (80, 72, 64)
    d = BoxDrive(size, seed=4, unknown_slab=0)
    m = _mapper(size)
    try:
        m.stream_enable(True)
        pos, q, lab = d.frame(0)
        _update(m, pos, q, lab)
        _check(m, size)
        m.stream_changed()
        # a ray-cast update: a point cloud of a solid block ahead of the sensor (sensor frame = world axes, yaw 0)
        g = np.arange(0.0, 1.2, 0.05, dtype=np.float32)
        blk = np.stack(np.meshgrid(g + 1.5, g - 0.6, g - 0.6, indexing="ij"), -1).reshape(-1, 3)
        m.set_pose(pos, q)
        m.ogm_pointcloud(blk)
        m.step()
        _, ids, loc = _check(m, size)
        assert (loc["type"] == 2).any()
    finally:
        m.close()


def test_sdf_calls_change_nothing_of_the_map_update():
    size = (80, 64, 64)
    d = BoxDrive(size, seed=5, unknown_slab=0)

    def calls(a, k, phase, pos):
        if phase == "labels":
            a.query_sdf(np.zeros((7, 3), np.float32))
        elif phase == "fuse":
            a.read_sdf()
        elif phase == "merge":
            a.query_sdf(np.random.default_rng(k).uniform(-5, 5, (1000, 3)).astype(np.float32))
    stage_calls_change_nothing(size, (d.frame(k) for k in range(12)), _mapper, calls)


def _points(rng, m, size, w, n):
    """n world points: uniform over the volume +- 3 voxels (some outside), exact faces and corners"""
    pvt = np.array(m.pivot(), np.float32)
    S = np.array(size, np.float32)
    u = rng.uniform(-3, S + 2, size=(n, 3)).astype(np.float32)
    face = rng.random(n) < 0.1
    ax = rng.integers(0, 3, n)
    u[face, ax[face]] = np.where(rng.random(face.sum()) < 0.5, 0.0, S[ax[face]] - 1)
    flat = S == 1
    u[:, flat] = rng.uniform(-0.7, 0.7, size=(n, int(flat.sum())))
    return ((u + pvt) * np.float32(w)).astype(np.float32)


@pytest.mark.parametrize("size", [(72, 64, 48), (61, 47, 1)])
def test_queries_match_the_reference_and_the_dev_form(size):
    import torch
    w = 0.125                                                  # a power of two: u = p / w - pvt is exact on the faces
    d = BoxDrive(size, seed=6, w=w, unknown_slab=0)
    m = _mapper(size, voxel=w)
    try:
        for k in range(3):
            pos, q, lab = d.frame(k)
            _update(m, pos, q, lab)
        r = m.read_sdf()
        loc = m.read_local(edt=False, dist_sq=False, coc=False)
        xyz = _points(np.random.default_rng(1), m, size, w, 120000)
        dist, grad, flags = m.query_sdf(xyz)
        rd, rg, rf = sdf_ref.query(r["sdf"], loc["type"], size, m.pivot(), w, xyz)
        assert np.array_equal(flags, rf)
        assert (flags & 1).mean() > 0.5 and (flags == 0).any() and ((flags & 4) != 0).any()
        assert np.array_equal(np.isnan(dist), np.isnan(rd))
        ok = ~np.isnan(rd)
        assert np.allclose(dist[ok], rd[ok], rtol=1e-5, atol=1e-5)
        assert np.allclose(grad, rg, rtol=1e-5, atol=1e-5)
        # the _dev form through torch tensors on the mapper's stream
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            dx = torch.from_numpy(xyz).to(dev)
            dd = torch.empty(len(xyz), dtype=torch.float32, device=dev)
            dg = torch.empty((len(xyz), 3), dtype=torch.float32, device=dev)
            df = torch.empty(len(xyz), dtype=torch.uint8, device=dev)
            m.query_sdf_dev(dx.data_ptr(), len(xyz), dd.data_ptr(), dg.data_ptr(), df.data_ptr())
            ds = torch.empty(size[::-1], dtype=torch.float32, device=dev)
            m.read_sdf_dev(ds.data_ptr(), 0)
        m.sync()
        assert np.array_equal(dd.cpu().numpy().view(np.uint32), dist.view(np.uint32))
        assert np.array_equal(dg.cpu().numpy(), grad) and np.array_equal(df.cpu().numpy(), flags)
        assert np.array_equal(ds.cpu().numpy().view(np.uint32), r["sdf"].view(np.uint32))
        prof = None
        m.profile_enable(True)
        m.query_sdf(xyz[:10])
        prof = m.profile_read()
        m.profile_enable(False)
        assert list(prof)[-2:] == ["sdf", "sdf_query"] and prof["sdf_query"][1] == 1
    finally:
        m.close()


def test_cache_follows_the_map():
    size = (64, 64, 48)
    d = BoxDrive(size, seed=7, unknown_slab=0)
    a, b = _mapper(size), _mapper(size)
    xyz = _points(np.random.default_rng(2), a, size, 0.1, 20000)
    try:
        for m in (a, b):
            pos, q, lab = d.frame(0)
            _update(m, pos, q, lab)
        first = a.query_sdf(xyz)
        again = a.query_sdf(xyz)                               # no update between: the cached planes, the same answer
        for x, y in zip(first, again):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        for m in (a, b):
            pos, q, lab = d.frame(3)                           # boxes toggle: occupancy changes
            _update(m, pos, q, lab)
        after = a.query_sdf(xyz)                               # a recomputes its cached planes ...
        fresh = b.query_sdf(xyz)                               # ... b computes them for the first time
        for x, y in zip(after, fresh):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        assert not np.array_equal(np.nan_to_num(after[0]), np.nan_to_num(first[0]))
        _check(a, size)
    finally:
        a.close()
        b.close()


def test_refusals():
    import ctypes as C
    size = (32, 32, 16)
    m = _mapper(size)
    t = _mapper(size)
    try:
        f, h = m._f, m._h
        xyz = np.zeros((4, 3), np.float32)
        out = np.zeros(4, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)            # noqa: E731
        assert f["query_sdf"](h, p(xyz), -1, p(out), None, None) == 1
        assert f["query_sdf"](h, p(xyz), 4, None, None, None) == 1
        assert f["query_sdf"](h, None, 4, p(out), None, None) == 1
        assert f["query_sdf"](h, p(xyz), 0, p(out), None, None) == 0
        assert f["query_sdf_dev"](h, None, 4, None, None, None) == 1
        assert f["query_sdf_dev"](h, None, -2, None, None, None) == 1
        assert f["read_sdf_dev"](h, None, None) == 1
        assert f["read_sdf"](None, None, None) == 1
        t.set_tile((8, 0, 0), (64, 32, 16))
        th = t._h
        assert f["read_sdf"](th, p(np.zeros(t.n, np.float32)), None) == 1
        assert f["read_sdf_dev"](th, None, None) == 1
        assert f["query_sdf"](th, p(xyz), 4, p(out), None, None) == 1
        assert f["query_sdf_dev"](th, None, 0, None, None, None) == 1
        t.set_tile((0, 0, 0), size)
        assert f["query_sdf"](th, p(xyz), 4, p(out), None, None) == 0
    finally:
        m.close()
        t.close()


# ---- the exact pass over its dispatch: k_sdf_line<CP, .> by max(Y, Z), long bit rows, word borders in x, axes of length 1 and 2

def _solid_case(size, cp, seed, fill=0.0, w=0.1, fence=False, ids_of=None):
    """a solid scene (planner_scenes.solid_labels) fed twice, read_sdf against the reference, the scene's properties on read_local's
    types, and the same bytes from the planes rebuilt after a third identical update"""
    assert ps.sdf_cp(size) == cp                               # the instantiation gie_sdf_ready selects for this shape
    m = _mapper(size, voxel=w)
    try:
        pos, q = scenes.pose(0, w, delta_vox=4, yaw_deg=0.0)
        if fence:                                              # as test_exact_with_external_boxes_and_fence, scaled to the volume
            pvt, S = np.array(scenes.local_pivot(pos, w, size)), np.array(size)
            ll = [(pvt + 20) * w, (pvt + S // 2 - S // 10) * w]
            ur = [(pvt + S - 25) * w, (pvt + S // 2 + S // 8) * w]
            m.set_ext_boxes(np.array(ll, np.float32), np.array(ur, np.float32), np.array([1, 1], np.uint8))
        lab = ps.solid_labels(size, seed, fill)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        sdf, ids, _ = _check(m, size, loc, None if ids_of is None else ids_of(loc["type"]))
        if fill == 0:
            ps.assert_scene(size, loc["type"], ids, fenced=fence)
        elif max(size) > 2:
            assert ids.max() >= int(fill * max(size)) ** 2     # the block at the low end: its first layer is that far from free space
        assert size == (1, 1, 1) or (ids > 1).any()            # interior voxels: the gate cannot hide the line kernels
        if fence:
            assert (loc["type"] == 2).mean() > 0.2
        _update(m, pos, q, lab)
        r = m.read_sdf()
        assert np.array_equal(r["inside_dist_sq"], ids) and np.array_equal(r["sdf"].view(np.uint32), sdf.view(np.uint32))
    finally:
        m.close()


@pytest.mark.parametrize("size,cp", ps.SDF_SIZES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "cp%d" % v)
def test_exact_over_the_line_kernel_dispatch(size, cp):
    _solid_case(size, cp, 1)
    _solid_case(size, cp, 2, fill=0.45)                        # distances of almost half the longest side


def test_exact_at_256_cube_with_interiors():
    _solid_case((256, 256, 256), 4, 1, w=0.05, fence=True)


def test_exact_at_512_cube_with_interiors(oracle_lib):
    """the reference is the CPU EDT of the complement (tests/test_sdf_reference.py pins it against scipy and brute force)"""
    from oracle_py import edt_mt
    _solid_case((512, 512, 512), 8, 1, w=0.05, fence=True, ids_of=lambda t: ps.complement_inside_dist_sq(t, edt_mt, 16))


# ---- key magnitude: a volume occupied but for one voxel; inside_dist_sq = (x-x0)² + (y-y0)² + (z-z0)², the largest a shape can hold

def _hole_case(size, hole):
    try:
        m = _mapper(size, voxel=0.05, cutoff_dist=1.0)
    except RuntimeError as e:
        if "allocation failed" in str(e):
            pytest.skip("the device cannot hold this volume right now: " + str(e))
        raise
    try:
        pos, q = scenes.pose(0, 0.05, delta_vox=0, yaw_deg=0.0)
        lab = ps.hole_labels(size, hole)
        for _ in range(2):
            _update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        assert np.array_equal(loc["type"] == 2, lab == 2)
        want = ps.hole_inside_dist_sq(size, hole)
        _, ids, _ = _check(m, size, loc, want)
        assert ids.max() == max((x - hole[0]) ** 2 + (y - hole[1]) ** 2 + (z - hole[2]) ** 2
                                for x in (0, size[0] - 1) for y in (0, size[1] - 1) for z in (0, size[2] - 1))
        return int(ids.max())
    finally:
        m.close()


@pytest.mark.parametrize("hole", [0, 1, 2])
@pytest.mark.parametrize("size", [(1024, 1024, 8), (1024, 8, 1024)])
def test_one_free_voxel_in_a_thin_1024_volume(size, hole):
    deepest = _hole_case(size, ps.hole_positions(size)[hole])
    assert deepest == 2093107 if hole < 2 else deepest > 500000


def test_one_free_voxel_at_1024_1024_128():
    size = (1024, 1024, 128)                                   # gie_create accepts it: X² + Y² + Z² + 1 + max(X, Z)² = 3 162 113 < 2^22
    deepest = [_hole_case(size, h) for h in ps.hole_positions(size)]
    assert deepest[0] == deepest[1] == 2109187


# ---- queries on the odd shapes

def _query_case(size, dev_form):
    import torch
    w = 0.125                                                  # a power of two: u = p / w - pvt is exact on the faces
    m = _mapper(size, voxel=w)
    try:
        pos, q = scenes.pose(0, w, delta_vox=4, yaw_deg=0.0)
        lab = ps.solid_labels(size, 3, fill=0.4)
        for _ in range(2):
            _update(m, pos, q, lab)
        r = m.read_sdf()
        loc = m.read_local(edt=False, dist_sq=False, coc=False)
        xyz = ps.query_points(np.random.default_rng(1), m.pivot(), size, w, 120000)
        dist, grad, flags = m.query_sdf(xyz)
        rd, rg, rf = sdf_ref.query(r["sdf"], loc["type"], size, m.pivot(), w, xyz)
        assert np.array_equal(flags, rf)
        assert (flags & 1).mean() > 0.3 and (flags == 0).any() and ((flags & 4) != 0).any()
        assert max(size) <= 2 or ((flags & 1) != 0)[(flags & 2) == 0].any()       # a never-seen corner somewhere
        assert np.array_equal(np.isnan(dist), np.isnan(rd))
        ok = ~np.isnan(rd)
        assert np.allclose(dist[ok], rd[ok], rtol=1e-5, atol=1e-5)
        assert np.allclose(grad, rg, rtol=1e-5, atol=1e-5)
        for k in range(3):
            if size[k] == 1:
                assert (grad[:, k] == 0).all()
        # a tenth of the in-volume samples interpolate a voxel deeper than the surface: the interpolant of the indicator is positive
        deep, _, _ = sdf_ref.query((r["inside_dist_sq"] > 1).astype(np.float32), loc["type"], size, m.pivot(), w, xyz)
        assert (deep[ok] > 0).mean() >= 0.1
        if dev_form:                                           # the _dev form through torch tensors on the mapper's stream
            dev = torch.device("cuda", 0)
            st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
            with torch.cuda.stream(st):
                dx = torch.from_numpy(xyz).to(dev)
                dd = torch.empty(len(xyz), dtype=torch.float32, device=dev)
                dg = torch.empty((len(xyz), 3), dtype=torch.float32, device=dev)
                df = torch.empty(len(xyz), dtype=torch.uint8, device=dev)
                m.query_sdf_dev(dx.data_ptr(), len(xyz), dd.data_ptr(), dg.data_ptr(), df.data_ptr())
                ds = torch.empty(size[::-1], dtype=torch.float32, device=dev)
                m.read_sdf_dev(ds.data_ptr(), 0)
            m.sync()
            assert np.array_equal(dd.cpu().numpy().view(np.uint32), dist.view(np.uint32))
            assert np.array_equal(dg.cpu().numpy().view(np.uint32), grad.view(np.uint32)) and np.array_equal(df.cpu().numpy(), flags)
            assert np.array_equal(ds.cpu().numpy().view(np.uint32), r["sdf"].view(np.uint32))
    finally:
        m.close()


@pytest.mark.parametrize("size", ps.QUERY_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_queries_on_flat_thin_and_long_volumes(size):
    _query_case(size, dev_form=size in ((1, 40, 40), (1024, 16, 12)))


def test_queries_at_256_cube_with_interiors():
    _query_case((256, 256, 256), dev_form=False)

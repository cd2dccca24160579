"""The numpy statement of the signed distance field (tests/sdf_ref.py) against brute force, and the C-ABI that exposes it
(include/gie.h gie_read_sdf / gie_query_sdf and their _dev forms).  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import planner_scenes as ps
import sdf_ref
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _types(shape, p_occ, rng, p_unknown=0.0):
    t = np.where(rng.random(shape) < p_occ, 2, 1).astype(np.int8)
    t[rng.random(shape) < p_unknown] = 0
    return t


def _grids():
    rng = np.random.default_rng(7)
    g = {}
    g["random_dense"] = _types((9, 11, 13), 0.8, rng, 0.05)
    g["random_sparse"] = _types((7, 6, 10), 0.2, rng)
    cube = np.ones((12, 12, 12), np.int8)
    cube[2:10, 3:11, 1:9] = 2
    g["solid_cube"] = cube
    slab = np.ones((10, 9, 8), np.int8)
    slab[3:8] = 2
    g["slab"] = slab
    shell = np.full((9, 9, 9), 2, np.int8)
    shell[1:8, 1:8, 1:8] = 0                  # a one-voxel shell round an unknown core: unknown counts as non-occupied
    g["shell_unknown_core"] = shell
    g["shell_fnt_core"] = np.where(shell == 0, 3, shell).astype(np.int8)
    g["all_occupied"] = np.full((4, 5, 6), 2, np.int8)
    g["flat_z1"] = _types((1, 17, 19), 0.85, rng)
    g["line_x"] = _types((1, 1, 23), 0.9, rng)
    g["one_voxel"] = np.full((1, 1, 1), 2, np.int8)
    return g


@pytest.mark.parametrize("name", sorted(_grids()))
def test_inside_dist_sq_matches_brute_force(name):
    t = _grids()[name]
    ref = sdf_ref.inside_dist_sq(t)
    assert ref.dtype == np.int32
    assert np.array_equal(ref, sdf_ref.inside_dist_sq_brute(t))
    assert (ref[t != 2] == 0).all()


def test_hand_built_values():
    g = _grids()
    c = sdf_ref.inside_dist_sq(g["solid_cube"])
    assert c[2, 3, 1] == 1 and c[5, 6, 4] == 16      # a corner, and the centre of the 8-voxel cube: 4 layers deep
    s = sdf_ref.inside_dist_sq(g["slab"])
    assert list(s[3:8, 4, 4]) == [1, 4, 9, 4, 1]
    sh = sdf_ref.inside_dist_sq(g["shell_unknown_core"])
    assert sh[0, 4, 4] == 1 and sh[0, 0, 4] == 2 and sh[0, 0, 0] == 3   # the core is non-occupied: faces 1, edges 2, corners 3
    assert (sdf_ref.inside_dist_sq(g["all_occupied"]) == -1).all()


def test_sdf_formula():
    size = (6, 5, 4)
    ids = np.array([0, 1, 2, 9, -1], np.int32)
    edt = np.array([3.5, 0.0, 0.0, 0.0, 0.0], np.float32)
    s = sdf_ref.sdf(ids, edt, size)
    assert s.dtype == np.float32
    assert s[0] == np.float32(3.5) and s[1] == 0
    assert s[2] == np.float32(1) - np.sqrt(np.float32(2))
    assert s[3] == np.float32(-2)
    assert s[4] == -np.float32(36 + 25 + 16)


def _field(shape, rng):
    t = _types(shape, 0.3, rng, 0.1)
    return t, (rng.random(shape) * 8 - 4).astype(np.float32)


def test_query_outside_and_faces():
    rng = np.random.default_rng(3)
    size = (7, 6, 5)
    t, f = _field((5, 6, 7), rng)
    pvt, w = (-3, 10, 2), 0.25
    u = np.array([[0, 0, 0], [6, 5, 4], [-1e-3, 1, 1], [6.001, 1, 1], [1, 1, 4.01], [2.5, 3.25, 1.75]], np.float32)
    xyz = (u + np.array(pvt, np.float32)) * np.float32(w)
    d, g, fl = sdf_ref.query(f, t, size, pvt, w, xyz)
    assert list(fl[[2, 3, 4]]) == [0, 0, 0] and np.isnan(d[[2, 3, 4]]).all() and (g[[2, 3, 4]] == 0).all()
    assert (fl[[0, 1, 5]] & 1).all()
    assert np.isclose(d[0], f[0, 0, 0] * w) and np.isclose(d[1], f[4, 5, 6] * w)
    # flags: all corners known / some corner occupied
    x0, y0, z0 = 2, 3, 1
    cube = t[z0:z0 + 2, y0:y0 + 2, x0:x0 + 2]
    assert bool(fl[5] & 2) == bool((cube != 0).all()) and bool(fl[5] & 4) == bool((cube == 2).any())


def test_query_gradient_matches_central_differences():
    rng = np.random.default_rng(11)
    size = (9, 8, 7)
    t, f = _field((7, 8, 9), rng)
    pvt, w = (4, -2, 0), 0.5
    # points strictly inside cells (away from the faces between cells, where the interpolant's gradient jumps)
    cell = rng.integers(0, [s - 1 for s in size], size=(400, 3))
    frac = rng.uniform(0.1, 0.9, size=(400, 3))
    u = (cell + frac).astype(np.float64)
    h = 1e-3
    xyz = ((u + np.array(pvt)) * w).astype(np.float32)
    _, g, fl = sdf_ref.query(f, t, size, pvt, w, xyz)
    assert (fl & 1).all()
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        dp, _, _ = sdf_ref.query(f, t, size, pvt, w, ((u + e + np.array(pvt)) * w).astype(np.float64).astype(np.float32))
        dm, _, _ = sdf_ref.query(f, t, size, pvt, w, ((u - e + np.array(pvt)) * w).astype(np.float64).astype(np.float32))
        fd = (dp.astype(np.float64) - dm) / (2 * h * w)
        assert np.allclose(g[:, k], fd, rtol=1e-2, atol=2e-2), k


def test_query_size_one_axis():
    rng = np.random.default_rng(5)
    size = (6, 5, 1)
    t, f = _field((1, 5, 6), rng)
    pvt, w = (0, 0, 7), 0.2
    zs = np.array([6.5, 6.51, 7.0, 7.49, 7.5], np.float32)
    xyz = np.stack([np.full(5, 0.5), np.full(5, 0.3), zs * np.float32(w)], axis=1).astype(np.float32)
    d, g, fl = sdf_ref.query(f, t, size, pvt, w, xyz)
    u = xyz[:, 2] / np.float32(w) - np.float32(7)
    inside = (u >= -0.5) & (u < 0.5)
    assert ((fl & 1) == inside).all()
    assert (g[:, 2] == 0).all()
    assert np.allclose(d[inside], d[inside][0])        # constant along the flat axis


@pytest.mark.parametrize("size", [(1, 5, 6), (6, 1, 5), (1, 1, 6), (2, 5, 2)])
def test_query_flat_x_and_flat_y(size):
    """a flat axis: inside for u in [-0.5, 0.5), zero gradient component, the value constant along it; a side of 2 is one cell"""
    rng = np.random.default_rng(sum(size))
    t, f = _field(size[::-1], rng)
    pvt, w = (3, -4, 7), 0.25
    n = 400
    u = rng.uniform(0, np.maximum(np.array(size) - 1, 0), size=(n, 3)).astype(np.float32)
    flat = [k for k in range(3) if size[k] == 1]
    ends = np.array([-0.7, -0.5, -0.25, 0.0, 0.49, 0.5, 0.7], np.float32)
    for k in flat:
        u[:, k] = ends[rng.integers(0, len(ends), n)]
    xyz = ((u + np.array(pvt, np.float32)) * np.float32(w)).astype(np.float32)
    d, g, fl = sdf_ref.query(f, t, size, pvt, w, xyz)
    inside = np.ones(n, bool)
    for k in flat:
        inside &= (u[:, k] >= -0.5) & (u[:, k] < 0.5)
        assert (g[:, k] == 0).all()
    assert ((fl & 1) != 0).tolist() == inside.tolist() and inside.any() and ((~inside).any() or not flat)
    # moving a point along a flat axis inside [-0.5, 0.5) changes nothing
    moved = u.copy()
    for k in flat:
        moved[:, k] = np.where(inside, 0.0, u[:, k])
    d2, g2, fl2 = sdf_ref.query(f, t, size, pvt, w, ((moved + np.array(pvt, np.float32)) * np.float32(w)).astype(np.float32))
    assert np.array_equal(d2[inside], d[inside]) and np.array_equal(g2, g) and np.array_equal(fl2, fl)
    # a side of 2: the one cell 0..1, its value at the two ends of the axis is the plane's
    for k in range(3):
        if size[k] == 2:
            z = np.zeros((2, 3), np.float32)
            z[1, k] = 1.0
            dd, _, ff = sdf_ref.query(f, t, size, pvt, w, (z + np.array(pvt, np.float32)) * np.float32(w))
            idx = [[0, 0, 0], [0, 0, 0]]
            idx[1][2 - k] = 1
            assert (ff & 1).all() and np.allclose(dd, [f[tuple(i)] * w for i in idx])


# ---- the scenes and references of the device tests on long lines and thin volumes (tests/planner_scenes.py)

@pytest.mark.parametrize("size,cp", ps.SDF_SIZES + ps.BIG_SIZES[:1], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "cp%d" % v)
def test_solid_scene_meets_its_requirements_at_every_shape(size, cp):
    """on the labels: a fully labelled scan fed twice commits them (the device test asserts the same on read_local)"""
    assert ps.sdf_cp(size) == cp
    lab = ps.solid_labels(size, 1)
    assert lab.shape == size[::-1] and lab.dtype == np.int8 and np.array_equal(lab, ps.solid_labels(size, 1))
    ps.assert_scene(size, lab, sdf_ref.inside_dist_sq(lab))
    if max(size) > 2 and max(size) <= 1024 and np.prod(size) < 10 ** 6:
        filled = sdf_ref.inside_dist_sq(ps.solid_labels(size, 2, fill=0.45))
        assert filled.max() >= int(0.45 * max(size)) ** 2


def test_every_line_kernel_of_the_dispatch_is_in_the_table():
    assert {cp for _, cp in ps.SDF_SIZES} == {1, 2, 4, 8, 16}
    assert [ps.sdf_cp((8, y, 8)) for y in (64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert ps.sdf_cp((1024, 8, 8)) == 1 and ps.sdf_cp((8, 8, 600)) == 16      # by max(Y, Z): X does not count


def test_complement_edt_is_inside_dist_sq(oracle_lib):
    """the reference of the 512^3 device case: the project's CPU EDT on the complement of the obstacles, restricted to them"""
    from oracle_py import edt_mt
    mid = ps.solid_labels((96, 80, 72), 4)
    assert np.array_equal(ps.complement_inside_dist_sq(mid, edt_mt, 4), sdf_ref.inside_dist_sq(mid))
    thin = ps.solid_labels((16, 300, 12), 4, fill=0.45)
    assert np.array_equal(ps.complement_inside_dist_sq(thin, edt_mt, 4), sdf_ref.inside_dist_sq(thin))
    g = _grids()
    for name in ("random_dense", "solid_cube", "shell_unknown_core", "all_occupied", "flat_z1", "line_x", "one_voxel"):
        assert np.array_equal(ps.complement_inside_dist_sq(g[name], edt_mt, 2), sdf_ref.inside_dist_sq_brute(g[name])), name


@pytest.mark.parametrize("size", [(1024, 1024, 8), (7, 5, 3)])
def test_one_free_voxel_closed_form(size):
    for hole in ps.hole_positions(size):
        lab = ps.hole_labels(size, hole)
        want = ps.hole_inside_dist_sq(size, hole)
        assert want.dtype == np.int32 and (lab != 2).sum() == 1 and want[hole[2], hole[1], hole[0]] == 0
        assert np.array_equal(want, sdf_ref.inside_dist_sq(lab))
        if np.prod(size) < 1000:
            assert np.array_equal(want, sdf_ref.inside_dist_sq_brute(lab))
    if size[0] == 1024:
        assert want.max() == 512 ** 2 + 512 ** 2 + 49 and ps.hole_inside_dist_sq(size, (0, 0, 0)).max() == 2093107


def test_query_points_hit_the_faces_and_the_ends_of_flat_axes():
    for size in ps.QUERY_SIZES:
        pvt, w = (5, -3, 2), 0.125
        xyz = ps.query_points(np.random.default_rng(1), pvt, size, w, 20000)
        u = xyz / np.float32(w) - np.array(pvt, np.float32)
        for k in range(3):
            if size[k] == 1:
                assert (u[:, k] == -0.5).any() and (u[:, k] == 0.5).any() and (np.abs(u[:, k]) <= 0.7).all()
            else:
                assert (u[:, k] == 0).any() and (u[:, k] == size[k] - 1).any() and (u[:, k] < 0).any() and (u[:, k] > size[k] - 1).any()
        # with the labels for types: a tenth of the in-volume samples have a corner deeper than the surface
        lab = ps.solid_labels(size, 3, fill=0.4)
        ids = sdf_ref.inside_dist_sq(lab)
        deep, _, fl = sdf_ref.query((ids > 1).astype(np.float32), lab, size, pvt, w, xyz)
        assert (fl & 1).mean() > 0.3 and (deep[(fl & 1) != 0] > 0).mean() >= 0.1, size


def _declared():
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_and_binding_binds_the_sdf_calls():
    txt = _declared()
    for sig in (r"int\s+gie_read_sdf\s*\(\s*gie_mapper\s*\*\s*h\s*,\s*float\s*\*\s*sdf\s*,\s*int32_t\s*\*\s*inside_dist_sq\s*\)",
                r"int\s+gie_read_sdf_dev\s*\(\s*gie_mapper\s*\*\s*h\s*,\s*float\s*\*\s*d_sdf\s*,\s*int32_t\s*\*\s*d_inside_dist_sq\s*\)",
                r"int\s+gie_query_sdf\s*\(\s*gie_mapper\s*\*\s*h\s*,\s*const\s+float\s*\*\s*xyz\s*,\s*int\s+n\s*,\s*float\s*\*\s*dist\s*,"
                r"\s*float\s*\*\s*grad\s*,\s*uint8_t\s*\*\s*flags\s*\)",
                r"int\s+gie_query_sdf_dev\s*\(\s*gie_mapper\s*\*\s*h\s*,\s*const\s+float\s*\*\s*d_xyz\s*,\s*int\s+n\s*,\s*float\s*\*\s*d_dist\s*,"
                r"\s*float\s*\*\s*d_grad\s*,\s*uint8_t\s*\*\s*d_flags\s*\)"):
        assert re.search(sig, txt), sig
    for name, nargs in (("read_sdf", 3), ("read_sdf_dev", 3), ("query_sdf", 6), ("query_sdf_dev", 6)):
        assert name in _capi.DEVICE_ONLY and len(_capi.DEVICE_ONLY[name][1]) == nargs
        assert name not in _capi.SIGNATURES          # the oracle and the emulation do not have them


def test_mapper_and_host_layer_expose_the_sdf(tmp_path):
    import gie
    for meth in ("read_sdf", "read_sdf_dev", "query_sdf", "query_sdf_dev"):
        assert callable(getattr(gie.Mapper, meth))
    src = tmp_path / "use_sdf.cpp"
    src.write_text('#include "gie_host.hpp"\n'
                   "void use(gie_host::VolumetricMapper &m, std::vector<float> &sdf, const float *xyz, float *d, float *g, uint8_t *f)\n"
                   "{ m.readSignedDistance(sdf); m.querySignedDistance(xyz, 4, d, g, f); }\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "gie-mapping_amd", "host"), str(src)], check=True)

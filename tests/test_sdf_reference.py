"""The numpy statement of the signed distance field (tests/sdf_ref.py) against brute force, and the C-ABI that exposes it
(include/gie.h gie_read_sdf / gie_query_sdf and their _dev forms).  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

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

"""The numpy reference of the display clouds (tests/cloud_ref.py) against a literal restatement of the two loops of the reference's
visualize (include/volumetric_mapper.h:181-317) on hand-made arrays, and the binding's view of the C-ABI section."""
import ctypes as C
import os
import re

import numpy as np

import cloud_ref as R
import gie
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY_VALUE = 999999                    # GIE_EMPTY_VALUE (include/gie.h)
W = np.float32(0.1)


def _loop_local(types, edt, pvt, w, p):
    """publish_local_ptcld_2_rviz, generalised to a mask and a band: one voxel at a time"""
    Z, Y, X = types.shape
    out = []
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                t = int(types[z, y, x])
                g = (x + pvt[0], y + pvt[1], z + pvt[2])
                if t == 0 or not (p["type_mask"] >> t) & 1 or g[2] < p["z_lo"] or g[2] > p["z_hi"]:
                    continue
                pos = [np.float32(c) * w for c in g]
                inten = np.float32(t) if p["intensity"] == R.TYPE else np.float32(edt[z, y, x]) * w
                out.append((pos[0], pos[1], pos[2], inten))
    return np.array(out, R.CLOUD_DTYPE) if out else np.zeros(0, R.CLOUD_DTYPE)


def _loop_global(records, xyz, w, p):
    """publish_glb_2_rviz over a list of voxels: type, slice, invalid_dist_glb"""
    out = []
    for r, g in zip(records, xyz):
        t, d = int(r["vox_type"]), int(r["dist_sq"])
        if t == 0 or not (p["type_mask"] >> t) & 1 or g[2] < p["z_lo"] or g[2] > p["z_hi"]:
            continue
        if p["intensity"] == R.DIST and (d < 0 or d >= 900000):
            continue
        pos = [np.float32(int(c)) * w for c in g]
        inten = np.float32(t) if p["intensity"] == R.TYPE else np.sqrt(np.float32(d)) * w
        out.append((pos[0], pos[1], pos[2], inten))
    return np.array(out, R.CLOUD_DTYPE) if out else np.zeros(0, R.CLOUD_DTYPE)


PVT = (-7, 3, -4)                       # negative and positive coordinates on the axes
SHAPE = (9, 10, 11)                     # [Z][Y][X]


def _params():
    zs = (PVT[2], PVT[2] + SHAPE[0] - 1)
    bands = [(None, None), (zs[0], zs[0]), (zs[1], zs[1]), (zs[0] - 5, zs[0] + 2), (zs[0] - 9, zs[0] - 1), (zs[1] + 1, zs[1] + 4), (zs[0] + 3, None)]
    masks = [(1 << R.OCCUPIED, R.TYPE), (R.KNOWN, R.DIST), (1 << R.FNT, R.TYPE), ((1 << R.FREE) | (1 << R.FNT), R.DIST)]
    return [R.param(m, i, lo, hi) for m, i in masks for lo, hi in bands]


def test_local_reference_is_the_reference_loop():
    rng = np.random.default_rng(1)
    types = rng.integers(0, 4, SHAPE).astype(np.int8)
    edt = rng.integers(0, 3000, SHAPE).astype(np.float32) ** np.float32(0.5)
    edt[0, 0, :3] = (0.0, 1e6, 1732.0508)                       # "see nothing" values are kept: the local loop drops no distance
    n_nonempty = 0
    for p in _params():
        a, b = R.local_cloud(types, edt, PVT, W, p), _loop_local(types, edt, PVT, W, p)
        assert R.same(a, b), p
        n_nonempty += len(a) > 0
        if p["z_lo"] > PVT[2] + SHAPE[0] - 1 or p["z_hi"] < PVT[2]:
            assert len(a) == 0, p
    assert n_nonempty >= 16
    occ = R.local_cloud(types, edt, PVT, W, R.param(1 << R.OCCUPIED))
    assert len(occ) == int((types == 2).sum()) and (occ["intensity"] == 2.0).all() and (occ["x"] < 0).any() and (occ["y"] > 0).all()


def test_global_reference_is_the_reference_loop():
    rng = np.random.default_rng(2)
    xyz = R.box_coords(PVT, (PVT[0] + SHAPE[2], PVT[1] + SHAPE[1], PVT[2] + SHAPE[0]))
    rec = np.zeros(len(xyz), gie.mapper.VOXEL_DTYPE)
    rec["vox_type"] = rng.integers(0, 4, len(xyz))
    rec["dist_sq"] = rng.integers(0, 5000, len(xyz))
    edge = np.array([-1, 0, 899999, 900000, EMPTY_VALUE], np.int32)
    for t in (1, 2, 3):                                         # every edge value under every selectable type, on several layers
        idx = rng.choice(len(xyz), 3 * len(edge), replace=False)
        rec["vox_type"][idx] = t
        rec["dist_sq"][idx] = np.tile(edge, 3)
    n_nonempty = 0
    for p in _params():
        a, b = R.global_cloud(rec, xyz, W, p), _loop_global(rec, xyz, W, p)
        assert R.same(a, b), p
        n_nonempty += len(a) > 0
    assert n_nonempty >= 16
    known = rec["vox_type"] != 0
    full = R.global_cloud(rec, xyz, W, R.param(R.KNOWN, R.DIST))
    valid = known & (rec["dist_sq"] >= 0) & (rec["dist_sq"] < 900000)
    assert len(full) == int(valid.sum()) < int(known.sum())
    assert np.float32(np.sqrt(np.float32(899999))) * W in full["intensity"] and 0.0 in full["intensity"]
    assert len(R.global_cloud(rec, xyz, W, R.param(R.KNOWN, R.TYPE))) == int(known.sum())      # the type cloud drops no distance


def test_canonical_order_tells_clouds_apart():
    a = np.array([(0.1, -0.2, 0.3, 2.0), (-0.0, 0.0, 0.0, 1.0)], R.CLOUD_DTYPE)
    assert R.same(a, a[::-1]) and not R.same(a, a[:1])
    b = a.copy()
    b["x"][1] = 0.0                                             # -0.0 and 0.0 are different records: the comparison is on bits
    assert not R.same(a, b)


def test_binding_matches_the_header():
    assert C.sizeof(_capi.CloudParam) == 32 and C.sizeof(_capi.CloudPoint) == 16
    assert gie.CLOUD_DTYPE.itemsize == 16 and gie.CLOUD_DTYPE == R.CLOUD_DTYPE
    assert (gie.CLOUD_TYPE, gie.CLOUD_DIST) == (R.TYPE, R.DIST) and gie.CLOUD_NO_BAND == R.NO_BAND
    assert (gie.VOX_UNKNOWN, gie.VOX_FREE, gie.VOX_OCCUPIED, gie.VOX_FNT) == (0, 1, 2, 3)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    for name in ("gie_cloud_local", "gie_cloud_local_dev", "gie_cloud_global", "gie_cloud_global_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*gie_mapper\s*\*" % name, txt), name
        assert name[4:] in _capi.DEVICE_ONLY and name[4:] not in _capi.SIGNATURES      # the emulation does not have them and keeps loading
    assert re.search(r"#define\s+GIE_CLOUD_TYPE\s+0\b", txt) and re.search(r"#define\s+GIE_CLOUD_DIST\s+1\b", txt)
    p = gie.Mapper.cloud_param(None, 1 << gie.VOX_FNT)
    assert (p.z_lo, p.z_hi, p.max_points, list(p.reserved)) == (-2 ** 31, 2 ** 31 - 1, 0, [0, 0, 0])


def test_host_layer_knows_cpu_mirror():
    txt = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert "bool cpu_mirror = true" in txt and '"cpu_mirror"' in txt and "visualize(const float sensor_pos[3])" in txt
    drv = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_driver.cpp")).read()
    assert "gie_cloud" not in drv and "visualize" not in drv       # the CPU tests link the driver against the emulation

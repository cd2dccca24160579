"""The builders of tests/stage_common.py that the query stages' device tests share, pinned by SHA-256 of their outputs: the label
planes, poses, cells and points those tests feed the device are the ones they were written with.

The digests were taken from the per-file definitions of commit 3019d61 (each test file's own _BoxDrive, _box_labels, _random_boxes,
_serpentine and _world, which agreed with one another wherever two files defined the same thing), not from this module."""
import hashlib
import types

import numpy as np

import stage_common as sc

PINS = {
    "drive_80x64x64_seed5_0": "aec52952ede965bbcf8adf73cd80fdee414a9e9e674e873afce3cfe4afa5a5d8",
    "drive_80x64x64_seed5_7": "2b45b51264a432f7c28408453727c18efa24b07aed0aa19841237708fdcb2f99",
    "drive_80x64x64_seed5_20": "90d00672e19c9ad70ceb54266df91e86578a1b8552949649ed8035bbd7e7f4ef",
    "drive_96x80x64_16_slab4": "d91384c3ddabefbd7eac0a9a42486c97120fae4c00f2ec048e9ff047f682d9db",
    "drive_96x80x64_16_slab0": "4ab6cf0174d054350313eddbd919bf04dc8ad1e7e374cca0409ae2bbec71ab33",
    "serpentine_150x36x20": "c5b55a8a14c968039a5d74673c693b83183f506598888a770d91689dec862cbd",
    "serpentine_cells_128x128x24_p4_m2": "d4ca0956734c1ed5282f2eb5172e32e676d5c92b1f972e482f700190518b75b6",
    "random_boxes": "b238cc0931767702354d97a4d3862988d1fd7e8308b3364d4c7e74b92db0c1e3",
    "world_int": "e682d1e1f3e7d3233697168d12ae4e6b44741f9a60fe85edcd88ea68043414e5",
    "world_f32": "4333f95eb9af22640d677911c640b45c82bbc2e921065b8a745b0ab8adb5b2d8",
    "world_int_jitter": "daa0cb410d8bedba9b66031d4f581828d5a76ceda3afaa65c9fa9fb617914885",
    "world_f32_jitter": "948a233101e7c0b7380774517f45ffb31449a1b86bec00050d6db69406f1940c",
}


def digest(*arrays):
    """over the dtype, shape and bytes of every array"""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_box_drive_frames():
    d = sc.BoxDrive((80, 64, 64), seed=5)
    for k in (0, 7, 20):                                        # the way out, and the way back (k >= 15)
        assert digest(*d.frame(k)) == PINS["drive_80x64x64_seed5_%d" % k], k
    assert digest(*sc.BoxDrive((96, 80, 64)).frame(16)) == PINS["drive_96x80x64_16_slab4"]
    assert digest(*sc.BoxDrive((96, 80, 64), unknown_slab=4).frame(16)) == PINS["drive_96x80x64_16_slab4"]
    assert digest(*sc.BoxDrive((96, 80, 64), unknown_slab=0).frame(16)) == PINS["drive_96x80x64_16_slab0"]


def test_serpentines():
    lab, cells = sc.serpentine_labels((150, 36, 20))
    assert digest(lab, cells) == PINS["serpentine_150x36x20"]
    assert digest(cells) == digest(sc.serpentine_cells((150, 36, 20), 2, 1))
    assert digest(sc.serpentine_cells((128, 128, 24), 4, 2)) == PINS["serpentine_cells_128x128x24_p4_m2"]


def test_random_boxes():
    assert digest(np.array(sc.random_boxes(np.random.default_rng(3), 24, 60, 6, 26))) == PINS["random_boxes"]


def test_world_points():
    stub = types.SimpleNamespace(pivot=lambda: (-37, 12, 5), cfg=types.SimpleNamespace(voxel_width=0.1))
    rng = np.random.default_rng(11)
    vi = rng.integers(-5, 100, (50, 3))
    vf = rng.uniform(-5, 100, (50, 3)).astype(np.float32)
    jit = rng.uniform(-0.4, 0.4, (50, 3))
    assert digest(sc.world(stub, vi)) == PINS["world_int"]
    assert digest(sc.world(stub, vf)) == PINS["world_f32"]
    assert digest(sc.world(stub, vi, jit)) == PINS["world_int_jitter"]
    assert digest(sc.world(stub, vf, jit)) == PINS["world_f32_jitter"]
    assert digest(sc.world(stub, vi, pvt=(-37, 12, 5))) == PINS["world_int"]

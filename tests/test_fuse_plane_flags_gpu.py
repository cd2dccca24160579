"""The per-plane obstacle flags gie_fuse leaves (k_fuse_rows: one lane per wave and layer that holds an obstacle stores the flag)
and EDT pass Y behind them (a linear grid, (strip, z) from the workgroup index: gie_edty_strip; planes without a flag are skipped),
bit for bit against the oracle: the types after fuse(), then dist_sq and coc of read_batch_edt().

* volumes with one, two, three (odd) and nine (more than eight) strips of pass Y, a partial last strip, Y not a multiple of 16, Z that
  cuts the last block, and one with X % 4 != 0 (the byte form k_edt_y);
* every volume at a block-aligned pivot and at one that is 3, 5 and 6 voxels off block alignment on x, y and z (the eight layers of a
  virtual wave then reach below plane 0 and beyond plane Z - 1);
* obstacles in planes 0, one middle plane and Z - 1 only: the planes between them must stay unflagged (pass Y skips them);
* three updates: the middle plane's obstacles are observed free in the second (its flag must be 0 again) and put back in the third;
* both feeds: labels (the byte-parallel row filter of k_fuse_rows<false>) and a point cloud (k_fuse_rows<true>; in the second update
  rays to points below the volume pass through the middle plane's obstacles).

Every case runs on the product library (gie.Mapper) and on the test build of the same sources, whose gie_debug_plane_flags hook copies
the flags out.  The oracle's side of a case is computed once."""
import ctypes as C
import functools

import numpy as np
import pytest

import gie
import stage_common as sc

pytestmark = pytest.mark.gpu

VOLUMES = [(64, 48, 24), (72, 40, 9), (128, 16, 8), (192, 33, 17), (520, 24, 5), (70, 20, 6)]
PIVOTS = {"aligned": (8, 16, -8), "off356": (8 + 3, 16 + 5, -8 + 6)}
FEEDS = ("labels", "cloud")
W = sc.W
N_RAYS = 6                                                   # rays through a middle-plane obstacle in the second update of the cloud feed


def planes(size):
    """the three planes that hold obstacles: 0, the one below the sensor's, Z - 1"""
    Z = size[2]
    return 0, Z // 2 - 1, Z - 1


def obstacles(size):
    """{plane: local voxels [n, 3]} — about 4 % of each of the three planes, the corners of the volume's x-y face among them"""
    X, Y, Z = size
    rng = np.random.default_rng(X * 1000 + Z)
    out = {}
    for z in planes(size):
        m = rng.random((Y, X)) < 0.04
        m[0, 0] = m[Y - 1, X - 1] = m[0, X - 1] = m[Y - 1, 0] = True
        yy, xx = np.nonzero(m)
        out[z] = np.stack([xx, yy, np.full_like(xx, z)], -1)
    return out


def frames(size, pvt, feed):
    """[(pos, scan)] of the three updates: scan is a label plane [Z][Y][X] or sensor-frame points [n, 3]"""
    X, Y, Z = size
    s = np.array([X // 2, Y // 2, Z // 2])                   # the sensor's voxel (local): gie_set_pose puts the pivot size // 2 below it
    pos = ((np.array(pvt) + s).astype(np.float32) * np.float32(W)).astype(np.float32)
    ob = obstacles(size)
    z0, zm, z1 = planes(size)
    out = []
    for k in range(3):
        live = [z0, z1] + ([zm] if k != 1 else [])
        if feed == "labels":
            lab = np.ones((Z, Y, X), np.int8)
            for z in live:
                lab[z, ob[z][:, 1], ob[z][:, 0]] = 2
            lab[:, :, 5:9] = 0                                # a slab that is never observed (obstacles in it included)
            out.append((pos, lab))
        else:
            v = [ob[z] for z in live]
            if k == 1:                                        # points below the volume on the rays through the middle plane's obstacles
                d = (ob[zm] - s).astype(np.float64)
                v += [s + d * (s[2] + 2 + j) for j in range(N_RAYS)]
            g = (np.concatenate(v).astype(np.float64) + np.array(pvt)).astype(np.float32) * np.float32(W)
            out.append((pos, (g - pos).astype(np.float32)))
    return out


def run(m, size, pvt, feed, flags=None):
    """[(types after fuse, plane flags or None, dist_sq, coc)] of the three updates on mapper m"""
    res = []
    for pos, scan in frames(size, pvt, feed):
        m.set_pose(pos)
        assert tuple(m.pivot()) == tuple(pvt)
        m.ogm_labels(scan) if feed == "labels" else m.ogm_pointcloud(scan)
        m.fuse()
        ty = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
        fl = flags(m) if flags else None
        m.batch_edt()
        e = m.read_batch_edt()
        m.merge()
        res.append((ty, fl, e["dist_sq"], e["coc"]))
    return res


@functools.lru_cache(maxsize=None)
def oracle_side(size, pname, feed):
    from oracle_py import OracleMapper
    a = OracleMapper(gie.make_config(W, size, fast_mode=False, cutoff_dist=3.0))
    try:
        res = run(a, size, PIVOTS[pname], feed)
    finally:
        a.close()
    for r in res:
        for x in r:
            if x is not None:
                x.setflags(write=False)
    return res


def want_flags(ty):
    return (ty == 2).any(axis=(1, 2)).astype(np.uint8)


def hook_flags(m):
    import hooks_py
    f = hooks_py._lib.gie_debug_plane_flags
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    out = np.full(m.size[2] + 8, 0x55, np.uint8)              # (guard bytes behind the Z flags)
    if f(m._h, out.ctypes.data_as(C.c_void_p)):
        raise RuntimeError(m._err())
    assert (out[m.size[2]:] == 0x55).all()
    return out[:m.size[2]]


@pytest.mark.parametrize("feed", FEEDS)
@pytest.mark.parametrize("pname", list(PIVOTS))
@pytest.mark.parametrize("size", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_plane_flags_and_pass_y_against_the_oracle(oracle_lib, size, pname, feed):
    import hooks_py
    hooks_py.load()
    want = oracle_side(size, pname, feed)
    z0, zm, z1 = planes(size)
    # what the case is about, stated on the oracle's types: obstacles in the three planes only, none in the middle one after the
    # second update, there again after the third
    for k, (ty, _, _, _) in enumerate(want):
        fl = want_flags(ty)
        assert set(np.nonzero(fl)[0]) == ({z0, z1} | ({zm} if k != 1 else set())), (k, np.nonzero(fl)[0])
    cfg = gie.make_config(W, size, fast_mode=False, cutoff_dist=3.0)
    for make, flags in ((gie.Mapper, None), (hooks_py.HooksMapper, hook_flags)):
        b = make(cfg)
        try:
            got = run(b, size, PIVOTS[pname], feed, flags)
        finally:
            b.close()
        for k, ((ty, _, d, c), (gty, gfl, gd, gc)) in enumerate(zip(want, got)):
            assert np.array_equal(ty, gty), (make.__name__, k, "type")
            if gfl is not None:
                assert np.array_equal(gfl, want_flags(ty)), (k, gfl)
            assert np.array_equal(d, gd), (make.__name__, k, "dist_sq")
            assert np.array_equal(c, gc), (make.__name__, k, "coc")

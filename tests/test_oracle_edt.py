"""Pins the oracle's batch-EDT stage (EDTphase1-3 restatement) against the mathematical
definition (brute force), and pins the closest-obstacle tie rule the HIP kernels rely on."""
import numpy as np
import pytest

import gie
from oracle_py import OracleMapper, brute_force_edt


def _edt(shape_xyz, occ):
    cfg = gie.make_config(0.1, shape_xyz)
    m = OracleMapper(cfg)
    t = np.where(occ, 2, 1).astype(np.int8)
    d, c = m.edt_only(t)
    m.close()
    return d, c


@pytest.mark.parametrize("shape,dens,seed", [
    ((24, 24, 24), 0.02, 1), ((32, 32, 32), 0.005, 2), ((40, 40, 16), 0.01, 3), ((32, 48, 16), 0.002, 4),
    ((48, 32, 16), 0.02, 5), ((16, 16, 1), 0.05, 6), ((33, 17, 9), 0.01, 7), ((8, 8, 8), 0.3, 8),
    ((64, 64, 24), 0.0005, 9), ((20, 20, 20), 1.0, 10),
])
def test_edt_matches_brute_force(oracle_lib, shape, dens, seed):
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    occ = rng.random((Z, Y, X)) < dens
    if not occ.any():
        occ[Z // 2, Y // 3, X // 4] = True
    d, c = _edt(shape, occ)
    bf = brute_force_edt(occ.astype(np.int8))
    assert np.array_equal(d, bf)
    # witness: coc is an obstacle at exactly that distance
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    assert (c >= 0).all()
    dd = (c[..., 0] - xx) ** 2 + (c[..., 1] - yy) ** 2 + (c[..., 2] - zz) ** 2
    assert np.array_equal(dd, d)
    assert occ[c[..., 2], c[..., 1], c[..., 0]].all()


def test_empty_volume_is_invalid(oracle_lib):
    d, c = _edt((12, 10, 8), np.zeros((8, 10, 12), bool))
    assert (c == -1).all()
    assert (d >= (12 + 10 + 8) ** 2).all()


from edt_reference import tie_rule_reference as _tie_rule_reference      # noqa: E402  (shared with the batch EDT's form table)


@pytest.mark.parametrize("shape,dens,seed", [
    ((16, 16, 16), 0.05, 11), ((24, 12, 8), 0.02, 12), ((9, 31, 5), 0.1, 13), ((32, 32, 8), 0.004, 14),
    ((12, 12, 12), 0.5, 15), ((20, 7, 11), 0.01, 16),
])
def test_meijster_tie_rule(oracle_lib, shape, dens, seed):
    """The literal Meijster scans of the oracle pick exactly the closed-form argmin with the
    tie rule above — so a kernel may compute the envelope any way it likes as long as it keeps
    that rule."""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    occ = rng.random((Z, Y, X)) < dens
    occ[Z // 2, Y // 2, X // 2] = True
    d, c = _edt(shape, occ)
    rd, rc = _tie_rule_reference(occ)
    assert np.array_equal(d, rd)
    assert np.array_equal(c, rc)


def test_tie_rule_exhaustive_1d(oracle_lib):
    """All 2^10 occupancy patterns of a 10x1x1 row and of a 1x1x10 column, plus structured 2-D cases."""
    for n in range(1, 1 << 10):
        bits = np.array([(n >> i) & 1 for i in range(10)], bool)
        for shape, occ in (((10, 1, 1), bits.reshape(1, 1, 10)), ((1, 10, 1), bits.reshape(1, 10, 1)),
                           ((1, 1, 10), bits.reshape(10, 1, 1))):
            d, c = _edt(shape, occ)
            rd, rc = _tie_rule_reference(occ)
            assert np.array_equal(d, rd) and np.array_equal(c, rc), (n, shape)


@pytest.mark.parametrize("toggle,sensor", [(0.0, "depth"), (0.0, "lidar_points"), (0.3, "depth"), (0.3, "mixed")])
def test_incremental_field_against_the_definition(oracle_lib, toggle, sensor):
    """The whole incremental pipeline (OGM → fuse → batch EDT → Mark / frontiers / waves → commit)
    checked against the DEFINITION of what it maintains, in a static and in a changing world (30 % of
    the obstacles toggle) observed from a moving robot: for every known voxel of the local volume
      * the stored closest obstacle is a voxel the global map believes OCCUPIED, at exactly the
        stored distance (witness), and
      * the stored distance is never below the true distance to the nearest believed-occupied
        voxel of the global map region around the volume (the waves may leave an over-estimate —
        SURVEY App. C measured <= 0.17 voxel in a few voxels — but can never invent a closer
        obstacle), and equals it for the vast majority."""
    from parity import Scenario
    from gie import scenes
    sc = Scenario("definition", (40, 36, 16), sensor=sensor, frames=10, delta_vox=3, yaw_deg=20.0, toggle=toggle, cutoff_dist=3.0,
                  lidar_az=360)
    m = OracleMapper(sc.config())
    try:
        for pos, q, kind, data, kw in sc.frames_iter():
            m.update(pos, q, kind, data, **kw)
        r = m.read_local()
        pv = np.array(m.pivot())
        X, Y, Z = sc.size
        # the map's belief in a generous region around the volume
        mg = 20
        gx, gy, gz = np.meshgrid(np.arange(-mg, X + mg), np.arange(-mg, Y + mg), np.arange(-mg, Z + mg), indexing="ij")
        reg = (np.stack([gx, gy, gz], -1).reshape(-1, 3) + pv).astype(np.int32)
        g = m.query_global(reg)
        occ = reg[g["vox_type"] == 2]
        assert len(occ) > 50
        known = (r["type"] != 0) & (r["dist_sq"] < 900000)
        zz, yy, xx = np.nonzero(known)
        vox = np.stack([xx, yy, zz], -1) + pv
        d = r["dist_sq"][known].astype(np.int64)
        coc = r["coc"][known].astype(np.int64)
        assert np.array_equal(((coc - vox) ** 2).sum(-1), d)                     # witness distance
        w = m.query_global(coc.astype(np.int32))
        assert (w["vox_type"] == 2).all()                                        # witness is believed occupied
        from scipy.spatial import cKDTree
        true_d, _ = cKDTree(occ).query(vox)
        true_sq = np.rint(true_d ** 2).astype(np.int64)
        inside = true_sq <= (mg - 1) ** 2                                        # nearest obstacle certainly inside the probed region
        assert (d[inside] >= true_sq[inside]).all()                              # never closer than the truth
        assert (d[inside] == true_sq[inside]).mean() > 0.995                     # measured: 1.0 / 1.0 / 1.0 / 0.9997
    finally:
        m.close()


@pytest.mark.parametrize("shape,dens,seed,threads", [
    ((32, 32, 32), 0.01, 1, 1), ((64, 48, 40), 0.002, 2, 3), ((33, 70, 17), 0.05, 3, 8), ((1, 40, 1), 0.1, 4, 2),
    ((50, 1, 30), 0.03, 5, 4), ((24, 24, 24), 1.0, 6, 5), ((40, 40, 40), 0.00002, 7, 8),
])
def test_edt_mt_equals_brute_force(oracle_lib, shape, dens, seed, threads):
    """The full-size CPU baseline (multi-threaded separable EDT, oracle/edt_mt.c) is exact: its
    squared distances equal the O(N*M) brute force, and its closest obstacle is an occupied voxel at
    exactly that distance."""
    from oracle_py import EDT_MT_NONE, brute_force_edt, edt_mt
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    occ = rng.random((Z, Y, X)) < dens
    occ[Z // 2, Y // 2, X // 2] = True
    ty = np.where(occ, 2, 1).astype(np.int8)
    d, c = edt_mt(ty, nthreads=threads)
    assert np.array_equal(d, brute_force_edt(occ.astype(np.int8)))
    cx, cy, cz = c & 1023, (c >> 10) & 1023, c >> 20
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    assert occ[cz, cy, cx].all()
    assert np.array_equal((xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2, d)
    d0, c0 = edt_mt(np.ones((6, 5, 4), np.int8), nthreads=2)
    assert (d0 == EDT_MT_NONE).all() and (c0 == -1).all()

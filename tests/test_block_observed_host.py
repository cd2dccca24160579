"""gie_block_observed (gie_ops.h) on the host: the question gie_fuse's block allocation asks of a label plane left in place — does
table cell (bx, by, bz) hold an observed voxel inside the local volume? — against a plain numpy statement of it, for every pivot
residue modulo 8, and with the plane embedded in bytes that are all OCCUPIED: a read outside the plane shows as a wrong answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("probe") / "libblock_observed_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "emu", "block_observed_probe.cpp")])
    lib = C.CDLL(so)
    lib.gie_probe_block_observed.restype = None
    lib.gie_probe_block_observed.argtypes = [C.c_void_p] * 6

    def run(lab, pvt, guard_value=2):
        Z, Y, X = lab.shape
        buf = np.full(GUARD + lab.size + GUARD, guard_value, np.int8)
        buf[GUARD:GUARD + lab.size] = lab.ravel()
        tb0 = np.array([(pvt[i] >> 3) - 1 for i in range(3)], np.int32)
        tdim = np.array([((pvt[i] + s - 1) >> 3) - int(tb0[i]) + 2 for i, s in enumerate((X, Y, Z))], np.int32)
        out = np.zeros(int(tdim.prod()), np.uint8)
        size = np.array([X, Y, Z], np.int32)
        p = np.array(pvt, np.int32)
        lib.gie_probe_block_observed(buf.ctypes.data + GUARD, size.ctypes.data, p.ctypes.data, tb0.ctypes.data, tdim.ctypes.data, out.ctypes.data)
        assert np.array_equal(buf[:GUARD], np.full(GUARD, guard_value, np.int8))
        return out.reshape(tdim[2], tdim[1], tdim[0]), tb0
    return run


def _want(lab, pvt, tb0, shape):
    want = np.zeros(shape, np.uint8)
    z, y, x = np.nonzero((lab == 1) | (lab == 2))
    want[((z + pvt[2]) >> 3) - tb0[2], ((y + pvt[1]) >> 3) - tb0[1], ((x + pvt[0]) >> 3) - tb0[0]] = 1
    return want


@pytest.mark.parametrize("size", [(16, 9, 17), (32, 24, 8), (8, 8, 8), (5, 3, 1)], ids=lambda s: "x".join(map(str, s)))
def test_every_pivot_residue_against_numpy(probe, size):
    X, Y, Z = size
    rng = np.random.default_rng(1)
    values = np.array([0, 0, 0, 0, 0, 0, 1, 2, 3, 127, -1, -128], np.int8)
    for r in range(8):
        for pvt in ((r - 16, (r * 3) % 8 - 8, (r * 5) % 8 + 8), ((r * 5) % 8, r - 24, (r * 3) % 8 - 16), ((r * 3) % 8 + 40, (r * 5) % 8, r - 8)):
            lab = rng.choice(values, size=(Z, Y, X))
            lab[rng.random(lab.shape) < 0.9] = 0              # a few observations, most blocks with none
            got, tb0 = probe(lab, pvt)
            assert np.array_equal(got, _want(lab, pvt, tb0, got.shape)), (pvt,)
            one = np.zeros((Z, Y, X), np.int8)                # a single observation: the last voxel, the first
            for at in ((Z - 1, Y - 1, X - 1), (0, 0, 0)):
                one[:] = 0
                one[at] = 2
                got, tb0 = probe(one, pvt)
                assert got.sum() == 1 and np.array_equal(got, _want(one, pvt, tb0, got.shape)), (pvt, at)


@pytest.mark.parametrize("size", [(16, 9, 17), (32, 24, 8), (5, 3, 1)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_outside_the_plane_is_read(probe, size):
    """an all-unknown plane between OCCUPIED (and FREE) guard bytes: no cell may answer yes, whatever the pivot"""
    X, Y, Z = size
    lab = np.zeros((Z, Y, X), np.int8)
    for gv in (2, 1):
        for rx in range(8):
            for ry in (0, 1, 7):
                for rz in (0, 1, 7):
                    got, _ = probe(lab, (rx - 8, ry, rz + 8), guard_value=gv)
                    assert not got.any(), (rx, ry, rz)


def test_labels_that_are_not_observations(probe):
    for v in range(-128, 128):
        lab = np.full((8, 8, 16), v, np.int8)
        got, _ = probe(lab, (0, 0, 0))
        assert bool(got.any()) == (v in (1, 2)), v

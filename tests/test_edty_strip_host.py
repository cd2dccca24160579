"""gie_edty_strip (gie_ops.h) on the host: EDT pass Y launches a linear grid of 16 * gie_edty_groups(nstrip, Z) workgroups and each
derives its (strip, z) from its index.  For every strip count 1..17 and every Z 1..40 the launch's indices must take every
(strip, z) exactly once, the rest must be refused; and the two strips 2p, 2p + 1 that share the 128-byte lines of a plane must
sit at indices that are equal modulo 8 and eight apart (what the mapping is for: one XCD fetches the line for both)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("probe") / "libedty_strip_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "emu", "edty_strip_probe.cpp")])
    lib = C.CDLL(so)
    lib.gie_probe_edty_grid.restype = C.c_int
    lib.gie_probe_edty_grid.argtypes = [C.c_int, C.c_int]
    lib.gie_probe_edty_strip.restype = None
    lib.gie_probe_edty_strip.argtypes = [C.c_int, C.c_int, C.c_void_p]

    def run(nstrip, Z):
        n = lib.gie_probe_edty_grid(nstrip, Z)
        out = np.full((n + 1, 3), -7, np.int32)              # one guard row
        lib.gie_probe_edty_strip(nstrip, Z, out.ctypes.data)
        assert (out[n] == -7).all()
        return out[:n]
    return run


def test_every_strip_and_plane_exactly_once(probe):
    for nstrip in range(1, 18):
        for Z in range(1, 41):
            t = probe(nstrip, Z)
            n = len(t)
            assert n % 16 == 0 and n >= nstrip * Z, (nstrip, Z, n)
            assert n < 2 * ((nstrip + 1) // 2) * Z + 16, (nstrip, Z, n)        # no more padding than the odd strip and one group
            ok = t[:, 0] != 0
            assert set(np.unique(t[:, 0])) <= {0, 1}
            s, z = t[ok, 1], t[ok, 2]
            assert ((s >= 0) & (s < nstrip) & (z >= 0) & (z < Z)).all(), (nstrip, Z)
            seen = np.zeros((Z, nstrip), np.int32)
            np.add.at(seen, (z, s), 1)
            assert (seen == 1).all(), (nstrip, Z)


def test_the_two_strips_of_a_line_are_eight_apart(probe):
    for nstrip in range(1, 18):
        for Z in (1, 2, 7, 8, 9, 40):
            t = probe(nstrip, Z)
            at = {(int(s), int(z)): l for l, (ok, s, z) in enumerate(t) if ok}
            for (s, z), l in at.items():
                if s % 2 == 0 and s + 1 < nstrip:
                    assert at[(s + 1, z)] == l + 8, (nstrip, Z, s, z)

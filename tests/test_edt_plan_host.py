"""gie_edt_plan_for (gie_edt_plan.h) on the host: the one statement of which kernels the batch EDT launches, with which template
arguments, grids and scalar arguments — what be_edt and be_edt_z (gie_hip.hip) execute — compiled with g++ and held against the
restatement in edt_forms.py: the kernel names for every size of the table, every row of test_host_forms_by_hand and a sweep of
the rules' borders, each under every guess, full = 0 / 1, update / completion and the GIE_ZS_FUSED switch on and off; the streaming
kernel's z segments; and the arithmetic the kernels rely on."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import edt_forms as F
from test_edt_forms import HAND_ROWS

HERE = os.path.dirname(os.path.abspath(__file__))
GUESSES = (F.NONE, F.LEFT, F.TOOK)
CUS = (16, 256, 1024)


class Probe:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.gie_probe_edt_plan_fields.restype = C.c_char_p
        lib.gie_probe_edt_plan.restype = None
        lib.gie_probe_edt_plan.argtypes = [C.c_int] * 8 + [C.c_void_p]
        lib.gie_probe_edt_plan_consts.restype = None
        lib.gie_probe_edt_plan_consts.argtypes = [C.c_void_p]
        self.lib = lib
        self.fields = lib.gie_probe_edt_plan_fields().decode().split(",")
        k = np.full(17, -7, np.int32)
        lib.gie_probe_edt_plan_consts(k.ctypes.data)
        assert k[16] == -7 and (k[:16] != -7).all()
        self.y_names = dict(zip(k[1:6].tolist(), F.Y_KERNELS))           # (the enumerators are in F.Y_KERNELS' order)
        self.y_none = int(k[0])
        assert tuple(k[6:9]) == (F.NONE, F.LEFT, F.TOOK)
        self.edty_cols, self.edty4_lanes, self.edtx_waves, self.zstream_waves, self.tx, self.waves, self.lds_bytes = k[9:16].tolist()

    def __call__(self, size, cu_total=F.CU_TOTAL, full=1, guess=F.NONE, completion=False, fused_switch=True):
        out = np.full(len(self.fields) + 1, -7, np.int32)                 # one guard word
        self.lib.gie_probe_edt_plan(size[0], size[1], size[2], cu_total, int(full), guess, int(completion), int(fused_switch), out.ctypes.data)
        assert out[-1] == -7 and (out[:-1] != -7).all()
        return dict(zip(self.fields, out[:-1].tolist()))

    def names(self, p):
        """the kernel names the executor announces for plan p (blanks removed, as the GPU test reads the trace)"""
        out = set()
        if p["y_kernel"] != self.y_none:
            out.add(self.y_names[p["y_kernel"]])
        if p["x"]:
            out.add("k_edt_x<%d>" % p["cp_x"])
        if p["stream"]:
            out.add("k_edt_z_stream<%s>" % ("true" if p["stream_fused"] else "false"))
        if p["direct"]:
            out.add("k_edt_z_direct")
        if p["redo"]:
            out.add("k_edt_x_redo<%d>" % p["cp_x"])
        out.add("k_edt_z<%d,%d,%d>" % (p["cp_z"], self.tx, self.waves))
        return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("probe") / "libedt_plan_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "emu", "edt_plan_probe.cpp")])
    return Probe(so)


def border_sizes():
    """every border of the rules: Z around the streaming form's range, X even / odd and X % 4, Y around pass Y's kernels, X and Z
    around every CP's range"""
    lines = (64, 65, 128, 129, 256, 257, 512, 513)
    out = set()
    for Z in (63, 64, 1024, 1025):
        for X in (8, 9, 10, 11):                                     # even / odd, X % 4 zero and not
            for Y in (256, 257, 512, 513):
                out.add((X, Y, Z))
    for X in lines + (66, 130, 258, 514):                           # (the odd side of a CP's border again with X even: the fused form)
        for Z in lines:
            out.add((X, 24, Z))
    for X in lines:                                           # ... with Y at pass Y's borders and Z at the form's
        for Y in (256, 257, 512, 513):
            for Z in (63, 64):
                out.add((X, Y, Z))
    return sorted(out)


ALL_SIZES = sorted({c.size for c in F.CASES} | {r[0] for r in HAND_ROWS} | set(border_sizes()))


def test_the_sweep_holds_the_borders():
    s = border_sizes()
    assert {z for _, _, z in s} >= {63, 64, 1024, 1025} and {y for _, y, _ in s} >= {256, 257, 512, 513}
    assert {x % 4 for x, _, z in s if z in (63, 64, 1024, 1025)} == {0, 1, 2, 3}
    lines = {64, 65, 128, 129, 256, 257, 512, 513}
    assert {(x, z) for x, _, z in s} >= set(itertools.product(lines, lines))
    assert {F.cp_of(x) for x, _, _ in s} == set(F.CPS) and {F.cp_of(z) for _, _, z in s} == set(F.CPS)
    assert {F.pass_y_kernel(x, y)[0] for x, y, _ in s} == set(F.Y_KERNELS)


def test_kernel_names_equal_host_forms(probe):
    seen = set()
    for size in ALL_SIZES:
        for guess, full, completion, sw in itertools.product(GUESSES, (0, 1), (False, True), (True, False)):
            p = probe(size, F.CU_TOTAL, full, guess, completion, sw)
            want = F.host_forms(size, 1, 1, full, completion, guess, sw)
            assert probe.names(p) == want, (size, guess, full, completion, sw, p)
            seen |= want
    # the sweep reaches every kernel the batch EDT has
    assert seen >= set(F.Y_KERNELS) | {"k_edt_z_direct", "k_edt_z_stream<true>", "k_edt_z_stream<false>"}
    for cp in F.CPS:
        assert {"k_edt_x<%d>" % cp, "k_edt_x_redo<%d>" % cp, "k_edt_z<%d,16,8>" % cp} <= seen


def test_the_rows_read_off_by_hand(probe):
    for size, full, completion, guess, want in HAND_ROWS:
        assert probe.names(probe(size, F.CU_TOTAL, full, guess, completion)) == want, (size, full, completion, guess)


def test_the_guess_counts_only_where_the_fused_form_may_take_the_volume(probe):
    for size in ALL_SIZES:
        X, Y, Z = size
        for guess, full, completion, sw in itertools.product(GUESSES, (0, 1), (False, True), (True, False)):
            p = probe(size, F.CU_TOTAL, full, guess, completion, sw)
            host = F.zs_mode(X, Z, sw)
            counts = host == 2 and not completion
            assert p["guess"] == (guess if counts else F.NONE)
            assert p["zs"] == (1 if counts and guess == F.LEFT else host)
            none = probe(size, F.CU_TOTAL, full, F.NONE, completion, sw)
            if not counts:
                assert p == none
            # the scalar arguments: pass X is told of the fused form alone; the streaming kernel gets the guess and the hint word from
            # an update and not from a completion; the fused kernel is the one launched with zs = 2
            assert p["x_zs"] == (2 if p["zs"] == 2 else 0)
            assert p["x"] == (not completion and p["guess"] != F.TOOK)
            assert p["stream"] == (p["zs"] != 0) and p["stream_fused"] == (p["zs"] == 2) and p["redo"] == (p["zs"] == 2)
            assert p["stream_note"] == (not completion)
            assert p["direct"] == (p["zs"] == 0 and not full and not completion)


def test_cp_and_pass_y_agree(probe):
    for size in ALL_SIZES:
        X, Y, Z = size
        p = probe(size, F.CU_TOTAL, 0)
        assert (p["cp_x"], p["cp_z"]) == (F.cp_of(X), F.cp_of(Z))
        kern, share = F.pass_y_kernel(X, Y)
        assert probe.y_names[p["y_kernel"]] == kern
        # the launch: a thread's share times the threads along y covers the column; the strips cover the row; 16 workgroups a group
        cols = probe.edty4_lanes * 4 if kern.startswith("k_edt_y4") else probe.edty_cols
        assert p["y_block_x"] * (4 if kern.startswith("k_edt_y4") else 1) == cols
        assert p["y_block_y"] * share >= Y and p["y_block_x"] * p["y_block_y"] <= 1024
        if kern.startswith("k_edt_y4"):
            assert (p["y_block_y"] - 1) * share < Y                       # (k_edt_y4: no row of threads without a row)
        nstrip = (X + cols - 1) // cols
        assert p["y_grid"] % 16 == 0 and p["y_grid"] >= nstrip * Z
        assert p["y_grid"] < 2 * ((nstrip + 1) // 2) * Z + 16             # (test_edty_strip_host.py: the padding)
        assert (p["x_grid_x"], p["x_grid_y"]) == ((Y + probe.edtx_waves - 1) // probe.edtx_waves, Z)
        c = probe(size, F.CU_TOTAL, 1, F.NONE, True)
        assert c["y_kernel"] == probe.y_none and not c["x"]


def test_stream_segments_and_grids(probe):
    assert probe.zstream_waves == F.ZS_WAVES
    for size in sorted({c.size for c in F.CASES}):
        for cu in CUS:
            want = F.stream_segments(size, cu)                            # (asserts that the device does not matter on the table's volumes)
            for full in (0, 1):
                p = probe(size, cu, full)
                assert (p["nseg"], p["seg_len"]) == want, (size, cu)
    for size in ALL_SIZES:
        X, Y, Z = size
        for cu, full, completion in itertools.product(CUS, (0, 1), (False, True)):
            p = probe(size, cu, full, F.NONE, completion)
            assert 1 <= p["stream_grid"] <= cu * 32
            if not full:
                assert p["stream_grid"] >= cu * 16 == p["direct_grid"]    # (the list form rides in this launch: its own kernel's grid)
            assert p["seg_len"] % 32 == 0 and p["nseg"] >= 1 and p["nseg"] * p["seg_len"] >= Z
            assert (p["nseg"] - 1) * p["seg_len"] < Z                     # (no segment without a plane)
            assert p["nseg"] <= max(Z // 64, 1)
            assert p["redo_grid"] == cu * 8
            # the column kernel: LDS as k_edt_z lays it out (column tile + per-wave sites + plane list), tiles in pairs
            lp = 64 * p["cp_z"]
            assert p["col_lds"] == ((Z * (probe.tx + 1) + 3) & ~3) * 4 + probe.waves * lp * 8 + lp * 2 + 16
            if Z <= 1024:
                assert p["col_lds"] <= probe.lds_bytes == 160 * 1024
            assert (p["col_ntx"], p["col_ntiles"]) == ((X + probe.tx - 1) // probe.tx, (X + probe.tx - 1) // probe.tx * Y)
            assert 1 <= p["col_grid"] <= min(4 * cu, (p["col_ntiles"] + 1) // 2)
            fit = max(1, min(4, probe.lds_bytes // (p["col_lds"] + 256)))
            assert p["col_grid"] == min(fit * cu, (p["col_ntiles"] + 1) // 2)

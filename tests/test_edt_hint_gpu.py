"""The batch EDT launches its passes for a guess (be_edt takes it, gie_edt_plan_for in gie_edt_plan.h states what it changes —
tests/test_edt_plan_host.py holds that statement against edt_forms.host_forms for every guess without a GPU): "pass Z's fused streaming form took the last volume" — pass X is not
launched, and where the form does not take this volume after all k_edt_x_redo does every row and the column kernel every tile
(GIE_CNT_XMISS) —, "it did not" — pass X in full, the streaming form from pass X's planes, no k_edt_x_redo —, or none (both
launches, as before).  The guess comes from a word the device stores and the host reads without waiting, so a test cannot make it
wrong on purpose: the test build's gie_debug_edt_hint forces it.  Whatever the guess, every update equals the oracle bit for bit.

Every volume is driven through six label-feed updates:

    0  obstacles in every plane
    1  in half the planes                       (a forced / inherited "took" is wrong here wherever it was right before)
    2  in every plane again                     ("did not take" is wrong where the form takes the volume)
    3  a jump of 40 voxels, every plane
    4  every plane, with a pocket without obstacles that is more than 24 voxels deep (planes without obstacles where the volume is
       too narrow for that): trips redone with the wide window, slabs given up (k_edt_x_redo + the column kernel's repair)
    5  in 6 planes of 10

with an x-slab that is not observed and, at the face the volume moves towards, new to the map in every update, so that wave B
asks for the batch distance of UNKNOWN neighbours (gie_batch_dist_direct) in every update — right after a wrong guess of either
kind among them.  After every update read_local (edt, type, dist_sq, coc: what the merge made of the pass) and read_batch_edt
(dist_sq, coc: the completion of the partial pass, behind the same launches) are compared with the oracle, after the last one a
probe of the global map.

The volumes: 64 x 16 x 64 (eight tiles high: pass Z's list form, which a wrong "took" has to keep from reading planes pass X has
not written), 72 x 24 x 96 (a partial 64-column strip, Y not a multiple of 16), 16 x 16 x 128 (X narrower than a wave).  No
volume of at most 160 planes can hold more than GIE_BAND_MAXK = 160 planes with obstacles, so on these three the form never takes
the volume: "took" is wrong on every update.  64 x 16 x 192, 72 x 24 x 176 and 16 x 16 x 224 are the same volumes made tall
enough to cross the threshold in both directions (updates 1 and 5 below it, the others above).

Each sequence runs with the guess forced to each of its three values on every update and left alone on the test build, left alone
on the product library, and — in one child process for all volumes, since the switch is read once per process — with
GIE_EDT_HINT=0.  The counts of wrong guesses the device keeps tell that each run met the updates it is about."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gie
import parity

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W = 0.1
SHORT = [(64, 16, 64), (72, 24, 96), (16, 16, 128)]
TALL = [(64, 16, 192), (72, 24, 176), (16, 16, 224)]
VOLUMES = SHORT + TALL
MAXK = 160                                                   # GIE_BAND_MAXK
NONE, LEFT, TOOK = 0, 1, 2                                   # GIE_EDT_HINT_*
UPDATES = 6


def _id(size):
    return "x".join(map(str, size))


def allowed_planes(size, k):
    """the local z planes that hold obstacles in update k"""
    X, Y, Z = size
    if k == 1:
        return np.arange(0, Z, 2)
    if k == 5:
        return np.array([z for z in range(Z) if z % 10 < 6])
    if k == 4 and X < 50:                                    # too narrow for a pocket: 52 planes without obstacles
        return np.array([z for z in range(Z) if not (Z // 2 - 26 <= z < Z // 2 + 26)])
    return np.arange(Z)


def takes(size, k):
    """gie_zs_takes of update k: more than GIE_BAND_MAXK planes with obstacles (these volumes are swept, or eight tiles high)"""
    return len(allowed_planes(size, k)) > MAXK and size[2] > 64


def slab(size):
    """the local x columns that are not observed: near the face the volume moves towards, so that they are new to the map"""
    return size[0] - 4, size[0] - 1


def pivot(size, k):
    return (3 * k + (40 if k >= 3 else 0) - size[0] // 2, -(size[1] // 2), -(size[2] // 2))


def frame(size, k):
    """(pos, labels [Z][Y][X]) of update k: obstacles fixed in the world (a hash of the global voxel, 3 %), one more in every
    plane that is to hold any, none in the other planes, the pocket, the slab"""
    X, Y, Z = size
    pvt = np.array(pivot(size, k))
    pos = ((pvt + np.array(size) // 2).astype(np.float32) * np.float32(W)).astype(np.float32)
    gz, gy, gx = np.meshgrid(np.arange(Z) + pvt[2], np.arange(Y) + pvt[1], np.arange(X) + pvt[0], indexing="ij")
    h = (gx * 73856093) ^ (gy * 19349663) ^ (gz * 83492791)
    lab = np.where((h % 1000) < 30, 2, 1).astype(np.int8)
    if k == 4 and X >= 50:
        lab[Z // 2 - 30:Z // 2 + 30, :, 4:60] = 1
    # (no obstacle ever in a column of the world that some update's slab covers: the map would remember it there, in a plane that
    # is to hold none)
    cols = [pivot(size, j)[0] + x for j in range(UPDATES) for x in range(*slab(size))]
    lab[:, :, np.isin(np.arange(X) + pvt[0], cols)] = 1
    keep = np.zeros(Z, bool)
    keep[allowed_planes(size, k)] = True
    lab[~keep] = 1
    lab[keep, 3, 1] = 2
    lab[:, :, slab(size)[0]:slab(size)[1]] = 0
    return pos, lab


def run(m, size, before=None, after=None):
    """the six updates on mapper m: [{"type", "edt", "dist_sq", "coc", "b.dist_sq", "b.coc"}], then {"global"}"""
    res = []
    for k in range(UPDATES):
        pos, lab = frame(size, k)
        m.set_pose(pos)
        assert tuple(m.pivot()) == pivot(size, k)
        m.ogm_labels(lab)
        if before:
            before(m, k)
        m.step()
        r = m.read_local()
        if after:
            after(m, k)
        e = m.read_batch_edt()
        r["b.dist_sq"], r["b.coc"] = e["dist_sq"], e["coc"]
        res.append(r)
    xyz = parity.probe_coords(m.pivot(), size, np.random.default_rng(5), n=4000, margin=12)
    g = m.query_global(xyz)
    res.append({key: np.ascontiguousarray(g[key]) for key in ("occ_val", "vox_type", "dist_sq", "coc")})
    return res


def config(size):
    return gie.make_config(W, size, fast_mode=False, cutoff_dist=2.0)


@functools.lru_cache(maxsize=None)
def oracle_side(size):
    from oracle_py import OracleMapper
    a = OracleMapper(config(size))
    try:
        res = run(a, size)
    finally:
        a.close()
    for r in res:
        for v in r.values():
            v.setflags(write=False)
    # what the sequence is about, stated on the oracle's types: the planes with obstacles are the ones meant
    for k in range(UPDATES):
        got = np.nonzero((res[k]["type"] == 2).any(axis=(1, 2)))[0]
        assert np.array_equal(got, allowed_planes(size, k)), (size, k)
    return res


def same(want, got, tag):
    assert len(want) == len(got)
    for k, (a, b) in enumerate(zip(want, got)):
        assert sorted(a) == sorted(b)
        for key in a:
            x, y = np.asarray(a[key]), np.asarray(b[key])
            if x.dtype.kind == "f":
                x, y = x.view(np.uint32), y.view(np.uint32)
            bad = int((x != y).sum())
            print("%s update %d %s: %d of %d differ" % (tag, k, key, bad, x.size))
            assert bad == 0, (tag, k, key, bad)


def hint_hook(m, force):
    """gie_debug_edt_hint: force the next update's guess (-1: leave it alone); (word, wrong LEFT, wrong TOOK, last guess)"""
    import hooks_py
    f = hooks_py._lib.gie_debug_edt_hint
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    info = np.zeros(4, np.int32)
    if f(m._h, int(force), info.ctypes.data_as(C.c_void_p)):
        raise RuntimeError(m._err())
    return [int(v) for v in info]


def wrong_guesses(size, guesses):
    """(wrong LEFT, wrong TOOK) of a run launched for guesses[k]"""
    wl = sum(1 for k, g in enumerate(guesses) if g == LEFT and takes(size, k))
    wt = sum(1 for k, g in enumerate(guesses) if g == TOOK and not takes(size, k))
    return wl, wt


@pytest.mark.parametrize("force", [NONE, LEFT, TOOK, -1], ids=["none", "left", "took", "alone"])
@pytest.mark.parametrize("size", VOLUMES, ids=_id)
def test_every_guess_on_every_update(oracle_lib, size, force):
    import hooks_py
    hooks_py.load()
    want = oracle_side(size)
    state = []

    def before(m, k):
        hint_hook(m, force)

    def after(m, k):
        word, _, _, guess = hint_hook(m, -1)
        ts = m.debug_tile_state()
        state.append((guess, word & 3, word >> 2, ts["zstream"], ts["zwide"], ts["zfail"]))

    b = hooks_py.HooksMapper(config(size))
    try:
        got = run(b, size, before, after)
        _, wl, wt, _ = hint_hook(b, -1)
    finally:
        b.close()
    print(_id(size), "force", force, "(guess, outcome, planes, zstream, zwide, zfail):", state, "wrong guesses", (wl, wt))
    same(want, got, "%s force %d" % (_id(size), force))
    # the updates met the launches they are about
    outcomes = [TOOK if takes(size, k) else LEFT for k in range(UPDATES)]
    guesses = [force] * UPDATES if force >= 0 else [NONE] + outcomes[:-1]      # (left alone: the update before, read after a wait)
    assert [s[0] for s in state] == guesses
    assert [s[1] for s in state] == outcomes
    assert [s[2] for s in state] == [len(allowed_planes(size, k)) for k in range(UPDATES)]
    assert [s[3] for s in state] == [int(takes(size, k)) for k in range(UPDATES)]
    assert (wl, wt) == wrong_guesses(size, guesses)
    if size in TALL:
        assert state[4][4] > 0 or state[4][5] > 0, state[4]            # the pocket: wide trips or slabs given up
        if size[0] >= 50:
            assert state[4][5] > 0, state[4]


@pytest.mark.parametrize("size", VOLUMES, ids=_id)
def test_product_library_left_alone(oracle_lib, size):
    want = oracle_side(size)
    b = gie.Mapper(config(size))
    try:
        got = run(b, size)
    finally:
        b.close()
    same(want, got, "%s product" % _id(size))


CHILD = r'''
import sys
sys.path[:0] = [ROOT, ROOT + "/gie-mapping_amd", HERE]
import numpy as np
import gie
import test_edt_hint_gpu as T
res = {}
for size in T.VOLUMES:
    b = gie.Mapper(T.config(size))
    try:
        got = T.run(b, size)
    finally:
        b.close()
    for k, r in enumerate(got):
        for key, v in r.items():
            res["%s/%d/%s" % (T._id(size), k, key)] = v
np.savez(sys.argv[1], **res)
print("ok")
'''


def test_switched_off(oracle_lib, tmp_path):
    """GIE_EDT_HINT=0: the launches of before on every update"""
    import hooks_py
    hooks_py.load()                                   # (builds the test library if need be, outside the child)
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, GIE_EDT_HINT="0", GIE_LIB=hooks_py.TEST_SO)
    r = subprocess.run([sys.executable, "-c", "ROOT, HERE = %r, %r\n" % (ROOT, HERE) + CHILD, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(out)
    for size in VOLUMES:
        want = oracle_side(size)
        got = [{key: z["%s/%d/%s" % (_id(size), k, key)] for key in r} for k, r in enumerate(want)]
        same(want, got, "%s off" % _id(size))

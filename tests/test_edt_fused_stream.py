"""Pass Z's fused streaming form (k_edt_z_stream<true>): it reads pass Y's planes and pass X is skipped when it takes the volume.
Every case runs twice, in a child process each (the library reads its switches once per process): with the fused form
(GIE_ZS_FUSED=1, the default) and with the form that reads pass X's planes (GIE_ZS_FUSED=0).  Both are compared with the oracle,
and with each other bit for bit.

* batch EDT alone on volumes the streaming form takes (Z >= 64, more than 160 planes with obstacles, X >= 128 and not a multiple
  of 64): a random field, a lattice with in-plane ties, pockets that need the wide trip and pockets that make slabs give up
  (k_edt_x_redo + the column kernel), an odd X (the fused form is not used there: pass X runs).  gie_read_batch_edt completes
  the partial pass Z of these updates, so the completion path runs with pass X skipped as well.
* a drive through a dense field with an unobserved slab (wave B looks up the batch distance of UNKNOWN neighbours,
  gie_batch_dist_direct) towards a pocket that makes slabs give up (their tiles' bounds for Mark's lazy tiles, tbmax): the
  local planes and the global map against the oracle after every update.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

EDT_CASES = {
    "dense_200": dict(shape=(200, 96, 192), dens=0.01, seed=1),
    "lattice": dict(shape=(192, 64, 176), lattice=(4, 4, 3), seed=2),
    "pockets": dict(shape=(256, 64, 192), dens=0.02, seed=3, pockets=[((40, 20, 30), 20), ((150, 2, 100), 60), ((220, 30, 170), 16)]),
    "odd_x": dict(shape=(201, 64, 176), dens=0.01, seed=4, pockets=[((100, 10, 80), 40)]),
}


def edt_occupancy(name):
    p = EDT_CASES[name]
    X, Y, Z = p["shape"]
    rng = np.random.default_rng(p["seed"])
    if "lattice" in p:
        lx, ly, lz = p["lattice"]
        zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        occ = (xx % lx == 1) & (yy % ly == 2) & (zz % lz == 0)
        occ |= rng.random((Z, Y, X)) < 0.0005
    else:
        occ = rng.random((Z, Y, X)) < p["dens"]
    for (x0, y0, z0), s in p.get("pockets", []):
        occ[z0:z0 + s, y0:y0 + s, x0:x0 + s] = False
    occ[0, 0, 0] = True
    return occ


DRIVE = dict(size=(128, 96, 192), voxel=0.05, frames=5, p_occ=0.01, seed=11)


def drive_frames():
    """(pos, q, labels) per update: the hash world, an unobserved slab of x, a pocket the robot drives towards along x"""
    from gie import scenes
    X, Y, Z = DRIVE["size"]
    w = DRIVE["voxel"]
    pocket = (np.array([180, 20, 60]), 56)                   # global voxel corner, side
    for k in range(DRIVE["frames"]):
        pos, q = scenes.pose(k, w, delta_vox=12, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, w, DRIVE["size"])
        lab = scenes.hash_world_labels(pvt, DRIVE["size"], k, seed=DRIVE["seed"], p_occ=DRIVE["p_occ"], toggle_frac=0.25).astype(np.int8)
        lo = np.maximum(pocket[0] - np.array(pvt), 0)
        hi = np.minimum(pocket[0] + pocket[1] - np.array(pvt), np.array([X, Y, Z]))
        if np.all(hi > lo):
            lab[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = 1
        lab[:, :, 8:20 + 3 * k] = 0                          # not observed this update
        yield pos, q, lab


CHILD = r'''
import sys, json
sys.path[:0] = [ROOT, ROOT + "/gie-mapping_amd", HERE]
import numpy as np
import gie, parity
from oracle_py import OracleMapper
import test_edt_fused_stream as T
out, with_oracle = sys.argv[1], sys.argv[2] == "1"
res = {}
for name in T.EDT_CASES:
    sys.stderr.write("case %s\n" % name); sys.stderr.flush()
    occ = T.edt_occupancy(name)
    X, Y, Z = T.EDT_CASES[name]["shape"]
    w = 0.1
    cfg = gie.make_config(w, (X, Y, Z), cutoff_dist=1.0)
    zz, yy, xx = np.nonzero(occ)
    b = gie.Mapper(cfg)
    b.set_pose((0.0, 0.0, 0.0))
    pv = np.array(b.pivot())
    pts = ((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32)
    b.ogm_pointcloud(pts); b.fuse(); b.batch_edt()
    e = b.read_batch_edt()
    b.close()
    res[name + ".dist_sq"] = e["dist_sq"]; res[name + ".coc"] = e["coc"]
sys.stderr.write("case drive\n"); sys.stderr.flush()
cfg = gie.make_config(T.DRIVE["voxel"], T.DRIVE["size"], cutoff_dist=2.0)
a = OracleMapper(cfg) if with_oracle else None
b = gie.Mapper(cfg)
rng = np.random.default_rng(7)
for k, (pos, q, lab) in enumerate(T.drive_frames()):
    for m in ((a, b) if a else (b,)):
        m.update(pos, q, "labels", lab)
    rb = b.read_local()
    for key in ("type", "dist_sq", "coc"):
        res["drive%d.%s" % (k, key)] = rb[key]
    if a:
        ra = a.read_local()
        for key in ("type", "dist_sq", "coc"):
            assert np.array_equal(ra[key], rb[key]), (k, key)
        parity.compare_global("drive update %d" % k, a, b, parity.probe_coords(a.pivot(), T.DRIVE["size"], rng, n=20000, margin=12))
b.close()
if a: a.close()
np.savez(out, **res)
print("ok")
'''


def _run_child(tmp_path, fused, with_oracle):
    import hooks_py
    hooks_py.load()                                   # (builds the test library if need be, outside the child)
    out = str(tmp_path / ("fused%d.npz" % fused))
    code = "ROOT, HERE = %r, %r\n" % (ROOT, HERE) + CHILD
    env = dict(os.environ, GIE_ZS_FUSED=str(fused), GIE_LIB=hooks_py.TEST_SO, GIE_DEBUG_COUNTS="1")
    r = subprocess.run([sys.executable, "-c", code, out, "1" if with_oracle else "0"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out), _stream_counts(r.stderr)


def _stream_counts(err):
    """case -> [(streamed, wide trips, slabs given up)] of every counter read-back (GIE_DEBUG_COUNTS) while it ran"""
    out, case = {}, None
    for line in err.splitlines():
        if line.startswith("case "):
            case = line[5:].strip()
            out[case] = []
        m = re.search(r"pass Z streamed (\d+) \(wide trips (\d+), slabs given up (\d+)\)", line)
        if m and case is not None:
            out[case].append(tuple(int(g) for g in m.groups()))
    return out


def test_fused_stream_form_matches_the_oracle_and_the_unfused_form(oracle_lib, tmp_path):
    from oracle_py import OracleMapper
    new, cn = _run_child(tmp_path, 1, True)           # (the drive is compared with the oracle inside the child, globally too)
    old, co = _run_child(tmp_path, 0, False)
    # the paths this test is about ran, in both forms: every volume streamed, pockets that need the wide trip and pockets
    # that make slabs give up (k_edt_x_redo + the column kernel in the fused form), give-ups in the drive
    for counts in (cn, co):
        assert set(counts) == set(EDT_CASES) | {"drive"}, counts
        for case, seen in counts.items():
            assert seen and all(st == 1 for st, _, _ in seen), (case, seen)
        for case in ("pockets", "odd_x"):
            assert max(w for _, w, _ in counts[case]) > 0, (case, counts[case])
        assert max(f for _, _, f in counts["pockets"]) > 0, counts["pockets"]
        assert max(f for _, _, f in counts["drive"]) > 0, counts["drive"]
    assert sorted(new.files) == sorted(old.files)
    for k in new.files:
        assert np.array_equal(new[k], old[k]), k
    import gie
    for name in EDT_CASES:
        occ = edt_occupancy(name)
        X, Y, Z = EDT_CASES[name]["shape"]
        w = 0.1
        cfg = gie.make_config(w, (X, Y, Z), cutoff_dist=1.0)
        zz, yy, xx = np.nonzero(occ)
        a = OracleMapper(cfg)
        try:
            a.set_pose((0.0, 0.0, 0.0))
            pv = np.array(a.pivot())
            a.ogm_pointcloud(((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32))
            a.fuse(); a.batch_edt()
            e = a.read_batch_edt()
        finally:
            a.close()
        assert np.array_equal(e["dist_sq"], new[name + ".dist_sq"]), name
        assert np.array_equal(e["coc"], new[name + ".coc"]), name


def test_completion_of_a_partial_headline_sized_update(oracle_lib):
    """gie_read_batch_edt after a map update of the headline's size (512^3, the hash world under full observation: partial, since
    the volume is at most 64 tiles high, and taken by the fused form, so pass X did not run): the completion runs pass Z again over
    the whole volume from pass Y's planes.  Against the oracle, and the local map after it."""
    import bench
    import gie
    from gie import scenes
    from oracle_py import OracleMapper
    size = (512, 512, 512)
    cfg = gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False)
    a, b = OracleMapper(cfg), gie.Mapper(cfg)
    try:
        pos, q = bench.c5_pose(scenes, 1, 0.05)
        lab = np.ascontiguousarray(scenes.hash_world_labels(scenes.local_pivot(pos, 0.05, size), size, 1, seed=bench.C5["seed"],
                                                            p_occ=bench.C5["p_occ"], toggle_frac=bench.C5["toggle_frac"]).astype(np.int8))
        for m in (a, b):
            m.update(pos, q, "labels", lab)
        del lab
        ea, eb = a.read_batch_edt(), b.read_batch_edt()
        for key in ("dist_sq", "coc"):
            assert np.array_equal(ea[key], eb[key]), key
        del ea, eb
        ra, rb = a.read_local(), b.read_local()
        for key in ("type", "dist_sq", "coc"):
            assert np.array_equal(ra[key], rb[key]), key
    finally:
        a.close(); b.close()

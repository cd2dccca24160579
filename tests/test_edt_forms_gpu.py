"""Every case of the batch EDT's form table (edt_forms.py) on the device: the kernels the update announces are the ones the host
statement of the launch rules names (GIE_TRACE_LAUNCHES), the streaming form's counters agree with the outcome the case was
built for (GIE_DEBUG_COUNTS), and distances and closest obstacles equal the oracle's bit for bit — and the expectation
test_edt_forms.py has held against the closed form on the CPU.

The library reads its switches once per process, so the cases run in child processes on the test build, one fresh interpreter
per group of cases, each under its own timeout; a child that fails ends its tests without a retry.

Full cases: set_pose, ogm_pointcloud (one point per obstacle voxel), fuse, batch_edt, read_batch_edt — the update is partial
where the volume is at most 64 tiles high, and the read completes it with a second pass Z over the whole volume, so both sets
of launches are checked.  Partial cases: a label feed (label 0 = not observed) decides which tiles are known, the partial result
is exported as it is (GIE_EDT_EXPORT_PARTIAL=1) and compared on exactly the voxels of the tiles with a known voxel, the local
map after the merge everywhere; under GIE_TILE_LIST unset, 0 and 1.

What these tests would catch, by their assertions: a launch rule that sends Y > 512 at X % 4 != 0 to k_edt_y<16,16> fails the
comparison of the announced names with host_forms in y_7x513, y_67x1024 and y_3x1024; a tie in k_edt_y that goes to the smaller
y ('<' for '<=') fails the comparison of coc in every pass Y case with the 'even_pairs' column (the midpoints of its pairs)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import edt_forms as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD_TIMEOUT = 240                                   # seconds per child (a group takes a few)

CHILD = r'''
import sys
sys.path[:0] = [ROOT, ROOT + "/gie-mapping_amd", HERE]
import numpy as np
import gie
import edt_forms as F
out, group = sys.argv[1], sys.argv[2]
res = {}
def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()
for c in F.CASES:
    if c.group != group:
        continue
    w = 0.1
    b = gie.Mapper(gie.make_config(w, c.size, cutoff_dist=1.0))
    b.set_pose((0.0, 0.0, 0.0))
    if c.partial:
        b.ogm_labels(c.labels())
    else:
        zz, yy, xx = np.nonzero(c.occ())
        pv = np.array(b.pivot())
        b.ogm_pointcloud(((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32))
    b.fuse()
    say("case %s update" % c.name)
    b.batch_edt()
    say("case %s completion" % c.name)
    e = b.read_batch_edt()
    say("case %s end" % c.name)
    res[c.name + ".dist_sq"] = e["dist_sq"]; res[c.name + ".coc"] = e["coc"]
    if c.partial:
        b.merge()
        r = b.read_local()
        for key in ("type", "dist_sq", "coc"):
            res[c.name + ".local." + key] = r[key]
    b.close()
np.savez(out, **res)
print("ok")
'''


def _parse(err):
    """case -> dict(update=set of batch EDT kernels announced by gie_batch_edt, completion=... by gie_read_batch_edt,
    counts=(streamed, wide trips, slabs given up) of the last counter read-back)"""
    out, cur, part = {}, None, None
    for line in err.splitlines():
        m = re.match(r"case (\S+) (update|completion|end)$", line)
        if m:
            cur, part = m.group(1), m.group(2)
            out.setdefault(cur, dict(update=set(), completion=set(), counts=None))
            continue
        if cur is None or part == "end":
            continue
        m = re.match(r"\[\d+\] launch (.+)$", line)
        if m:
            name = m.group(1).strip("()").replace(" ", "")
            if name.startswith("k_edt_") and name != "k_edt_prep":
                out[cur][part].add(name)
        m = re.search(r"pass Z streamed (\d+) \(wide trips (\d+), slabs given up (\d+)\)", line)
        if m:
            out[cur]["counts"] = tuple(int(g) for g in m.groups())
    return out


_runs = {}


def _run_group(tmp_path_factory, group, mode=None):
    """one child per (group, GIE_TILE_LIST mode), run once; its failure is kept and raised for every test of the group"""
    key = (group, mode)
    if key not in _runs and _runs.get("abnormal"):
        # a child was killed by a signal or ran into its timeout: nothing more is started on the device
        raise RuntimeError("not started: " + str(_runs["abnormal"]))
    if key not in _runs:
        import hooks_py
        hooks_py.load()                               # (builds the test library if need be, outside the child)
        out = str(tmp_path_factory.mktemp("edt_forms") / ("%s_%s.npz" % (group, mode)))
        env = dict(os.environ, GIE_LIB=hooks_py.TEST_SO, GIE_TRACE_LAUNCHES="1", GIE_DEBUG_COUNTS="1")
        env.pop("GIE_TILE_LIST", None)
        if group == "p":
            env["GIE_EDT_EXPORT_PARTIAL"] = "1"
            if mode is not None:
                env["GIE_TILE_LIST"] = str(mode)
        code = "ROOT, HERE = %r, %r\n" % (ROOT, HERE) + CHILD
        try:
            r = subprocess.run([sys.executable, "-c", code, out, group], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            if r.returncode != 0 or "ok" not in r.stdout:
                _runs[key] = RuntimeError("child of group %r ended with %s\n%s\n%s" % (group, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
                if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:
                    _runs["abnormal"] = "the child of group %r ended with %s" % (group, r.returncode)
            else:
                _runs[key] = (np.load(out), _parse(r.stderr))
        except subprocess.TimeoutExpired as e:
            _runs[key] = RuntimeError("child of group %r timed out: %s" % (group, e))
            _runs["abnormal"] = "the child of group %r timed out" % (group,)
    if isinstance(_runs[key], Exception):
        raise _runs[key]
    return _runs[key]


_oracle = {}


def _oracle_run(c):
    """the oracle through the same calls (computed once per case, read only)"""
    if c.name not in _oracle:
        import gie
        from oracle_py import OracleMapper
        w = 0.1
        a = OracleMapper(gie.make_config(w, c.size, cutoff_dist=1.0))
        try:
            a.set_pose((0.0, 0.0, 0.0))
            if c.partial:
                a.ogm_labels(c.labels())
            else:
                zz, yy, xx = np.nonzero(c.occ())
                pv = np.array(a.pivot())
                a.ogm_pointcloud(((np.stack([xx, yy, zz], -1) + pv) * np.float32(w)).astype(np.float32))
            a.fuse(); a.batch_edt()
            e = a.read_batch_edt()
            ty = a.read_local(edt=False, dist_sq=False, coc=False)["type"]
            loc = None
            if c.partial:
                a.merge()
                loc = a.read_local()
        finally:
            a.close()
        _oracle[c.name] = (e, ty, loc)
    return _oracle[c.name]


def _planes_and_known(c, ty):
    Z = c.size[2]
    return int((ty == 2).reshape(Z, -1).any(axis=1).sum()), int(F.need_of_labels(ty).sum())


FULL = [c.name for c in F.CASES if not c.partial]
PARTIAL = [c.name for c in F.CASES if c.partial]


@pytest.mark.parametrize("name", FULL)
def test_full_case(oracle_lib, tmp_path_factory, name):
    c = F.case(name)
    got, trace = _run_group(tmp_path_factory, c.group)
    e, ty, _ = _oracle_run(c)
    occ = c.occ()
    assert np.array_equal(ty == 2, occ)               # the point cloud made exactly the case's obstacles
    K, known = _planes_and_known(c, ty)
    partial = F.update_is_partial(c.size)
    t = trace[name]
    # (a) the launches of the update and of the completion
    assert t["update"] == F.host_forms(c.size, K, known, 0 if partial else 1), (t["update"], "update")
    assert t["completion"] == (F.host_forms(c.size, K, known, 1, completion=True) if partial else set()), (t["completion"], "completion")
    # (b) the streaming form's counters after the pass over the whole volume
    assert t["counts"] is not None
    streamed, wide, given_up = t["counts"]
    print(name, "launches", sorted(t["update"]), sorted(t["completion"]), "streamed / wide trips / slabs given up", t["counts"])
    if F.z_worker(c.size, K, known, 1) == "stream":
        so = F.stream_outcome(occ)
        assert streamed == 1
        assert (given_up > 0) == bool(so["given_up"]), (t["counts"], len(so["given_up"]))
        assert (wide > 0) == bool(so["wide"]), (t["counts"], so["wide"])
    else:
        assert (streamed, wide, given_up) == (0, 0, 0), t["counts"]
    # (c) the result: the oracle's through the same calls, and the expectation held against the closed form on the CPU
    xd, xc = F.expected(name)
    for key, want in (("dist_sq", xd), ("coc", xc)):
        assert np.array_equal(got[name + "." + key], e[key]), key
        assert np.array_equal(got[name + "." + key], want), key + " (expectation)"


@pytest.mark.parametrize("mode", F.PARTIAL_MODES, ids=lambda m: "tile_list_%s" % ("unset" if m is None else m))
@pytest.mark.parametrize("name", PARTIAL)
def test_partial_case(oracle_lib, tmp_path_factory, name, mode):
    c = F.case(name)
    got, trace = _run_group(tmp_path_factory, "p", mode)
    e, ty, loc = _oracle_run(c)
    lab = c.labels()
    assert np.array_equal(ty, lab)                    # a fresh map: the types are the labels
    K, known = _planes_and_known(c, ty)
    X, Y, Z = c.size
    assert F.update_is_partial(c.size)
    t = trace[name]
    assert t["update"] == F.host_forms(c.size, K, known, 0), t["update"]
    assert t["completion"] == set(), t["completion"]  # exported as it is
    worker = F.z_worker(c.size, K, known, 0, mode)
    assert t["counts"] is not None
    streamed, wide, given_up = t["counts"]
    print(name, mode, worker, "streamed / wide trips / slabs given up", t["counts"])
    assert streamed == (1 if worker == "stream" else 0), (worker, t["counts"])
    if worker == "stream":
        so = F.stream_outcome(c.occ())
        assert (given_up > 0) == bool(so["given_up"]) and (wide > 0) == bool(so["wide"]), (t["counts"], so["wide"], len(so["given_up"]))
    else:
        assert (wide, given_up) == (0, 0), t["counts"]
    # exactly the voxels of the tiles that hold a known voxel
    need = F.need_of_labels(lab)
    vox = np.repeat(np.repeat(np.repeat(need, 8, 0), 8, 1), 8, 2)[:Z, :Y, :X]
    assert vox.any() and not vox.all()
    xd, xc = F.expected(name)
    for key, want in (("dist_sq", xd), ("coc", xc)):
        assert np.array_equal(got[name + "." + key][vox], e[key][vox]), key
        assert np.array_equal(got[name + "." + key][vox], want[vox]), key + " (expectation)"
    for key in ("type", "dist_sq", "coc"):
        assert np.array_equal(got[name + ".local." + key], loc[key]), "local " + key

"""The segmented ray caster (k_free_rays) on the hand-made clouds of tests/ray_cases.py.

Three statements of freeLocObs walk every ray sequentially: the oracle, the emulation's gie_free_ray and the plain float32
statement of tests/raycast_ref.py.  The kernel does not: it cuts the walk into 8 time intervals, replays the walk's state per
axis, clips the walk to the ray's stay in the volume, finds the stop as a minimum over the segments and merges the decrements of
neighbouring lanes.  Without a GPU this module holds the three sequential statements against one another and asserts every
case's precondition (require) on the plain statement; on the GPU it holds gie.Mapper against the oracle, stage by stage and as
the production sequence (set_pose, ogm_pointcloud, step: then only the tile and block marks of gie_ray_touch / gie_ray_touch_k
tell gie_fuse where to look), over three updates with the pose moved 3 voxels each time, and against the plain statement
directly on the exact cases.  Counts and labels are integers: nothing is compared with a tolerance, nothing is left out.

The plain statement is given the stated subset of a case's cloud (ray_cases: every k-th ray of each group and all the special
ones: 600 rays, at most 640), on the first update; the oracle, the emulation and the HIP library get the whole cloud, and the subset as
a cloud of its own where the statement is compared."""
import functools
import types

import numpy as np
import pytest

import gie
import parity
import ray_cases
from emu_py import EmuMapper
from oracle_py import OracleMapper
from raycast_ref import _F, _pos2coord, _raycast_second_statement

NAMES = [c["name"] for c in ray_cases.CASES]
EXACT = [c["name"] for c in ray_cases.CASES if c["exact"]]
MARGIN = 10                                         # query_global is compared over the volume +- this many voxels


def _mapper(make, case):
    cfg = gie.make_config(case["voxel"], case["size"], cutoff_dist=1.0, ogm_min_h=case["min_h"], ogm_max_h=case["max_h"])
    m = make(cfg)
    if case["tile"]:
        m.set_tile(*case["tile"])
    return m


@functools.lru_cache(maxsize=None)
def _statement(name):
    """(count, labels, stats) of the plain statement for the subset of a case's cloud, first update; computed once per case."""
    case = ray_cases.BY_NAME[name]
    pos = ray_cases.poses(case)[0]
    pvt = ray_cases.pivot(case, pos)
    w = _F(case["voxel"])
    records = []
    count, lab = _raycast_second_statement(np.array(pos, np.float32), case["points"][case["subset"]], pvt, case["size"], w,
                                           _F(case["min_h"]), _F(case["max_h"]), records)
    sensor = [a - b for a, b in zip(_pos2coord([_F(v) for v in pos], w), pvt)]
    for a in (count, lab):
        a.setflags(write=False)
    return count, lab, dict(rays=records, count=count, sensor=sensor)


def _against_statement(make, name):
    case = ray_cases.BY_NAME[name]
    count, lab, _ = _statement(name)
    m = _mapper(make, case)
    try:
        pos = ray_cases.poses(case)[0]
        m.set_pose(pos, case["quat"])
        assert list(m.pivot()) == ray_cases.pivot(case, pos)
        m.ogm_pointcloud(case["points"][case["subset"]])
        got = m.read_ogm()
        bad = np.argwhere(got["ray_count"] != count)
        assert len(bad) == 0, "%s: %d cells differ in their ray count, first (z, y, x) %s: %d, statement %d" % (
            name, len(bad), tuple(bad[0]), got["ray_count"][tuple(bad[0])], count[tuple(bad[0])])
        assert np.array_equal(got["inst_type"], lab), "%s: labels differ" % name
    finally:
        m.close()


def _volume_probes(pvt, size):
    g = np.meshgrid(*[np.arange(pvt[i] - MARGIN, pvt[i] + size[i] + MARGIN) for i in range(3)], indexing="ij")
    return np.stack([v.ravel() for v in g], -1).astype(np.int32)


def _against_oracle(make, name, production):
    """A case's whole cloud through the oracle and a mapper under test, ray_cases.UPDATES updates."""
    case = ray_cases.BY_NAME[name]
    sc = types.SimpleNamespace(name=name, size=case["size"], probe_margin=MARGIN)
    rng = np.random.default_rng(5)
    a, b = _mapper(OracleMapper, case), _mapper(make, case)
    try:
        for k, pos in enumerate(ray_cases.poses(case)):
            tag = "%s update %d%s" % (name, k, " (production)" if production else "")
            for m in (a, b):
                m.set_pose(pos, case["quat"])
                m.ogm_pointcloud(case["points"])
            assert a.pivot() == b.pivot(), tag
            if production:
                a.step(); b.step()
                parity._compare_after_merge(sc, k, a, b, rng, True)
                continue
            oa, ob = a.read_ogm(), b.read_ogm()
            for key in ("ray_count", "inst_type"):
                bad = np.argwhere(oa[key] != ob[key])
                assert len(bad) == 0, "%s: %s differs in %d cells, first (z, y, x) %s: %d, oracle %d" % (
                    tag, key, len(bad), tuple(bad[0]), ob[key][tuple(bad[0])], oa[key][tuple(bad[0])])
            a.fuse(); b.fuse()
            ta, tb = a.read_local(edt=False, dist_sq=False, coc=False)["type"], b.read_local(edt=False, dist_sq=False, coc=False)["type"]
            assert np.array_equal(ta, tb), "%s: fused types differ in %d voxels" % (tag, int((ta != tb).sum()))
            xyz = _volume_probes(a.pivot(), case["size"])
            ga, gb = a.query_global(xyz), b.query_global(xyz)
            for key in ("occ_val", "vox_type"):
                assert np.array_equal(ga[key], gb[key]), "%s: global %s differs in %d voxels after the fusion" % (tag, key, int((ga[key] != gb[key]).sum()))
            a.batch_edt(); b.batch_edt()
            a.merge(); b.merge()
            parity._compare_after_merge(sc, k, a, b, rng, True)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", NAMES)
def test_case_precondition_holds_on_the_statement(name):
    """What a case is there for (ties, a stop in every eighth, rays that enter late, never, or leave early ...) is a fact about the
    plain statement's walk of its rays, not about any mapper."""
    case = ray_cases.BY_NAME[name]
    assert len(case["subset"]) <= 640
    if not case["exact"]:
        # far from the origin, tilted: the statement's ties do not hold there.  Such a case is the cloud of an exact case (its twin:
        # the same points in the map frame, the same tile), shifted or rotated, and the twin's walk states its precondition
        twin = ray_cases.BY_NAME[case["twin"]]
        assert twin["exact"] and twin["size"] == case["size"] and twin["tile"] == case["tile"] and len(twin["points"]) == len(case["points"])
        assert np.array_equal(twin["subset"], case["subset"])
        if case["quat"] == ray_cases.IDENT:
            assert np.array_equal(twin["points"], case["points"])
        else:                                         # rotated into the sensor frame: back in the map frame it is the twin's cloud
            back = case["points"].astype(np.float64) @ ray_cases.rot_from_quat(case["quat"]).T
            assert np.allclose(back, twin["points"], rtol=0.0, atol=1e-4 * max(1.0, float(np.abs(twin["points"]).max())))
        case = twin
    _, _, stats = _statement(case["name"])
    assert case["require"](stats), name


def test_families_are_all_there():
    fam = {c["family"] for c in ray_cases.CASES}
    assert fam == {"axis", "ties", "stops", "ends", "aggregation", "outside", "far", "tilted"}
    sizes = sorted({len(c["points"]) for c in ray_cases.CASES if c["family"] == "aggregation"})
    assert sizes[:4] == [1, 63, 64, 65] and sizes[4] % 64 == 1
    assert sum(r["ties"] for r in _statement("ties")[2]["rays"]) >= 100


@pytest.mark.parametrize("name", EXACT)
def test_oracle_equals_the_statement(oracle_lib, name):
    _against_statement(OracleMapper, name)


@pytest.mark.parametrize("name", EXACT)
def test_emulation_equals_the_statement(oracle_lib, name):
    _against_statement(EmuMapper, name)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_the_oracle(oracle_lib, name):
    _against_oracle(EmuMapper, name, production=False)


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_equals_the_oracle_stage_by_stage(oracle_lib, name):
    _against_oracle(gie.Mapper, name, production=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_equals_the_oracle_in_the_production_sequence(oracle_lib, name):
    _against_oracle(gie.Mapper, name, production=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXACT)
def test_hip_equals_the_statement(name):
    _against_statement(gie.Mapper, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aggregation", "outside_-x"])
def test_device_cloud_equals_host_cloud(name):
    """gie_ogm_pointcloud_dev on a torch tensor, enqueued on the mapper's stream, against the host form: byte for byte."""
    import torch
    case = ray_cases.BY_NAME[name]
    host, devm = _mapper(gie.Mapper, case), _mapper(gie.Mapper, case)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(devm.stream_handle(), device=dev)
        for k, pos in enumerate(ray_cases.poses(case)):
            host.set_pose(pos, case["quat"]); devm.set_pose(pos, case["quat"])
            host.ogm_pointcloud(case["points"])
            with torch.cuda.stream(st):
                d = torch.from_numpy(case["points"]).to(dev)
                devm.ogm_pointcloud_dev(d.data_ptr(), len(case["points"]))
            oh, od = host.read_ogm(), devm.read_ogm()
            for key in ("ray_count", "inst_type"):
                assert oh[key].tobytes() == od[key].tobytes(), (name, k, key)
            host.step(); devm.step()
            rh, rd = host.read_local(), devm.read_local()
            for key in ("type", "dist_sq", "coc", "edt"):
                assert rh[key].tobytes() == rd[key].tobytes(), (name, k, key)
            del d
    finally:
        host.close(); devm.close()

"""The projective classifiers (gie_classify_depth / _multiscan / _scan2d under k_voxz) with a sensor whose z axis is not the map's:
the case table of tests/sensor_edges.py (roll and pitch up to upside down and on its side; lidars with a negative increment, a
one-sided field of view, wrapping bins, one ring, +-88 degrees; cameras with fx != fy and a principal point outside the image;
volumes across every edge of the z-column kernel) through the emulation (CPU) and the HIP library (GPU), against the oracle bit for
bit and against the float64 statements of tests/ogm_f64.py; the device-resident sensor entry points against the host forms; a
production sequence (set_pose / ogm_* / step only) of tilted updates against the oracle.

What the tilts pin is op_classify_multiscan's pair of early-outs (gie_functors.h): checked by hand against two mutations, see
DESIGN.md section 2."""
import numpy as np
import pytest

import gie
import parity
import sensor_edges as se
from emu_py import EmuMapper
from oracle_py import OracleMapper

SETS = [(s, n) for s in ("multiscan", "depth", "scan2d") for n in se.SETS[s]]
IDS = ["%s-%s" % sn for sn in SETS]


def _run_set(make_test, sensor, name):
    for case in se.cases(sensor, name):                     # the main volume with every tilt, the small ones with the strongest
        se.run(OracleMapper, make_test, sensor, case)


def _production(make_test):
    """Eight tilted lidar updates (set a), then eight tilted depth updates of the same drive, 4 voxels per update, driven as a node
    drives them; after every update the local volume, the global probes and the wave statistics against the oracle."""
    lidar = dict(se.cases("multiscan", "a")[0])
    depth = dict(se.cases("depth", "60x80")[0], voxel=lidar["voxel"], world="multiscan", k0=len(lidar["tilts"]))
    sc = parity.Scenario("tilted_production", lidar["size"], voxel=lidar["voxel"])
    cfg = se.config(lidar)
    a, b = OracleMapper(cfg), make_test(cfg)
    rng = np.random.default_rng(5)
    try:
        k = 0
        for case in (lidar, depth):
            for pos, q, data, kw, _ in se.frames(case):
                for m in (a, b):
                    m.set_pose(pos, q)
                    se.feed(m, case["sensor"], data, kw)
                    m.step()
                assert a.pivot() == b.pivot()
                parity._compare_after_merge(sc, k, a, b, rng, True)
                k += 1
            types = a.read_local(edt=False, dist_sq=False, coc=False)["type"]
            assert (types == 1).sum() > 1000 and (types == 2).sum() > 50      # the map holds free space and obstacles
        assert k == 16
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ CPU: the emulation (it shares the functors with the kernels)

@pytest.mark.parametrize("sensor,name", SETS, ids=IDS)
def test_tilted_sensor_emulation(oracle_lib, sensor, name):
    _run_set(EmuMapper, sensor, name)


def test_tilted_multiscan_for_motion_planner_emulation(oracle_lib):
    se.run(OracleMapper, EmuMapper, "multiscan", se.planner_case())


def test_tilted_production_sequence_emulation(oracle_lib):
    _production(EmuMapper)


# ------------------------------------------------------------------ GPU: the HIP library

@pytest.mark.gpu
@pytest.mark.parametrize("sensor,name", SETS, ids=IDS)
def test_tilted_sensor_hip(oracle_lib, sensor, name):
    _run_set(gie.Mapper, sensor, name)


@pytest.mark.gpu
def test_tilted_multiscan_for_motion_planner_hip(oracle_lib):
    se.run(OracleMapper, gie.Mapper, "multiscan", se.planner_case())


@pytest.mark.gpu
def test_tilted_production_sequence_hip(oracle_lib):
    _production(gie.Mapper)


@pytest.mark.gpu
@pytest.mark.parametrize("sensor,name", [("depth", "37x53"), ("multiscan", "a")], ids=["depth", "multiscan"])
def test_device_forms_equal_the_host_forms_under_tilt(sensor, name):
    """gie_ogm_depth_dev / gie_ogm_multiscan_dev on torch tensors on the mapper's stream against a second mapper fed the host
    forms: scan labels, ray counts and everything read_local returns after the merge, byte for byte, for two tilted updates.
    (Set a: its field of view spans the horizon, so tile_skip is at work in the device form too.)"""
    import torch
    case = dict(se.cases(sensor, name)[0], tilts=((-1.2, 0.9), (1.5, 0.0)))
    cfg = se.config(case)
    h, d = gie.Mapper(cfg), gie.Mapper(cfg)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(d.stream_handle(), device=dev)
        for pos, q, data, kw, _ in se.frames(case):
            h.set_pose(pos, q)
            se.feed(h, sensor, data, kw)
            d.set_pose(pos, q)
            with torch.cuda.stream(st):
                t = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev)
                if sensor == "depth":
                    d.ogm_depth_dev(t.data_ptr(), data.shape[0], data.shape[1], **kw)
                else:
                    d.ogm_multiscan_dev(t.data_ptr(), data.shape[1], data.shape[0], **kw)
            oh, od = h.read_ogm(), d.read_ogm()             # (synchronises: the tensor t has been read by the time it is replaced)
            assert (oh["inst_type"] == 1).sum() > 1000 and (oh["inst_type"] == 2).sum() > 10
            for key in ("inst_type", "ray_count"):
                assert oh[key].tobytes() == od[key].tobytes(), key
            for m in (h, d):
                m.fuse(); m.batch_edt(); m.merge()
            rh, rd = h.read_local(), d.read_local()
            for key in ("type", "dist_sq", "coc", "edt"):
                assert rh[key].tobytes() == rd[key].tobytes(), key
    finally:
        h.close(); d.close()

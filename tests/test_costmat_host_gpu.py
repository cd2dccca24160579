"""VolumetricMapper::exploration_costs (host/gie_host.hpp): the chain frontier clusters -> goals behind the robot's position ->
cost matrix, all on the mapper's stream with one copy back, against the same three steps through the Python mapper."""
import os
import subprocess

import numpy as np
import pytest

import gie
from gie import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_layer_exploration_costs_match_the_mapper(tmp_path):
    import __graft_entry__ as ge
    ge.build_hip()
    exe = str(tmp_path / "costmat_host_probe")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DGIE_HOST_WITH_HIP", "-I" + os.path.join(rocm, "include"),
                           "-Wno-unused-result", os.path.join(ROOT, "tests", "gpu_helpers", "costmat_host_probe.cpp"), "-o", exe,
                           "-L" + ge.CSRC, "-lgie_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + ge.CSRC, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    size, w, cutoff, cap, clearance, min_size = (48, 40, 33), 0.1, 3.0, 20, 0.1, 3
    world = scenes.BoxWorld(4, extent=(2.5, 2.5, 1.0), n_boxes=30)
    frames, words = [], [np.float32(4)]
    for k in range(4):
        pos, q = scenes.pose(k, w, delta_vox=3, yaw_deg=5.0)
        pts, _ = scenes.lidar_frame(world, k, pos, q, az=360, max_range=6.0)
        frames.append((pos, q, pts))
        words += [np.array(list(pos) + list(q) + [len(pts)], np.float32), pts.ravel()]
    fpath = str(tmp_path / "frames.f32")
    np.concatenate([np.atleast_1d(x) for x in words]).astype(np.float32).tofile(fpath)
    m = gie.Mapper(gie.make_config(w, size, fast_mode=False, cutoff_dist=cutoff))
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.fuse(); m.batch_edt(); m.merge()
        kept, _ = m.frontier_compute(clearance, min_size, 26, cap)
        _, goals, _ = m.read_frontier_clusters()
        points = np.concatenate([np.array([frames[-1][0]], np.float32), goals]).astype(np.float32)
        cost, valid = m.costmat(points, clearance)
    finally:
        m.close()
    nan = np.isnan(points).any(axis=1)
    assert 1 <= kept and (~nan[1:]).sum() == min(kept, cap) and np.array_equal(valid[1:], ~nan[1:])
    out = str(tmp_path / "on")
    res = subprocess.run([exe, fpath, out, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), str(cap), repr(clearance), str(min_size)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "frames 4 kept %d points %d" % (kept, cap + 1) in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".goals", np.uint8).tobytes() == points.tobytes()
    assert np.fromfile(out + ".cost", np.int32).tobytes() == cost.tobytes()
    if valid[0]:
        assert (cost[0, 1:][valid[1:]] >= 0).any()

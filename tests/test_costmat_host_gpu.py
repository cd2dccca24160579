"""VolumetricMapper::exploration_costs (host/gie_host.hpp): the chain frontier clusters -> goals behind the robot's position ->
cost matrix, all on the mapper's stream with one copy back, against the same three steps through the Python mapper."""
import os
import subprocess

import numpy as np
import pytest

import gie
from stage_common import build_host_probe, lidar_frames

pytestmark = pytest.mark.gpu


def test_host_layer_exploration_costs_match_the_mapper(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = build_host_probe(tmp_path, "costmat_host_probe", ["-DGIE_HOST_WITH_HIP", "-I" + os.path.join(rocm, "include"), "-Wno-unused-result",
                                                            "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    size, w, cutoff, cap, clearance, min_size = (48, 40, 33), 0.1, 3.0, 20, 0.1, 3
    frames, fpath = lidar_frames(tmp_path)
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

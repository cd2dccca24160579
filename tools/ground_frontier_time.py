#!/usr/bin/env python3
"""What the ground frontier clusters cost on an MI355X, beside the host route they replace.

  python tools/ground_frontier_time.py [--out profiles/r22_ground_frontier_times.txt] [--cases ugv,c5,rooms,specks]

Four cases (include/gie.h "ground frontier clusters"):
  ugv     the reference's UGV configuration, 200 x 200 x 24 at 0.05 m (tools/ground_nf1_time.py's room of boxes), clearance_sq 4;
  c5      the headline workload as bench.py builds it (the hash world at 512^3; bench.py itself is not touched), the ground field of a
          band of 24 layers, clearance_sq 0;
  rooms   512 x 512 x 2, ONE component of a quarter of a million cells and a few hundred of nine cells
          (tests/test_ground_frontier_gpu.py's large-component field);
  specks  512 x 512 x 3, the band on the middle layer: a never-seen cell every four cells, 16 000 four-cell rings.
Per case, through the _dev forms, connectivity 8, min_size 1, max_clusters 1024: device time of a compute and of each reader from the
"ground_frontier" entry of gie_profile_read, median of five rounds of 20 calls.  That entry brackets the section's own launches;
rocPRIM's scan inside a compute is not among them, so the compute is also timed on the wall clock: 200 _dev calls back to back and
one sync.  The gather of the ground navigation function at the goal array is read from "ground_nf1".  The host route —
gie_read_ground, then scipy.ndimage.label and find_objects on the member plane — is timed on the wall clock in the same session,
and so is the whole numpy / scipy statement of tests/ground_frontier_ref.py, which also makes the records."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

CAP = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="ugv,c5,rooms,specks")
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    import bench
    import gie
    import ground_frontier_ref as F
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def measure(tag, m, size, csq):
        pvt = m.pivot()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            g = m.read_ground()
            t1 = time.perf_counter()
            lab, k = ndimage.label(F.members(g, csq), structure=F.structure(8))
            ndimage.find_objects(lab)
            t2 = time.perf_counter()
            ref = F.clusters(g, csq, 8, 1, CAP, pvt, m.cfg.voxel_width)
            ts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        rd, lb, full = (np.median([t[i] for t in ts]) * 1e3 for i in range(3))
        big = int(ref["sizes"].max()) if len(ref["sizes"]) else 0
        say(f"{tag}: host route  gie_read_ground {rd:.2f} ms + label and find_objects {lb:.2f} ms (the whole statement with its records {full:.1f} ms); "
            f"{ref['n_members']} members, {ref['n_clusters']} components, the largest {big} cells")
        n = size[0] * size[1]
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            d_rec = torch.empty(64 * CAP, dtype=torch.uint8, device=dev)
            d_goal = torch.empty(2 * CAP, dtype=torch.float32, device=dev)
            d_cnt = torch.empty(4, dtype=torch.int32, device=dev)
            d_lab = torch.empty(n, dtype=torch.int32, device=dev)
            d_steps = torch.empty(CAP, dtype=torch.int32, device=dev)
            d_robot = torch.from_numpy(ref["goals"][:1].copy() if ref["n_clusters"] else np.zeros((1, 2), np.float32)).to(dev)
        calls = {"compute": ("ground_frontier", lambda: m.ground_frontier_compute_dev(csq, 1, 8, CAP, d_cnt.data_ptr())),
                 "clusters": ("ground_frontier", lambda: m.read_ground_frontier_clusters_dev(d_rec.data_ptr(), d_goal.data_ptr(), d_cnt.data_ptr() + 8)),
                 "labels": ("ground_frontier", lambda: m.read_ground_frontier_labels_dev(d_lab.data_ptr())),
                 "gather": ("ground_nf1", lambda: m.ground_nf1_query_dev(d_goal.data_ptr(), CAP, d_steps.data_ptr()))}
        us = {}
        for name in ("compute", "clusters", "labels", "gather"):
            entry, run = calls[name]
            if name == "gather":
                m.ground_nf1_compute_dev(d_robot.data_ptr(), 1, csq)
            run()
            m.sync()
            med = []
            m.profile_enable(True)
            for _ in range(5):
                m.profile_read()
                for _ in range(20):
                    run()
                tot, k = m.profile_read()[entry]
                assert k == 20
                med.append(tot / k * 1e3)
            m.profile_enable(False)
            us[name] = float(np.median(med))
        wall = []
        for _ in range(3):
            m.sync()
            t0 = time.perf_counter()
            for _ in range(200):
                calls["compute"][1]()
            m.sync()
            wall.append((time.perf_counter() - t0) / 200 * 1e6)
        m.sync()
        have = min(ref["n_clusters"], CAP)
        assert d_cnt.cpu().tolist()[:3] == [ref["n_clusters"], ref["n_cells"], ref["n_clusters"]]
        assert np.array_equal(d_lab.cpu().numpy().reshape(size[1], size[0]), ref["labels"])
        assert d_rec.cpu().numpy()[:64 * have].tobytes() == ref["records"].tobytes()
        say(f"{tag}: device      compute {us['compute']:.1f} us in its own launches, {np.median(wall):.1f} us a call back to back with the scan (wall clock); "
            f"clusters {us['clusters']:.1f} us, labels {us['labels']:.1f} us, gather at {CAP} goals {us['gather']:.1f} us")
        say(f"{tag}: device route (compute + clusters, wall clock) {np.median(wall) + us['clusters']:.1f} us = 1 / {(rd + lb) * 1e3 / (np.median(wall) + us['clusters']):.0f} of the host route")

    def labelled(size, lab, band=None, w=0.1, cutoff=2.0):
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=cutoff, fast_mode=False))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(np.repeat(lab[None], size[2], axis=0))
            m.step()
        z = m.pivot()[2]
        lo, hi = band if band is not None else (0, size[2] - 1)
        m.ground_compute(z + lo, z + hi)
        return m

    if "ugv" in a.cases:
        size = (200, 200, 24)
        rng = np.random.default_rng(18)
        lab = np.ones((size[2], size[1], size[0]), np.int8)
        lab[0] = 2
        for _ in range(40):
            x, y, sx, sy, h = rng.integers(0, 190), rng.integers(0, 190), rng.integers(2, 12), rng.integers(2, 12), rng.integers(2, 24)
            lab[:h, y:y + sy, x:x + sx] = 2
        lab[:, :, :6] = 0
        m = gie.Mapper(gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        z = m.pivot()[2]
        m.ground_compute(z + 1, z + 23)                        # the body's band: the floor lies below it
        measure("ugv 200x200", m, size, 4)
        m.close()
    if "c5" in a.cases:
        pre = bench.PRESETS["c5"]
        size, w, total = pre["size"], pre["voxel"], 8
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=pre["cutoff"], fast_mode=pre["fast"], max_blocks=bench.pool_blocks("c5", size, total),
                                       wave_workgroups=bench.WAVE_GRID["wgs"], place_tries=bench.PLACE_TRIES))
        feed = bench.HashWorldFeed(torch, scenes, dev, w, size, (0, 0, 0))
        feed.prepare(0, total)
        for i in range(total):
            feed.step_input(m, i)
            m.step()
        m.sync()
        z = m.pivot()[2]
        m.ground_compute(z + 244, z + 267)
        measure("c5 512x512", m, size, 0)
        m.close()
    if "rooms" in a.cases:
        size = (512, 512, 2)
        lab = np.ones((size[1], size[0]), np.int8)
        lab[0] = lab[-1] = 2
        lab[:, 0] = lab[:, -1] = 2
        for y in range(8, size[1] - 8, 24):
            for x in range(8, size[0] - 8, 24):
                lab[y:y + 5, x:x + 5] = 2
                lab[y + 1:y + 4, x + 1:x + 4] = 1
        m = labelled(size, lab)
        measure("rooms 512x512", m, size, 0)
        m.close()
    if "specks" in a.cases:
        size = (512, 512, 3)
        lab = np.ones((size[1], size[0]), np.int8)
        lab[0] = lab[-1] = 2
        lab[:, 0] = lab[:, -1] = 2
        lab[2:size[1] - 2:4, 2:size[0] - 2:4] = 0
        lab[16:size[1] - 8:32, 16:size[0] - 8:32] = 2           # (an obstacle inside every cell's cut-off)
        m = labelled(size, lab, (1, 1))
        measure("specks 512x512", m, size, 0)
        m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ground_frontier_time.py   (MI355X; gie_profile_read and the wall clock for the device, wall clock for the host route)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

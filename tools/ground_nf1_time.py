#!/usr/bin/env python3
"""What the ground navigation function costs on an MI355X, beside the host route it replaces.

  python tools/ground_nf1_time.py [--out profiles/r20_ground_nf1_times.txt] [--host-route] [--cases ugv,c5,maze,glb]

Four cases (include/gie.h "ground navigation function"):
  ugv   the reference's UGV configuration, 200 x 200 x 24 at 0.05 m (tools/ground_time.py's room of boxes), one goal, clearance_sq 4;
  c5    the headline workload as bench.py builds it (the hash world at 512^3; bench.py itself is not touched), the ground field of a
        band of 24 layers, one goal on the cell nearest the centre in the largest traversable region, clearance_sq 0 (at 9 the
        largest region of that cluttered band has 31 cells);
  maze  512 x 512 x 1, ONE serpentine corridor of one cell (rows two apart): about 130 000 BFS levels, one cell each;
  glb   512 x 769 x 1 — one row beyond the LDS budget: the propagation on planes in global memory — a corridor with rows 16 apart.
Per case, through the _dev forms: device time of a compute (the bit planes, the goals, the propagation) from the "ground_nf1" entry
of gie_profile_read, median of five rounds of 20 calls; the same for a compute WITHOUT a source (the bit planes and a propagation
that finds nothing: what a compute costs before its first level); one path and the CostMap.  The number of levels is the field's
largest value.  The host route — gie_read_ground, then the level-synchronous BFS of tests/ground_nf1_ref.py in numpy and a queue BFS
in plain Python — is timed on the wall clock; --host-route measures only that."""
import argparse
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def queue_bfs(trav, src):
    Y, X = trav.shape
    nf = np.full(Y * X, -1, np.int32)
    ok = trav.ravel().tolist()
    q = collections.deque(np.flatnonzero(src.ravel()).tolist())
    val = nf.tolist()
    for i in q:
        val[i] = 0
    while q:
        i = q.popleft()
        x, v = i % X, val[i] + 1
        for j, inside in ((i - 1, x > 0), (i + 1, x < X - 1), (i - X, i >= X), (i + X, i < (Y - 1) * X)):
            if inside and ok[j] and val[j] < 0:
                val[j] = v
                q.append(j)
    return np.array(val, np.int32).reshape(Y, X)


def serpentine(X, Y, pitch):
    lab = np.full((Y, X), 2, np.int8)
    rows = list(range(1, Y - 1, pitch))
    first = None
    for i, y in enumerate(rows):
        lab[y, 1:X - 1] = 1
        if i + 1 < len(rows):
            lab[y:rows[i + 1], X - 2 if i % 2 == 0 else 1] = 1
        first = first or (1, y)
    return lab, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-route", action="store_true", help="only the host route (any build of the library that has the ground costmap)")
    ap.add_argument("--cases", default="ugv,c5,maze,glb")
    a = ap.parse_args()
    import torch
    import bench
    import gie
    import ground_nf1_ref as N
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def measure(tag, m, size, goal_cell, csq, host_rounds):
        pvt = m.pivot()
        w = np.float32(m.cfg.voxel_width)
        goal = ((np.array([goal_cell], np.float64) + np.array(pvt[:2])).astype(np.float32) * w).astype(np.float32)
        ts = []
        for _ in range(host_rounds):
            t0 = time.perf_counter()
            g = m.read_ground()
            t1 = time.perf_counter()
            trav = N.traversable(g, csq)
            src = N.sources(g, trav, goal, pvt, m.cfg.voxel_width)
            ref = N.propagate(trav, src)
            t2 = time.perf_counter()
            ref_q = queue_bfs(trav, src)
            ts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        rd, npy, pyq = (np.median([t[k] for t in ts]) * 1e3 for k in range(3))
        assert np.array_equal(ref, ref_q)
        levels, reached = int(ref.max()), int((ref >= 0).sum())
        say(f"{tag}: host route  gie_read_ground {rd:.2f} ms + BFS {npy:.1f} ms (numpy, level-synchronous) / {pyq:.1f} ms (Python queue); "
            f"{levels} levels, {reached} cells reached   [{os.path.basename(gie.mapper._lib._name)}]")
        if a.host_route:
            return
        n = size[0] * size[1]
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            d_goal = torch.from_numpy(goal).to(dev)
            d_nf = torch.empty(n, dtype=torch.int32, device=dev)
            d_pay = torch.empty(2 * n, dtype=torch.int32, device=dev)
            d_path, d_len = torch.empty(2 * 4096, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
            far = np.argwhere(ref == levels)[0][::-1]
            d_start = torch.from_numpy(((far.astype(np.float64) + np.array(pvt[:2])).astype(np.float32) * w).astype(np.float32)[None]).to(dev)
        calls = {"compute": lambda: m.ground_nf1_compute_dev(d_goal.data_ptr(), 1, csq),
                 "empty": lambda: m.ground_nf1_compute_dev(0, 0, csq),
                 "read": lambda: m.read_ground_nf1_dev(d_nf.data_ptr()),
                 "costmap": lambda: m.read_costmap_ground_nf1_dev(d_pay.data_ptr()),
                 "path": lambda: m.ground_nf1_path_dev(d_start.data_ptr(), 1, 4096, d_path.data_ptr(), d_len.data_ptr())}
        us = {}
        for name in ("empty", "compute", "read", "costmap", "path"):       # (the readers after a compute WITH the source)
            run = calls[name]
            run()
            m.sync()
            med = []
            m.profile_enable(True)
            for _ in range(5):
                m.profile_read()
                for _ in range(20):
                    run()
                tot, k = m.profile_read()["ground_nf1"]
                assert k == 20
                med.append(tot / k * 1e3)
            m.profile_enable(False)
            us[name] = float(np.median(med))
        m.sync()
        assert np.array_equal(d_nf.cpu().numpy().reshape(size[1], size[0]), ref) and d_len.item() == levels + 1
        per = (us["compute"] - us["empty"]) / max(levels, 1)
        say(f"{tag}: device      compute {us['compute']:.1f} us, without a source {us['empty']:.1f} us: {levels} levels at {per:.3f} us per level "
            f"({reached / max(levels, 1):.1f} cells a level); read {us['read']:.1f} us, CostMap {us['costmap']:.1f} us, one path of {min(levels + 1, 4096)} points {us['path']:.1f} us")
        say(f"{tag}: device route (compute + path) {us['compute'] + us['path']:.1f} us = 1 / {(rd + npy) * 1e3 / (us['compute'] + us['path']):.0f} of the host route with numpy")

    def central(m, csq, c):
        """the cell nearest to (c, c) in the largest 4-connected region of traversable cells of the current ground field"""
        from scipy import ndimage
        g = m.read_ground()
        lab, k = ndimage.label(N.traversable(g, csq))
        free = np.argwhere(lab == 1 + np.argmax(np.bincount(lab.ravel())[1:])) if k else np.zeros((0, 2), np.int64)
        if len(free) == 0:
            say(f"no traversable cell at clearance_sq {csq}: columns U/F/O/FNT {np.bincount(g['type'].ravel(), minlength=4).tolist()}, dist_sq max {int(g['dist_sq'].max())}")
            return None
        return free[np.argmin(np.abs(free - c).sum(axis=1))][::-1]

    def labelled(size, lab, w=0.1, cutoff=1.0):
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=cutoff, fast_mode=False))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        z = m.pivot()[2]
        m.ground_compute(z, z + size[2] - 1)
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
        goal = central(m, 4, 100)
        if goal is not None:
            measure("ugv 200x200", m, size, goal, 4, 3)
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
        goal = central(m, 0, 256)
        if goal is not None:
            measure("c5 512x512", m, size, goal, 0, 3)
        m.close()
    if "maze" in a.cases:
        size = (512, 512, 1)
        lab, first = serpentine(size[0], size[1], 2)
        m = labelled(size, lab[None])
        measure("maze 512x512", m, size, first, 0, 1)
        m.close()
    if "glb" in a.cases:
        size = (512, 769, 1)
        lab, first = serpentine(size[0], size[1], 16)
        m = labelled(size, lab[None])
        measure("maze 512x769 (global planes)", m, size, first, 0, 1)
        m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ground_nf1_time.py   (MI355X; gie_profile_read for the device times, wall clock for the host route)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

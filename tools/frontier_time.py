#!/usr/bin/env python3
"""Device time of the frontier clusters (include/gie.h gie_frontier_compute_dev / gie_read_frontier_clusters_dev) on an MI355X.

  python tools/frontier_time.py [--out profiles/r10_frontier]   prints one line per case; with --out also writes <out>_times.txt
  python tools/frontier_time.py --quick                         one round of each case (what a rocprofv3 kernel trace needs)

Cases, after a warm-up, each timed with device events on the mapper's stream over a window of at least 0.2 s:
  c5       BASELINE config 5's hash world at 512^3 (0.05 m), connectivity 26, min_size 8, 256 records: clearance 0 and 2 voxels;
  tube     256^3 free volume (with a sparse lattice of single occupied voxels) and one never-seen 1-voxel tube snaking along x
           (rows 16 voxels apart in y, layers 16 apart in z): its shell is one component that crosses the whole volume many times;
  specks   the same free volume with a never-seen voxel every fourth voxel on every axis: a quarter of a million components;
  read     the cluster reader (records + goal points of 256 entries) after the c5 compute."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def free_space(size):
    """labels [Z][Y][X] of a free volume with a lattice of single occupied voxels: a free voxel becomes a frontier only when its
    closest obstacle lies inside the volume, so free space needs obstacles within the cutoff"""
    lab = np.ones(size[::-1], np.int8)
    lab[0::4, 0::4, 0::8] = 2
    return lab


def tube(size, pitch):
    """labels [Z][Y][X] of a free volume with one unknown tube, and the tube's voxels in order (x, y, z)"""
    X, Y, Z = size
    lab = free_space(size)
    ys, zs = list(range(2, Y - 2, pitch)), list(range(2, Z - 2, pitch))
    cells, d = [], 0
    for li, z in enumerate(zs):
        yo = ys if li % 2 == 0 else ys[::-1]
        for yi, y in enumerate(yo):
            xs = np.arange(2, X - 2) if d % 2 == 0 else np.arange(X - 3, 1, -1)
            d += 1
            cells.append(np.stack([xs, np.full_like(xs, y), np.full_like(xs, z)], 1))
            if yi + 1 < len(yo):
                st = 1 if yo[yi + 1] > y else -1
                yy = np.arange(y + st, yo[yi + 1], st)
                cells.append(np.stack([np.full_like(yy, xs[-1]), yy, np.full_like(yy, z)], 1))
        if li + 1 < len(zs):
            zz = np.arange(z + 1, zs[li + 1])
            cells.append(np.stack([np.full_like(zz, xs[-1]), np.full_like(zz, yo[-1]), zz], 1))
    c = np.concatenate(cells)
    lab[c[:, 2], c[:, 1], c[:, 0]] = 0
    return lab, c


def timed(torch, st, fn, quick):
    """ms per call: device events on the mapper's stream over >= 0.2 s of calls (one call with quick)"""
    for _ in range(1 if quick else 3):
        fn()
    torch.cuda.synchronize()
    if quick:
        return float("nan")
    reps = 4
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 200.0:
            return ms / reps
        reps *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    import gie
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    # c5 at 512^3
    n, w = 512, 0.05
    size = (n, n, n)
    m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
    for k in range(2):
        pos, q = scenes.pose(k, w, delta_vox=8, yaw_deg=2.0)
        m.set_pose(pos, q)
        m.ogm_labels(scenes.hash_world_labels(scenes.local_pivot(pos, w, size), size, k).astype(np.int8))
        m.step()
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    torch.cuda.synchronize()
    for cl in (0.0, 2 * w):
        nc, nv = m.frontier_compute(cl, 8, 26, 256)
        ms = timed(torch, st, lambda: m.frontier_compute_dev(cl, 8, 26, 256), a.quick)
        say(f"c5     512^3 clearance {cl / w:.0f} voxels, connectivity 26, min_size 8: {ms:.4f} ms per compute; {nc} kept components, {nv} voxels in them")
    rec = torch.empty(256 * 80, dtype=torch.uint8, device=dev)
    goal = torch.empty((256, 3), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ms = timed(torch, st, lambda: m.read_frontier_clusters_dev(rec.data_ptr(), goal.data_ptr(), cnt.data_ptr()), a.quick)
    say(f"read   256 records and goal points: {ms:.4f} ms per call")
    m.close()

    n, w = 256, 0.125
    size = (n, n, n)
    for name, lab in (("tube  ", tube(size, 16)[0]), ("specks", None)):
        if lab is None:
            lab = free_space(size)
            lab[2:-2:4, 2:-2:4, 2:-2:4] = 0
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        torch.cuda.synchronize()
        nc, nv = m.frontier_compute(0.0, 1, 26, 256)
        rec_h, _, _ = m.read_frontier_clusters()
        ms = timed(torch, st, lambda: m.frontier_compute_dev(0.0, 1, 26, 256), a.quick)
        say(f"{name} 256^3 clearance 0, connectivity 26, min_size 1: {ms:.4f} ms per compute; {nc} components, {nv} voxels, the largest "
            f"of the first 256 has {int(rec_h['size'].max()) if len(rec_h) else 0}")
        m.close()
    if a.out and not a.quick:
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/frontier_time.py   (MI355X; windows of >= 0.2 s, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

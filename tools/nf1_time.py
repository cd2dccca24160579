#!/usr/bin/env python3
"""Device time of the NF1 navigation function (include/gie.h gie_nf1_compute_dev / gie_nf1_path_dev) on an MI355X.

  python tools/nf1_time.py [--out profiles/r09_nf1]     prints one line per case; with --out also writes <out>_times.txt
  python tools/nf1_time.py --quick                      one round of each case (what a rocprofv3 kernel trace needs)

Cases, after a warm-up, each timed with device events on the mapper's stream over a window of at least 0.2 s:
  c5     BASELINE config 5's hash world at 512^3 (0.05 m), one goal at the volume's centre, clearance 2 voxels: one compute;
  maze   256^3 walled volume with one 1-voxel corridor snaking along x (rows 16 voxels apart in y, layers 16 apart in z), the goal
         at one end: one compute (the BFS levels are printed);
  paths  64 descents of about 1000 steps each in the maze's field (starts on the corridor 1000 - 1063 steps from the goal)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def serpentine(size, pitch):
    """labels [Z][Y][X] of a walled volume with one free corridor, and the corridor's voxels in order (x, y, z)"""
    X, Y, Z = size
    lab = np.full((Z, Y, X), 2, np.int8)
    ys, zs = list(range(1, Y - 1, pitch)), list(range(1, Z - 1, pitch))
    cells, d = [], 0
    for li, z in enumerate(zs):
        yo = ys if li % 2 == 0 else ys[::-1]
        for yi, y in enumerate(yo):
            xs = np.arange(1, X - 1) if d % 2 == 0 else np.arange(X - 2, 0, -1)
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
    lab[c[:, 2], c[:, 1], c[:, 0]] = 1
    return lab, c


def timed(torch, st, fn, quick):
    """ms per call: device events on the mapper's stream over >= 0.2 s of calls (one call with quick)"""
    for _ in range(1 if quick else 3):
        fn()
    torch.cuda.synchronize()
    if quick:
        return float("nan")
    reps, best = 4, None
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

    # c5 at 512^3
    n, w = 512, 0.05
    size = (n, n, n)
    m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
    pvt = scenes.local_pivot((0.0, 0.0, 0.0), w, size)
    for k in range(2):
        m.set_pose((0.0, 0.0, 0.0))
        m.ogm_labels(scenes.hash_world_labels(pvt, size, k).astype(np.int8))
        m.step()
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    goal = torch.tensor([[0.0, 0.0, 0.0]], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ns = m.nf1_compute(goal.cpu().numpy(), 2 * w)
    f = m.read_nf1()
    ms = timed(torch, st, lambda: m.nf1_compute_dev(goal.data_ptr(), 1, 2 * w), a.quick)
    lines.append(f"c5    512^3 centre goal, clearance 2 voxels: {ms:.4f} ms per compute; sources {ns}, reached {(f >= 0).mean():.3f} of the "
                 f"voxels, BFS levels {f.max()}")
    print(lines[-1], flush=True)
    m.close()
    del f

    # maze at 256^3 and its paths
    n, w = 256, 0.125
    size = (n, n, n)
    m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
    lab, cells = serpentine(size, 16)
    for _ in range(2):
        m.set_pose((0.0, 0.0, 0.0))
        m.ogm_labels(lab)
        m.step()
    pv = np.array(m.pivot())
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    goal = torch.from_numpy(((cells[:1] + pv).astype(np.float32) * np.float32(w))).to(dev)
    torch.cuda.synchronize()
    ns = m.nf1_compute(goal.cpu().numpy(), 0.0)
    f = m.read_nf1()
    ms = timed(torch, st, lambda: m.nf1_compute_dev(goal.data_ptr(), 1, 0.0), a.quick)
    lines.append(f"maze  256^3 one corridor, {len(cells)} voxels: {ms:.4f} ms per compute ({1000 * ms / max(int(f.max()), 1):.2f} us per BFS level); "
                 f"sources {ns}, BFS levels {f.max()}")
    print(lines[-1], flush=True)
    starts = torch.from_numpy(((cells[1000:1064] + pv).astype(np.float32) * np.float32(w))).to(dev)
    ml = 1100
    dp = torch.empty((64, ml, 3), dtype=torch.int32, device=dev)
    dl = torch.empty(64, dtype=torch.int32, device=dev)
    ms = timed(torch, st, lambda: m.nf1_path_dev(starts.data_ptr(), 64, ml, dp.data_ptr(), dl.data_ptr()), a.quick)
    torch.cuda.synchronize()
    ln = dl.cpu().numpy()
    lines.append(f"paths 64 descents in the maze's field, {ln.min() - 1}-{ln.max() - 1} steps: {ms:.4f} ms per call")
    print(lines[-1], flush=True)
    m.close()
    if a.out and not a.quick:
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/nf1_time.py   (MI355X; windows of >= 0.2 s, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the goal-to-goal cost matrix (include/gie.h gie_costmat_compute_dev) on an MI355X, against the same points through
n separate gie_nf1_compute_dev calls on the same build.

  python tools/costmat_time.py [--out profiles/r18_costmat] [--sizes 256 512]     one line per case; with --out also <out>_times.txt

Scene: BASELINE config 5's hash world (0.05 m) after two updates, clearance 2 voxels.  Points: n = 8, 32 and 64 voxels drawn (fixed
seed) from what the NF1 field of the volume's centre reaches, so they are spread over the connected free space and all valid.
  matrix   one gie_costmat_compute_dev;
  n x NF1  for each point j: gie_nf1_compute_dev for the single goal j, gie_read_nf1_dev into a device buffer and a gather of the n
           values (what today's interface costs a caller who keeps everything on the device).
Both are timed with device events on the mapper's stream after one warm-up call, over at least 0.2 s of calls; the two matrices are
compared entry by entry."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def timed(torch, st, fn):
    """ms per call: device events on the mapper's stream over >= 0.2 s of calls, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    reps = 1
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
        reps *= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--points", type=int, nargs="+", default=[8, 32, 64])
    a = ap.parse_args()
    import torch
    import gie
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []
    w = 0.05
    for n in a.sizes:
        size = (n, n, n)
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
        pvt = scenes.local_pivot((0.0, 0.0, 0.0), w, size)
        for k in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(scenes.hash_world_labels(pvt, size, k).astype(np.int8))
            m.step()
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        m.nf1_compute(np.zeros((1, 3), np.float32), 2 * w)
        f = m.read_nf1()
        reach = np.flatnonzero(f.ravel() >= 0)
        del f
        pick = reach[np.random.default_rng(n).choice(len(reach), max(a.points), replace=False)]
        vox = np.stack([pick % n, (pick // n) % n, pick // (n * n)], 1)
        pts = ((vox + np.array(m.pivot())).astype(np.float32) * np.float32(w)).astype(np.float32)
        with torch.cuda.stream(st):
            dpts = torch.from_numpy(pts).to(dev)
            dfield = torch.empty(n * n * n, dtype=torch.int32, device=dev)
            didx = torch.from_numpy(pick.astype(np.int64)).to(dev)
        torch.cuda.synchronize()
        for k in a.points:
            dcost = torch.full((k, k), -7, dtype=torch.int32, device=dev)
            dref = torch.full((k, k), -7, dtype=torch.int32, device=dev)

            def matrix():
                m.costmat_dev(dpts.data_ptr(), k, dcost.data_ptr(), 0, 2 * w)

            def fields():
                with torch.cuda.stream(st):
                    for j in range(k):
                        m.nf1_compute_dev(dpts[j:j + 1].data_ptr(), 1, 2 * w)
                        m.read_nf1_dev(dfield.data_ptr())
                        dref[:, j] = dfield[didx[:k]]

            ms_m = timed(torch, st, matrix)
            ms_f = timed(torch, st, fields)
            m.sync()
            c, r = dcost.cpu().numpy(), dref.cpu().numpy()
            lines.append(f"c5 {n}^3 clearance 2 voxels, n = {k:2d}: matrix {ms_m:9.3f} ms, {k:2d} x NF1 {ms_f:9.3f} ms, ratio NF1 / matrix "
                         f"{ms_f / ms_m:6.2f}; largest entry {c.max()}, finite {(c >= 0).mean():.3f}, equal to the NF1 fields: {np.array_equal(c, r)}")
            print(lines[-1], flush=True)
        m.close()
        del dfield
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/costmat_time.py   (MI355X; one warm-up, windows of >= 0.2 s, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

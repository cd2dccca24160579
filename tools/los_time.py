#!/usr/bin/env python3
"""Device time of the line-of-sight queries (include/gie.h gie_los_prepare_dev / gie_los_segments_dev / gie_view_gain_dev) on an MI355X.

  python tools/los_time.py [--out profiles/r13_los]   prints one line per case; with --out also writes <out>_times.txt
  python tools/los_time.py --quick                    one round of each case (what a rocprofv3 kernel trace needs)

Cases on BASELINE config 5's hash world at 512^3 (0.05 m), after a warm-up, each timed with device events on the mapper's stream over
a window of at least 0.2 s:
  prepare   the opaque plane at clearance 0 and at 2 voxels;
  segments  10^5 segments between random points of the volume, shortened to a mean length of about 100 voxels; the voxel steps are
            counted from the results (a segment is walked to its end for `len`; up to `first` with loads);
  gain      64 views at free voxels, sphere of r_max = 60 voxels; the steps are not known from the result: the candidates are."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def timed(torch, st, fn, quick):
    """ms per call: device events on the mapper's stream over >= 0.2 s of calls (one call with quick)"""
    for _ in range(1 if quick else 3):
        fn()
    torch.cuda.synchronize()
    if quick:
        return float("nan")
    reps = 2
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
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    import torch
    import gie
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    n, w = a.size, 0.05
    size = (n, n, n)
    m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
    for k in range(2):
        pos, q = scenes.pose(k, w, delta_vox=8, yaw_deg=2.0)
        m.set_pose(pos, q)
        m.ogm_labels(scenes.hash_world_labels(scenes.local_pivot(pos, w, size), size, k).astype(np.int8))
        m.step()
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    torch.cuda.synchronize()
    pvt = np.array(m.pivot(), np.float32)
    for cl in (2 * w, 0.0):
        nop = m.los_prepare(cl, 0)
        ms = timed(torch, st, lambda: m.los_prepare_dev(cl, 0), a.quick)
        say(f"prepare  {n}^3 clearance {cl / w:.0f} voxels: {ms:.4f} ms per prepare; {nop} opaque voxels of {m.n}")
    # (the queries run on the plane of clearance 0)
    rng = np.random.default_rng(0)
    ns = 100000
    pa = rng.uniform(0, n - 1, (ns, 3))
    d = rng.normal(size=(ns, 3))
    pb = np.clip(pa + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(20, 180, (ns, 1)), 0, n - 1)
    to_world = lambda v: ((np.asarray(v, np.float32) + pvt) * np.float32(w)).astype(np.float32)      # noqa: E731
    ha, hb = to_world(pa), to_world(pb)
    hits = m.los_segments(ha, hb)
    steps_all = int(hits["len"].sum())
    steps_loaded = int(np.where(hits["first"] >= 0, hits["first"] + 1, hits["len"]).sum())
    da, db = torch.from_numpy(ha).to(dev), torch.from_numpy(hb).to(dev)
    dh = torch.empty(ns * 24, dtype=torch.uint8, device=dev)
    ms = timed(torch, st, lambda: m.los_segments_dev(da.data_ptr(), db.data_ptr(), ns, dh.data_ptr()), a.quick)
    say(f"segments {ns} segments, mean length {steps_all / ns:.1f} voxels, {int((hits['first'] == -1).sum())} clear: {ms:.4f} ms per call; "
        f"{steps_all / ms / 1e6:.2f} G voxel steps/s ({steps_loaded / ms / 1e6:.2f} G/s of them with loads)")
    loc_type = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
    free = np.argwhere(loc_type == 1)[:, ::-1]
    inner = free[np.all((free >= 64) & (free < n - 64), axis=1)] if n >= 192 else free
    nv, r = 64, 60
    views = gie.make_views(to_world(inner[rng.integers(0, len(inner), nv)]))
    sc = m.view_gain(views, 0.0, r * w)
    dv = torch.from_numpy(views.view(np.uint8)).to(dev)
    ds = torch.empty(nv * 16, dtype=torch.uint8, device=dev)
    ms = timed(torch, st, lambda: m.view_gain_dev(dv.data_ptr(), nv, ds.data_ptr(), 0.0, r * w), a.quick)
    cand = int(sc["candidates"].sum())
    say(f"gain     {nv} views, sphere r_max {r} voxels: {ms:.4f} ms per call; {cand} candidates ({cand / ms / 1e6:.3f} G candidates/s), "
        f"mean unknown {sc['unknown'].mean():.0f} frontier {sc['frontier'].mean():.0f} occupied {sc['occupied'].mean():.0f} per view")
    m.close()
    if a.out and not a.quick:
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/los_time.py   (MI355X; windows of >= 0.2 s, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

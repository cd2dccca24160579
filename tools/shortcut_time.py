#!/usr/bin/env python3
"""Device time of path shortcutting (include/gie.h gie_path_shortcut_dev) on an MI355X.

  python tools/shortcut_time.py [--out profiles/r16_shortcut]   prints one line per case; with --out also writes <out>_times.txt
  python tools/shortcut_time.py --quick                         one round of each case (what a rocprofv3 kernel trace needs)

BASELINE config 5's hash world at 512^3 (0.05 m): the NF1 field towards the volume's centre, gie_nf1_path_dev from 4096 starts at
random free voxels (max_len 1024), the opaque plane at clearance 0, then gie_path_shortcut_dev on those buffers with a look-ahead
of 64 and of 512, each timed with device events on the mapper's stream over a window of at least 0.2 s after a warm-up.
The work is counted from the result: a leg from index k to k' with top = min(k + K, m - 1) walked the chunks of 64 candidates
top, top - 64, ... down to the one that holds k' (all of the window for a forced leg whose first point is clear; none when that
point is opaque or outside); every candidate's line is handed to gie_los_segments, whose `first` / `len` say how many voxel steps
the walk took before it left.  Beside them: k_los_segments' own rate from profiles/r13_los_times.txt."""
import argparse
import os
import re
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


def candidates(path, lens, wp, info, K):
    """(path index, k, j) of every candidate the kernel walks or looks at, from the waypoints it gave (wp holds every record)"""
    pi, pk, pj = [], [], []
    max_len = path.shape[1]
    for i in range(len(lens)):
        m = min(max(int(lens[i]), 0), max_len)
        idx = wp["index"][i, :info["count"][i]]
        for t in range(1, len(idx)):
            k, k2 = int(idx[t - 1]), int(idx[t])
            top = min(k + K, m - 1)
            low = k + 1 if wp["forced"][i, t] else max(top - 64 * ((top - k2) // 64) - 63, k + 1)
            j = np.arange(low, top + 1)
            pi.append(np.full(len(j), i)), pk.append(np.full(len(j), k)), pj.append(j)
    return np.concatenate(pi), np.concatenate(pk), np.concatenate(pj)


def yardstick():
    try:
        txt = open(os.path.join(ROOT, "profiles", "r13_los_times.txt")).read()
        return re.search(r"segments .*?([0-9.]+ G voxel steps/s)", txt).group(1)
    except Exception:
        return "not found"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--paths", type=int, default=4096)
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
    to_world = lambda v: ((np.asarray(v, np.float32) + pvt) * np.float32(w)).astype(np.float32)      # noqa: E731
    loc_type = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
    free = np.argwhere(loc_type == 1)[:, ::-1]
    rng = np.random.default_rng(0)
    centre = np.array([n // 2] * 3)
    goal = free[np.argmin(((free - centre) ** 2).sum(axis=1))]
    starts = free[rng.integers(0, len(free), a.paths)]
    del loc_type, free
    m.nf1_compute(to_world(goal[None]), 0.0)
    npth, max_len = a.paths, 1024
    ds = torch.from_numpy(to_world(starts)).to(dev)
    dp = torch.zeros((npth, max_len, 3), dtype=torch.int32, device=dev)
    dl = torch.zeros(npth, dtype=torch.int32, device=dev)
    with torch.cuda.stream(st):
        m.nf1_path_dev(ds.data_ptr(), npth, max_len, dp.data_ptr(), dl.data_ptr())
    nop = m.los_prepare(0.0, 0)
    path, lens = dp.cpu().numpy(), dl.cpu().numpy()
    ms_ = np.clip(lens, 0, max_len)
    say(f"paths    {n}^3, {npth} starts at free voxels, goal at the centre: {int((lens > 0).sum())} paths, mean {ms_[ms_ > 0].mean():.0f} points, "
        f"longest {int(lens.max())} (max_len {max_len}); plane at clearance 0: {nop} opaque voxels")
    for K in (64, 512):
        cap = max_len
        dwp = torch.zeros((npth, cap, 6), dtype=torch.int32, device=dev)
        di = torch.zeros((npth, 4), dtype=torch.int32, device=dev)
        ms = timed(torch, st, lambda: m.path_shortcut_dev(dp.data_ptr(), dl.data_ptr(), npth, max_len, dwp.data_ptr(), di.data_ptr(), K, cap), a.quick)
        torch.cuda.synchronize()
        wp = dwp.cpu().numpy().view(gie.WAYPOINT_DTYPE).reshape(npth, cap)
        info = di.cpu().numpy().view(gie.SHORTCUT_INFO_DTYPE).reshape(npth)
        del dwp
        pi, pk, pj = candidates(path, lens, wp, info, K)
        walks = steps = 0
        for b in range(0, len(pi), 1 << 21):
            s = slice(b, b + (1 << 21))
            va = path[pi[s], pk[s]].astype(np.float32) * np.float32(w)
            vb = path[pi[s], pj[s]].astype(np.float32) * np.float32(w)
            h = m.los_segments(va, vb)
            walked = h["first"] != -2
            walked &= h["first"] != 0                                     # (an opaque first point: no walk)
            walks += int(walked.sum())
            steps += int(np.where(h["first"] > 0, h["first"], h["len"] - 1)[walked].sum())
        legs = int(info["count"].sum() - (info["count"] > 0).sum())
        say(f"shortcut K = {K}: {ms:.4f} ms per call; {int(info['count'].sum())} waypoints, {legs} legs ({int(info['forced'].sum())} forced), "
            f"{len(pi)} candidates looked at, {walks} walked ({walks / ms / 1e6:.3f} G candidate walks/s), {steps} voxel steps "
            f"({steps / ms / 1e6:.2f} G voxel steps/s)")
    say(f"yardstick k_los_segments (profiles/r13_los_times.txt): {yardstick()}")
    m.close()
    if a.out and not a.quick:
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/shortcut_time.py   (MI355X; windows of >= 0.2 s, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

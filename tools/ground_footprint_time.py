#!/usr/bin/env python3
"""Device time of ground footprints (include/gie.h gie_ground_footprints_dev) on an MI355X, and beside each time, as context, the
same poses through gie_ground_rollouts_dev with the disc that holds the rectangle (clearance_sq = front_sq + side_sq, no cost, no NF1):
what the ground stack could say about those trajectories before — a different, coarser question, not the same numbers.

  python tools/ground_footprint_time.py [--out profiles/r26_ground_footprint]     one line per case; with --out also <out>_times.txt

Scene: the 512 x 512 x 24 box scene of tools/ground_rollout_time.py (0.1 m voxels, 300 boxes, a never-seen slab) and its ground field
of the band [4, 15].  The trajectories are unicycle arcs from the most open free cell within 100 cells of the centre, steps of about
one cell, headings all around and turn rates of up to 0.1 rad per step (fixed seed), every pose with its true heading, for
(n, T) = (1024, 32), (65 536, 32);
two rectangles: 20 x 12 cells (front_sq 225, back_sq 25, side_sq 36) and 40 x 24 cells (900, 100, 144); clearance_sq 0; without and
with GIE_GROUND_FOOTPRINT_MARGIN.  The first 48 records of every case are compared with tests/ground_footprint_ref.py.
Each call: three warm-up calls, then 15 windows of at least 20 ms of calls between two device events on the mapper's stream; the
figure is the MEDIAN window's time per call, with the fastest and slowest window beside it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

W = 0.1
WINDOWS, WINDOW_MS = 15, 20.0
CASES = ((1024, 32), (65536, 32))
RECTS = (("20 x 12", (225, 25, 36)), ("40 x 24", (900, 100, 144)))
CHECKED = 48


def timed(torch, st, fn):
    """(median, min, max) us per call over WINDOWS windows of >= WINDOW_MS of calls, after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def window(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)
    reps = 1
    while window(reps) < WINDOW_MS:
        reps *= 2
    t = sorted(window(reps) / reps * 1000.0 for _ in range(WINDOWS))
    return t[len(t) // 2], t[0], t[-1]


def settle(m, lab, pos):
    for _ in range(2):
        m.set_pose(pos, (1.0, 0.0, 0.0, 0.0))
        m.ogm_labels(lab)
        m.step()


def arcs(start, n, T, rng):
    """((n, T, 2) cells with fractions, (n, T, 2) int32 headings): pose 0 = start, steps of 0.8 .. 1.2 cells, the heading turning by up to
    0.1 rad per step"""
    k = np.arange(T)[None, :]
    th = rng.uniform(0, 2 * np.pi, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 1)) * k
    step = rng.uniform(0.8, 1.2, (n, 1))
    d = np.stack([np.cos(th), np.sin(th)], 2)
    cells = np.asarray(start, np.float64) + np.concatenate([np.zeros((n, 1, 2)), np.cumsum((d * step[:, :, None])[:, :-1], 1)], 1)
    return cells, np.ascontiguousarray(np.rint(32767.0 * d).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gie
    import ground_footprint_ref as P
    from gie import scenes
    from stage_common import box_labels
    dev = torch.device("cuda", 0)
    size = (512, 512, 24)
    rng = np.random.default_rng(512)
    boxes = [(lo, lo + s) for lo, s in zip(np.stack([rng.integers(-250, 250, 300), rng.integers(-250, 250, 300), rng.integers(-14, 10, 300)], 1),
                                           rng.integers(2, 12, (300, 3)))]
    pos, _ = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
    pos = tuple(np.float32(v) for v in pos)
    pvt = scenes.local_pivot(pos, W, size)
    m = gie.Mapper(gie.make_config(W, size, cutoff_dist=1.0, fast_mode=False))
    settle(m, box_labels(pvt, size, 0, boxes, unknown_slab=6), pos)
    assert tuple(m.pivot()) == tuple(pvt)
    m.ground_compute(pvt[2] + 4, pvt[2] + 15, 3)
    g = m.read_ground()
    near = np.argwhere((g["type"][156:357, 156:357] == 1)) + 156      # the most open free cell within 100 cells of the centre
    start = near[np.argmax(g["dist_sq"][near[:, 0], near[:, 1]])][::-1]
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    lines = ["ground field 512 x 512, clearance_sq 0; arcs from cell (%d, %d), dist_sq %d there" % (start[0], start[1], g["dist_sq"][start[1], start[0]])]
    print(lines[0], flush=True)
    all_same = True
    for n, T in CASES:
        cells, hd = arcs(start, n, T, np.random.default_rng(n + T))
        pts = ((cells + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
        with torch.cuda.stream(st):
            dxy, dhd = torch.from_numpy(pts).to(dev), torch.from_numpy(hd).to(dev)
            drec = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
            drol = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        m.sync()
        for name, e in RECTS:
            disc = e[0] + e[2]
            t_disc = timed(torch, st, lambda: m.ground_rollouts_dev(dxy.data_ptr(), n, T, drol.data_ptr(), disc))
            m.sync()
            rol = np.frombuffer(drol.cpu().numpy().tobytes(), gie.GROUND_ROLLOUT_DTYPE)
            for margin in (False, True):
                t = timed(torch, st, lambda: m.ground_footprints_dev(dxy.data_ptr(), dhd.data_ptr(), n, T, drec.data_ptr(), e[0], e[1], e[2], 0, False, margin))
                m.sync()
                rec = np.frombuffer(drec.cpu().numpy().tobytes(), gie.GROUND_FOOTPRINT_DTYPE)
                want = P.footprints(g, pts[:CHECKED], hd[:CHECKED], pvt, W, e[0], e[1], e[2], 0, P.MARGIN if margin else 0)
                same = rec[:CHECKED].tobytes() == want.tobytes()
                all_same &= same
                lines.append("n = %5d, T = %3d, %s cells, margin %d: gie_ground_footprints_dev median %8.1f us (min %8.1f, max %8.1f); "
                             "rollouts at clearance_sq %4d: %8.1f us; first %d records equal the reference: %s" %
                             ((n, T, name, margin) + t + (disc, t_disc[0], CHECKED, same)))
                print(lines[-1], flush=True)
            lines.append("    footprint ends: %d complete, %d blocked, %d no placement; mean prefix %.1f poses, mean hit_cells of the blocked %.1f; the disc's mean prefix %.1f poses" %
                         ((rec["end"] == 0).sum(), (rec["end"] == 1).sum(), (rec["end"] == 2).sum(), rec["poses"].mean(),
                          rec["hit_cells"][rec["end"] == 1].mean() if (rec["end"] == 1).any() else 0.0, rol["poses"].mean()))
            print(lines[-1], flush=True)
    m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_footprint_time.py   (MI355X; three warm-up calls, 15 windows of >= 20 ms, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")
    if not all_same:
        sys.exit("a record differs from the reference")


if __name__ == "__main__":
    main()

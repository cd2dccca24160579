#!/usr/bin/env python3
"""Device time of the ground pose navigation function (include/gie.h gie_ground_pose_nf1_compute_dev, _path_dev, _query_dev) on an
MI355X, and beside it, as context only, the parent's gie_ground_nf1_compute_dev on the same field at the inscribed and the
circumscribed clearance of the same rectangle: a disc's answer to a different, coarser question, not the same numbers.

  python tools/ground_pose_nf1_time.py [--out profiles/r27_ground_pose_nf1]     one line per case; with --out also <out>_times.txt

Scene: the 512 x 512 x 24 box scene of tools/ground_nf1_time.py (0.1 m voxels, 300 boxes, a never-seen slab) and its ground field of
the band [4, 15] (the global-plane form: 4096 words a layer), and the 192 x 256 corner of the same world as a mapper of its own (768
words: the LDS form).  The rectangle is 20 x 12 cells (front_sq 225, back_sq 25, side_sq 36), clearance_sq 0; one goal, all eight
headings, at the most open free cell near the centre; without and with GIE_GROUND_POSE_NF1_REVERSE.  A compute with NO source (n = 0)
is timed too: the blocked plane, the C-space, the sources and one empty level — what a compute costs before the first level.
The levels run are max(pnf1) + 2 (levels 0 .. max + 1; the last finds nothing).  Path and query: 1 and 256 starts on free cells.
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
RECT = (225, 25, 36)                                            # 15 ahead, 5 behind, 6 to either side


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gie
    from gie import scenes
    from stage_common import box_labels
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(512)
    boxes = [(lo, lo + s) for lo, s in zip(np.stack([rng.integers(-250, 250, 300), rng.integers(-250, 250, 300), rng.integers(-14, 10, 300)], 1),
                                           rng.integers(2, 12, (300, 3)))]
    pos, _ = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
    pos = tuple(np.float32(v) for v in pos)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for size in ((512, 512, 24), (192, 256, 24)):
        pvt = scenes.local_pivot(pos, W, size)
        m = gie.Mapper(gie.make_config(W, size, cutoff_dist=1.0, fast_mode=False))
        settle(m, box_labels(pvt, size, 0, boxes, unknown_slab=6), pos)
        assert tuple(m.pivot()) == tuple(pvt)
        m.ground_compute(pvt[2] + 4, pvt[2] + 15, 3)
        g = m.read_ground()
        X, Y = size[0], size[1]
        lo = (Y // 2 - 60, X // 2 - 60)
        near = np.argwhere(g["type"][lo[0]:lo[0] + 121, lo[1]:lo[1] + 121] == 1) + np.array(lo)
        goal_c = near[np.argmax(g["dist_sq"][near[:, 0], near[:, 1]])][::-1]
        goal = ((goal_c + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32).reshape(1, 2)
        nwords = (X + 63) // 64 * Y
        say("ground field %d x %d (%d words a layer: %s), rectangle 20 x 12 cells, clearance_sq 0, goal cell (%d, %d), dist_sq %d there" %
            (X, Y, nwords, "LDS form" if nwords <= 768 else "global planes", goal_c[0], goal_c[1], g["dist_sq"][goal_c[1], goal_c[0]]))
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        free = np.argwhere(g["type"] == 1)[:, ::-1]
        pick = free[np.random.default_rng(7).choice(len(free), 256, replace=False)]
        starts = ((pick + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
        with torch.cuda.stream(st):
            dg, ds = torch.from_numpy(goal).to(dev), torch.from_numpy(starts).to(dev)
            dcnt = torch.zeros(2, dtype=torch.int32, device=dev)
            dq = torch.zeros(256, dtype=torch.int32, device=dev)
            dl = torch.zeros(256, dtype=torch.int32, device=dev)
            dp = torch.zeros(256 * 2048 * 3, dtype=torch.int32, device=dev)
        m.sync()
        t = timed(torch, st, lambda: m.ground_pose_nf1_compute_dev(0, 0, 0, dcnt.data_ptr(), *RECT))
        say("  compute without a source (blocked plane, C-space, sources, one empty level): median %9.1f us (min %9.1f, max %9.1f)" % t)
        for rev in (False, True):
            t = timed(torch, st, lambda: m.ground_pose_nf1_compute_dev(dg.data_ptr(), 0, 1, dcnt.data_ptr(), *RECT, 0, False, False, rev))
            m.sync()
            f, cs = m.read_ground_pose_nf1()
            cnt = dcnt.cpu().tolist()
            say("  gie_ground_pose_nf1_compute_dev reverse %d: median %9.1f us (min %9.1f, max %9.1f); %d levels, %d sources, %d free states of %d, %d reached" %
                ((int(rev),) + t + (int(f.max()) + 2, cnt[0], cnt[1], 8 * X * Y, int((f >= 0).sum()))))
            for n in (1, 256):
                tq = timed(torch, st, lambda: m.ground_pose_nf1_query_dev(ds.data_ptr(), 0, n, dq.data_ptr()))
                tp = timed(torch, st, lambda: m.ground_pose_nf1_path_dev(ds.data_ptr(), 0, n, 2048, dp.data_ptr(), dl.data_ptr()))
                m.sync()
                ln = dl.cpu().numpy()[:n]
                say("    %3d starts: query median %7.1f us (min %7.1f, max %7.1f); path (max_len 2048) median %8.1f us (min %8.1f, max %8.1f), longest %d, %d without a route" %
                    ((n,) + tq + tp + (int(ln.max()), int((ln == 0).sum()))))
        for name, csq in (("inscribed", 25), ("circumscribed", 225 + 36)):
            t = timed(torch, st, lambda: m.ground_nf1_compute_dev(dg.data_ptr(), 1, 0, csq))
            m.sync()
            nf = m.read_ground_nf1()
            say("  context: gie_ground_nf1_compute_dev at the %s clearance_sq %d: median %9.1f us (min %9.1f, max %9.1f); %d levels, %d cells reached" %
                ((name, csq) + t + (int(nf.max()) + 2, int((nf >= 0).sum()))))
        m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_pose_nf1_time.py   (MI355X; three warm-up calls, 15 windows of >= 20 ms, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

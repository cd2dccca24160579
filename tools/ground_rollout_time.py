#!/usr/bin/env python3
"""Device time of ground rollouts (include/gie.h gie_ground_rollouts_dev) on an MI355X, beside the only other way to the same numbers
on the same build: three _dev calls over all poses, whose n * T records the host would still have to reduce.

  python tools/ground_rollout_time.py [--out profiles/r25_ground_rollout]     one line per case; with --out also <out>_times.txt

Scene: the 512 x 512 x 24 box scene of tests/test_ground_nf1_gpu.py::test_at_size_512x512x24 (0.1 m voxels, 300 boxes, a never-seen
slab), its ground field of the band [4, 15] and the ground NF1 of one goal at clearance_sq 4.  The rollouts are unicycle arcs from
the free cell nearest the centre, steps of about one cell, headings all around and turn rates of up to 0.1 rad per step (fixed
seed), for (n, T) = (256, 32), (4096, 32), (4096, 128), (65 536, 32).
  rollouts  gie_ground_rollouts_dev at clearance_sq 4, inflate_sq 64, with the NF1 flag: n records;
  chain     gie_ground_segments_dev over the n (T - 1) legs + gie_ground_query_dev over the n T poses + gie_ground_nf1_query_dev over
            the n T poses: the sum of the three device times.  The host's reduction of the n T records and their read-back are NOT
            counted, and the chain cannot give `cells` and `cost` at all.
The tool also reduces the chain's records in numpy and compares every field both ways can produce: end, poses, hit, min_dist_sq and
the three NF1 fields.
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
CASES = ((256, 32), (4096, 32), (4096, 128), (65536, 32))


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
    """(n, T, 2) cells (fractions): pose 0 = start, steps of 0.8 .. 1.2 cells, the heading turning by up to 0.1 rad per step"""
    k = np.arange(T)[None, :]
    th = rng.uniform(0, 2 * np.pi, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 1)) * k
    step = rng.uniform(0.8, 1.2, (n, 1))
    d = np.stack([np.cos(th), np.sin(th)], 2) * step[:, :, None]
    return np.asarray(start, np.float64) + np.concatenate([np.zeros((n, 1, 2)), np.cumsum(d[:, :-1], 1)], 1)


def reduce_chain(gie, xy, pvt, seg, cell, steps, csq):
    """what the host would make of the chain's records: the fields of gie_ground_rollout that they determine"""
    n, T = xy.shape[0], xy.shape[1]
    inside = cell["inside"] != 0
    t0, d0 = cell["type"][:, 0], cell["dist_sq"][:, 0]
    blocked0 = ~(((t0 == 1) | (t0 == 3)) & ((d0 == -1) | (d0 >= csq)))
    bad = np.concatenate([(~inside[:, :1]) | blocked0[:, None], seg["first"] != -1], 1)
    m = np.where(bad.any(1), bad.argmax(1), T)
    out = np.zeros(n, gie.GROUND_ROLLOUT_DTYPE)
    rows = np.arange(n)
    at = np.minimum(m, T - 1)
    out["poses"] = m
    out["end"] = np.where(m == T, 0, np.where(inside[rows, at], 1, 2))
    c0 = np.floor(xy[:, 0] / np.float32(W) + np.float32(0.5)).astype(np.int64)      # gie_pos2coord in float32 (finite here)
    hit = np.where((m == 0)[:, None], c0, seg["hit"][rows, np.maximum(at - 1, 0)])
    out["hit"] = np.where((out["end"] == 1)[:, None], hit, 0)
    legs = np.where(np.arange(T - 1)[None, :] < (m - 1)[:, None], seg["min_dist_sq"], np.iinfo(np.int32).max)
    out["min_dist_sq"] = np.where(m > 0, np.minimum(d0, legs.min(1) if T > 1 else d0), 0)
    reached = np.arange(T)[None, :] < m[:, None]
    vals = np.where(reached & (steps >= 0), steps, np.iinfo(np.int32).max)
    any_ = (vals != np.iinfo(np.int32).max).any(1)
    out["nf1_end"] = np.where(m > 0, steps[rows, np.maximum(m - 1, 0)], -1)
    out["nf1_min"] = np.where(any_, vals.min(1), -1)
    out["nf1_min_at"] = np.where(any_, vals.argmin(1), -1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gie
    from gie import scenes
    from stage_common import box_labels
    dev = torch.device("cuda", 0)
    size, csq, isq = (512, 512, 24), 4, 64
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
    free = np.argwhere((g["type"] == 1) & (g["dist_sq"] >= 25))
    start = free[np.argmin(np.abs(free - 256).sum(axis=1))][::-1]
    goal = free[np.argmin(np.abs(free - np.array([400, 380])).sum(axis=1))][::-1]

    def xy(cells):
        return ((np.asarray(cells, np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    m.ground_nf1_compute(xy([goal]), csq)
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    lines = ["ground field 512 x 512, clearance_sq %d, inflate_sq %d; arcs from cell (%d, %d), NF1 to cell (%d, %d)" % (csq, isq, start[0], start[1], goal[0], goal[1])]
    print(lines[0], flush=True)
    worst = 0.0
    for n, T in CASES:
        pts = xy(arcs(start, n, T, np.random.default_rng(n + T)))
        with torch.cuda.stream(st):
            dxy = torch.from_numpy(pts).to(dev)
            da = torch.from_numpy(np.ascontiguousarray(pts[:, :-1])).to(dev)
            db = torch.from_numpy(np.ascontiguousarray(pts[:, 1:])).to(dev)
            drec = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
            dhit = torch.zeros(n * (T - 1) * 24, dtype=torch.uint8, device=dev)
            dcell = torch.zeros(n * T * 16, dtype=torch.uint8, device=dev)
            dsteps = torch.zeros(n * T, dtype=torch.int32, device=dev)
        m.sync()
        t_new = timed(torch, st, lambda: m.ground_rollouts_dev(dxy.data_ptr(), n, T, drec.data_ptr(), csq, isq, False, True))
        t_seg = timed(torch, st, lambda: m.ground_segments_dev(da.data_ptr(), db.data_ptr(), n * (T - 1), dhit.data_ptr(), csq))
        t_qry = timed(torch, st, lambda: m.ground_query_dev(dxy.data_ptr(), n * T, dcell.data_ptr()))
        t_nf1 = timed(torch, st, lambda: m.ground_nf1_query_dev(dxy.data_ptr(), n * T, dsteps.data_ptr()))
        m.sync()
        rec = np.frombuffer(drec.cpu().numpy().tobytes(), gie.GROUND_ROLLOUT_DTYPE)
        seg = np.frombuffer(dhit.cpu().numpy().tobytes(), gie.GROUND_HIT_DTYPE).reshape(n, T - 1)
        cell = np.frombuffer(dcell.cpu().numpy().tobytes(), gie.GROUND_CELL_DTYPE).reshape(n, T)
        want = reduce_chain(gie, pts, pvt, seg, cell, dsteps.cpu().numpy().reshape(n, T), csq)
        same = all(np.array_equal(rec[k], want[k]) for k in ("end", "poses", "hit", "min_dist_sq", "nf1_end", "nf1_min", "nf1_min_at"))
        chain = t_seg[0] + t_qry[0] + t_nf1[0]
        worst = max(worst, t_new[0] / chain)
        lines.append("n = %5d, T = %3d: gie_ground_rollouts_dev median %8.1f us (min %8.1f, max %8.1f); segments %8.1f + query %8.1f + nf1 query %8.1f = %8.1f us; "
                     "rollouts / chain %.2f; same fields: %s" % ((n, T) + t_new + (t_seg[0], t_qry[0], t_nf1[0], chain, t_new[0] / chain, same)))
        print(lines[-1], flush=True)
        lines.append("    ends: %d complete, %d blocked, %d left; mean prefix %.1f poses, %.1f cells" %
                     ((rec["end"] == 0).sum(), (rec["end"] == 1).sum(), (rec["end"] == 2).sum(), rec["poses"].mean(), rec["cells"].mean()))
        print(lines[-1], flush=True)
    lines.append("largest rollouts / chain: %.2f (required: <= 1)" % worst)
    print(lines[-1], flush=True)
    m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_rollout_time.py   (MI355X; three warm-up calls, 15 windows of >= 20 ms, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

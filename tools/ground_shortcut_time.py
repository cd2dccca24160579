#!/usr/bin/env python3
"""Device time of ground line of sight (include/gie.h gie_ground_segments_dev, gie_ground_shortcut_dev) on an MI355X, beside the 3-D
section's way to the same waypoints on the same build.

  python tools/ground_shortcut_time.py [--out profiles/r21_ground_shortcut]     one line per case; with --out also <out>_times.txt

Scene: the 512 x 512 x 24 box scene of tests/test_ground_nf1_gpu.py::test_at_size_512x512x24 (0.1 m voxels, 300 boxes, a never-seen
slab), its ground field of the band [4, 15] and the ground NF1 of the free cell nearest the centre at clearance_sq 9; the paths are
that field's descents (max_len 1024) from starts drawn (fixed seed) among the cells it reaches, written by gie_ground_nf1_path_dev.
  segments  gie_ground_segments_dev at clearance_sq 9: 1 and 65 536 segments between cells drawn inside the rectangle;
  shortcut  gie_ground_shortcut_dev at clearance_sq 9: 1 and 256 paths, lookahead 64 and 256, max_wp 64;
  3-D       the same waypoints through the line-of-sight section: a 512 x 512 x 1 volume labelled with the ground field's column
            types (so its EDT is the ground field's), gie_los_prepare_dev at clearance 2.9 voxels (edt < 2.9 is dist_sq < 9) + gie_path_shortcut_dev on the same
            paths with z appended — a prepare per call, as the ground call builds its blocked plane per call.
Each case: three warm-up calls, then 15 windows of at least 20 ms of calls between two device events on the mapper's stream; the
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
    size, csq, max_len, max_wp = (512, 512, 24), 9, 1024, 64
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
    free = np.argwhere((g["type"] == 1) & (g["dist_sq"] >= csq))
    goal = free[np.argmin(np.abs(free - 256).sum(axis=1))][::-1]

    def xy(cells):
        return ((np.asarray(cells, np.float64).reshape(-1, 2) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    m.ground_nf1_compute(xy([goal]), csq)
    nf = m.read_ground_nf1()
    reach = np.argwhere(nf >= 64)[:, ::-1]
    r = np.random.default_rng(21)
    starts = xy(reach[r.choice(len(reach), 256, replace=False)])
    seg = r.integers(0, 512, (2, 65536, 2))
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    with torch.cuda.stream(st):
        ds = torch.from_numpy(starts).to(dev)
        dpath = torch.zeros((256, max_len, 2), dtype=torch.int32, device=dev)
        dlen = torch.zeros(256, dtype=torch.int32, device=dev)
        m.ground_nf1_path_dev(ds.data_ptr(), 256, max_len, dpath.data_ptr(), dlen.data_ptr())
        da, db = torch.from_numpy(xy(seg[0])).to(dev), torch.from_numpy(xy(seg[1])).to(dev)
        dhit = torch.zeros(65536 * 24, dtype=torch.uint8, device=dev)
        dwp = torch.zeros(256 * max_wp * 24, dtype=torch.uint8, device=dev)
        dinfo = torch.zeros(256 * 16, dtype=torch.uint8, device=dev)
    m.sync()
    lens = dlen.cpu().numpy()
    lines = ["ground field 512 x 512, clearance_sq %d; 256 paths of %d .. %d points (median %d)" % (csq, lens.min(), lens.max(), int(np.median(lens)))]
    print(lines[0], flush=True)
    ground = {}
    for n in (1, 65536):
        t = timed(torch, st, lambda: m.ground_segments_dev(da.data_ptr(), db.data_ptr(), n, dhit.data_ptr(), csq))
        lines.append("gie_ground_segments_dev  n = %5d:                 median %9.1f us  (min %9.1f, max %9.1f)" % ((n,) + t))
        print(lines[-1], flush=True)
    hits = np.frombuffer(dhit.cpu().numpy().tobytes(), gie.GROUND_HIT_DTYPE)
    lines.append("  65 536 segments: %d clear, %d blocked, mean len %.1f cells" % ((hits["first"] == -1).sum(), (hits["first"] >= 0).sum(), hits["len"].mean()))
    print(lines[-1], flush=True)
    for n in (1, 256):
        for K in (64, 256):
            t = timed(torch, st, lambda: m.ground_shortcut_dev(dpath.data_ptr(), dlen.data_ptr(), n, max_len, dwp.data_ptr(), dinfo.data_ptr(), K, max_wp, csq))
            m.sync()
            ground[n, K] = (np.frombuffer(dwp.cpu().numpy().tobytes(), gie.GROUND_WAYPOINT_DTYPE).reshape(256, max_wp)[:n].copy(),
                            np.frombuffer(dinfo.cpu().numpy().tobytes(), gie.SHORTCUT_INFO_DTYPE)[:n].copy(), t)
            lines.append("gie_ground_shortcut_dev  n = %5d, lookahead %3d:  median %9.1f us  (min %9.1f, max %9.1f); mean count %.1f"
                         % ((n, K) + t + (ground[n, K][1]["count"].mean(),)))
            print(lines[-1], flush=True)
    path2 = dpath.cpu().numpy()
    m.close()
    # the 3-D section on a flat volume that holds the same scene
    flat = (512, 512, 1)
    lab = np.where(g["type"] == 2, 2, np.where(g["type"] == 0, 0, 1)).astype(np.int8)[None]
    m3 = gie.Mapper(gie.make_config(W, flat, cutoff_dist=1.0, fast_mode=False))
    settle(m3, lab, pos)
    p3 = m3.pivot()
    assert tuple(p3[:2]) == tuple(pvt[:2])
    path3 = np.concatenate([path2, np.full(path2.shape[:2] + (1,), p3[2], np.int32)], 2)
    st3 = torch.cuda.ExternalStream(m3.stream_handle(), device=dev)
    with torch.cuda.stream(st3):
        dpath3 = torch.from_numpy(path3).to(dev)
        dlen3 = torch.from_numpy(lens).to(dev)
    m3.sync()
    for n in (1, 256):
        for K in (64, 256):
            def both():
                m3.los_prepare_dev(0.29, gie.LOS_UNKNOWN_OPAQUE)      # (metres: 2.9 voxels; edt < 2.9 is dist_sq < 9 on integers)
                m3.path_shortcut_dev(dpath3.data_ptr(), dlen3.data_ptr(), n, max_len, dwp.data_ptr(), dinfo.data_ptr(), K, max_wp)
            t = timed(torch, st3, both)
            m3.sync()
            w3 = np.frombuffer(dwp.cpu().numpy().tobytes(), gie.WAYPOINT_DTYPE).reshape(256, max_wp)[:n]
            i3 = np.frombuffer(dinfo.cpu().numpy().tobytes(), gie.SHORTCUT_INFO_DTYPE)[:n]
            w2, i2, t2 = ground[n, K]
            same = i3.tobytes() == i2.tobytes() and all(                  # (the written records only: count may exceed max_wp)
                np.array_equal(w3[k][key][:min(int(i3["count"][k]), max_wp)], w2[k][key][:min(int(i3["count"][k]), max_wp)])
                for k in range(n) for key in ("index", "forced"))
            lines.append("3-D prepare + shortcut   n = %5d, lookahead %3d:  median %9.1f us  (min %9.1f, max %9.1f); ground / 3-D %.2f; same waypoints: %s"
                         % ((n, K) + t + (t2[0] / t[0], same)))
            print(lines[-1], flush=True)
    m3.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_shortcut_time.py   (MI355X; three warm-up calls, 15 windows of >= 20 ms, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

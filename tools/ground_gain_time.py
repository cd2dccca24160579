#!/usr/bin/env python3
"""Device time of ground view gain (include/gie.h gie_ground_view_gain_dev, gie_ground_view_mask_dev) on an MI355X, beside the 3-D
section's way to the same counts on the same build.

  python tools/ground_gain_time.py [--out profiles/r24_ground_gain]     one line per case; with --out also <out>_times.txt

Scene: the 512 x 512 x 24 box scene of tests/test_ground_nf1_gpu.py::test_at_size_512x512x24 (0.1 m voxels, 300 boxes, a never-seen
slab) and its ground field of the band [4, 15]; the views stand on FREE cells drawn with a fixed seed, no half planes, UNKNOWN
transparent.
  gain   gie_ground_view_gain_dev: 1, 64 and 256 views at r_max 60 and 200 cells;
  mask   gie_ground_view_mask_dev of the first view at both radii;
  3-D    the only way to the same counts without this section: a 512 x 512 x 1 volume labelled with the ground field's column types
         (the construction of tools/ground_shortcut_time.py), gie_los_prepare_dev + gie_view_gain_dev on the same points with z
         appended — a prepare per call, as the ground call builds its opaque plane per call.  candidates, unknown and occupied must
         be equal; the flat volume derives its own FNT voxels from its one layer, so `frontier` is compared and reported apart.
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
    size, nmax = (512, 512, 24), 256
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
    free = np.argwhere(g["type"] == 1)[:, ::-1]
    cells = free[np.random.default_rng(24).choice(len(free), nmax, replace=False)]
    xy = ((cells.astype(np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
    radii = (60, 200)
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    with torch.cuda.stream(st):
        dxy = torch.from_numpy(xy).to(dev)
        dout = torch.zeros(nmax * 16, dtype=torch.uint8, device=dev)
        dmask = torch.zeros(size[0] * size[1], dtype=torch.uint8, device=dev)
    m.sync()
    lines = ["ground field 512 x 512 of the band [4, 15]: %d UNKNOWN, %d FREE, %d OCCUPIED, %d FNT columns; views on FREE cells"
             % tuple(int((g["type"] == k).sum()) for k in range(4))]
    print(lines[0], flush=True)
    ground = {}
    for rc in radii:
        r = float(np.float32(rc) * np.float32(W))
        for n in (1, 64, nmax):
            t = timed(torch, st, lambda: m.ground_view_gain_dev(dxy.data_ptr(), 0, n, dout.data_ptr(), 0.0, r))
            m.sync()
            sc = np.frombuffer(dout.cpu().numpy().tobytes(), gie.VIEW_SCORE_DTYPE)[:n].copy()
            ground[n, rc] = (sc, t)
            cand = int(sc["candidates"].sum())
            lines.append("gie_ground_view_gain_dev  n = %3d, r_max %3d cells:  median %9.1f us  (min %9.1f, max %9.1f); %9d candidates, %.2f G candidates/s"
                         % ((n, rc) + t + (cand, cand / t[0] / 1000.0)))
            print(lines[-1], flush=True)
        t = timed(torch, st, lambda: m.ground_view_mask_dev(dxy.data_ptr(), 0, dmask.data_ptr(), dout.data_ptr(), 0.0, r))
        m.sync()
        mk = dmask.cpu().numpy()
        sc = np.frombuffer(dout.cpu().numpy().tobytes(), gie.VIEW_SCORE_DTYPE)[0]
        ok = sc.tobytes() == ground[1, rc][0][0].tobytes() and int((mk > 0).sum()) == int(sc["candidates"])
        lines.append("gie_ground_view_mask_dev           r_max %3d cells:  median %9.1f us  (min %9.1f, max %9.1f); %d hidden, %d visible; score as the gain's: %s"
                     % ((rc,) + t + (int((mk == 1).sum()), int((mk == 2).sum()), ok)))
        print(lines[-1], flush=True)
    m.close()
    # the 3-D section on a flat volume that holds the same scene
    flat = (512, 512, 1)
    lab = np.where(g["type"] == 2, 2, np.where(g["type"] == 0, 0, 1)).astype(np.int8)[None]
    m3 = gie.Mapper(gie.make_config(W, flat, cutoff_dist=1.0, fast_mode=False))
    settle(m3, lab, pos)
    p3 = m3.pivot()
    assert tuple(p3[:2]) == tuple(pvt[:2])
    views = gie.make_views(np.concatenate([xy, np.full((nmax, 1), np.float32(p3[2]) * np.float32(W), np.float32)], 1))
    st3 = torch.cuda.ExternalStream(m3.stream_handle(), device=dev)
    with torch.cuda.stream(st3):
        dviews = torch.from_numpy(views.view(np.uint8).reshape(-1)).to(dev)
    m3.sync()
    for rc in radii:
        r = float(np.float32(rc) * np.float32(W))
        for n in (1, 64, nmax):
            def both():
                m3.los_prepare_dev(0.0, 0)
                m3.view_gain_dev(dviews.data_ptr(), n, dout.data_ptr(), 0.0, r, -1.0)
            t = timed(torch, st3, both)
            m3.sync()
            s3 = np.frombuffer(dout.cpu().numpy().tobytes(), gie.VIEW_SCORE_DTYPE)[:n]
            s2, t2 = ground[n, rc]
            same = all(np.array_equal(s3[k], s2[k]) for k in ("candidates", "unknown", "occupied"))
            lines.append("3-D prepare + view gain   n = %3d, r_max %3d cells:  median %9.1f us  (min %9.1f, max %9.1f); ground / 3-D %.3f; "
                         "same candidates, unknown, occupied: %s; same frontier: %s"
                         % ((n, rc) + t + (t2[0] / t[0], same, np.array_equal(s3["frontier"], s2["frontier"]))))
            print(lines[-1], flush=True)
    m3.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_gain_time.py   (MI355X; three warm-up calls, 15 windows of >= 20 ms, device events on the mapper's stream)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the ground cost matrix costs on an MI355X, beside what a user did before it: n computes of the ground navigation function.

  python tools/ground_costmat_time.py [--out profiles/r23_ground_costmat_times.txt] [--cases ugv,c5,maze,glb]

Four cases (include/gie.h "ground cost matrix"):
  ugv   the reference's UGV configuration, 200 x 200 x 24 at 0.05 m (tools/ground_nf1_time.py's room of boxes), clearance_sq 4;
  c5    the headline workload as bench.py builds it (the hash world at 512^3; bench.py itself is not touched), the ground field of a
        band of 24 layers, clearance_sq 0;
  maze  512 x 512 x 1, ONE serpentine corridor of one cell (rows two apart), the points spread evenly over its first 20 000 cells:
        every search runs one cell a level, the two at the ends 20 000 levels — the time per level with n compute units busy;
  glb   512 x 769 x 1 — one row beyond the LDS budget: a pair of planes per source in global memory — a corridor with rows 16 apart,
        the points over its first 5 000 cells.
Per case and n: the points are drawn (seeded) from the largest traversable region, the first two of them a far pair, so the matrix
has no -1 and a search runs max(row) + 1 levels (it ends one level after its last target).  Through the _dev forms: device time of
one matrix call from the "ground_nf1" entry of gie_profile_read, median of five rounds; the baseline in the same session, from the
same entry: n times gie_ground_nf1_compute_dev with the single goal j and gie_ground_nf1_query_dev at all points, whose columns must
equal the matrix (in the two mazes up to n = 8: a compute there runs the whole corridor, 130 000 and 25 000 levels).  "per level" =
(the call - the call with n = 1, which runs no level) / the levels of the longest search."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def serpentine(X, Y, pitch):
    """(label plane, the corridor's cells in order)"""
    lab = np.full((Y, X), 2, np.int8)
    cells = []
    rows = list(range(1, Y - 1, pitch))
    for i, y in enumerate(rows):
        xs = list(range(1, X - 1)) if i % 2 == 0 else list(range(X - 2, 0, -1))
        cells += [(x, y) for x in xs]
        if i + 1 < len(rows):
            cells += [(xs[-1], yy) for yy in range(y + 1, rows[i + 1])]
    c = np.array(cells)
    lab[c[:, 1], c[:, 0]] = 1
    return lab, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="ugv,c5,maze,glb")
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    import bench
    import gie
    import ground_nf1_ref as N
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def world(m, cells):
        pvt = m.pivot()
        return ((np.asarray(cells, np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(m.cfg.voxel_width)).astype(np.float32)

    def region_points(m, csq, n_max, seed):
        """n_max cells of the largest traversable region: a far pair first (the cell nearest the low corner and the one farthest from
        it in steps), then a seeded draw"""
        g = m.read_ground()
        trav = N.traversable(g, csq)
        lab, k = ndimage.label(trav)
        big = lab == 1 + np.argmax(np.bincount(lab.ravel())[1:])
        cells = np.argwhere(big)[:, ::-1]
        first = cells[np.argmin(cells.sum(axis=1))]
        src = np.zeros(trav.shape, bool)
        src[first[1], first[0]] = True
        nf = N.propagate(trav, src)
        far = np.argwhere(nf == nf.max())[0][::-1]
        rng = np.random.default_rng(seed)
        return np.concatenate([[first, far], cells[rng.choice(len(cells), n_max - 2, replace=False)]]), int(big.sum())

    def profiled(m, run, brackets, rounds, calls):
        run()
        m.sync()
        med = []
        m.profile_enable(True)
        for _ in range(rounds):
            m.profile_read()
            for _ in range(calls):
                run()
            tot, k = m.profile_read()["ground_nf1"]
            assert k == calls * brackets, (k, calls, brackets)
            med.append(tot / calls * 1e3)
        m.profile_enable(False)
        return float(np.median(med))

    def measure(tag, m, cells, csq, ns, rounds=5, calls=10, base_rounds=3, base_upto=256, empty=None):
        """returns the time of the call with n = 1 (no level runs), for the next call on the same field"""
        xy = world(m, cells)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        n_max = max(ns)
        with torch.cuda.stream(st):
            d_xy = torch.from_numpy(xy).to(dev)
            d_cost = torch.empty(n_max * n_max, dtype=torch.int32, device=dev)
            d_cols = torch.empty(n_max * n_max, dtype=torch.int32, device=dev)
        for n in ns:
            us = profiled(m, lambda: m.ground_costmat_dev(d_xy.data_ptr(), n, d_cost.data_ptr(), 0, csq), 1, rounds, calls)
            m.sync()
            cost = d_cost.cpu().numpy()[:n * n].reshape(n, n).copy()

            def baseline():
                for j in range(n):
                    m.ground_nf1_compute_dev(d_xy.data_ptr() + 8 * j, 1, csq)
                    m.ground_nf1_query_dev(d_xy.data_ptr(), n, d_cols.data_ptr() + 4 * n * j)
            assert (cost >= 0).all(), tag
            base = None
            if n <= base_upto:
                base = profiled(m, baseline, 2 * n, base_rounds, 1)
                m.sync()
                assert np.array_equal(d_cols.cpu().numpy()[:n * n].reshape(n, n).T, cost), tag
            levels = int(cost.max()) + 1 if n > 1 else 0
            if n == 1:
                empty = us
            per = f", {(us - empty) / levels:.3f} us per level over {levels} levels" if levels and empty is not None else ""
            tail = f";  n x (compute + query) {base:11.1f} us = {base / us:6.1f} x the matrix" if base is not None else ""
            say(f"{tag}: n = {n:3d}  matrix {us:9.1f} us{per}{tail}")
        return empty

    def labelled(size, lab, w=0.1, cutoff=1.0):
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=cutoff, fast_mode=False))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        z = m.pivot()[2]
        m.ground_compute(z, z + size[2] - 1)
        return m

    if "ugv" in a.cases:
        size = (200, 200, 24)
        rng = np.random.default_rng(18)
        lab = np.ones((size[2], size[1], size[0]), np.int8)
        lab[0] = 2
        for _ in range(40):
            x, y, sx, sy, h = rng.integers(0, 190), rng.integers(0, 190), rng.integers(2, 12), rng.integers(2, 12), rng.integers(2, 24)
            lab[:h, y:y + sy, x:x + sx] = 2
        lab[:, :, :6] = 0
        m = gie.Mapper(gie.make_config(0.05, size, cutoff_dist=2.0, fast_mode=False))
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        z = m.pivot()[2]
        m.ground_compute(z + 1, z + 23)                        # the body's band: the floor lies below it
        cells, big = region_points(m, 4, 256, 1)
        say(f"ugv 200x200: clearance_sq 4, the largest region {big} cells")
        measure("ugv 200x200", m, cells, 4, (1, 8, 64, 256))
        m.close()
    if "c5" in a.cases:
        pre = bench.PRESETS["c5"]
        size, w, total = pre["size"], pre["voxel"], 8
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=pre["cutoff"], fast_mode=pre["fast"], max_blocks=bench.pool_blocks("c5", size, total),
                                       wave_workgroups=bench.WAVE_GRID["wgs"], place_tries=bench.PLACE_TRIES))
        feed = bench.HashWorldFeed(torch, scenes, dev, w, size, (0, 0, 0))
        feed.prepare(0, total)
        for i in range(total):
            feed.step_input(m, i)
            m.step()
        m.sync()
        z = m.pivot()[2]
        m.ground_compute(z + 244, z + 267)
        cells, big = region_points(m, 0, 256, 2)
        say(f"c5 512x512: clearance_sq 0, the largest region {big} cells")
        measure("c5 512x512", m, cells, 0, (1, 8, 64, 256))
        m.close()
    if "maze" in a.cases:
        size = (512, 512, 1)
        lab, corridor = serpentine(size[0], size[1], 2)
        m = labelled(size, lab[None])
        empty = None
        for n in (2, 8, 64, 256):                               # (n points evenly over the same stretch: the same levels for every n)
            at = np.linspace(0, 20000, n).astype(int)
            empty = measure("maze 512x512", m, corridor[at], 0, (1, n) if n == 2 else (n,), rounds=3, calls=3, base_rounds=1, base_upto=8, empty=empty)
        m.close()
    if "glb" in a.cases:
        size = (512, 769, 1)
        lab, corridor = serpentine(size[0], size[1], 16)
        m = labelled(size, lab[None])
        empty = None
        for n in (2, 8, 64):
            at = np.linspace(0, 5000, n).astype(int)
            empty = measure("maze 512x769 (global planes)", m, corridor[at], 0, (1, n) if n == 2 else (n,), rounds=3, calls=3, base_rounds=1, base_upto=8, empty=empty)
        m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ground_costmat_time.py   (MI355X; gie_profile_read for every device time, the matrix and its baseline in one session)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

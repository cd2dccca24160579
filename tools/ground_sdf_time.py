#!/usr/bin/env python3
"""Device time of the ground signed distance field (include/gie.h "ground signed distance") on an MI355X, beside the host route to the
same numbers on the same machine: read_ground + scipy's distance transform of the complement + scipy.ndimage.map_coordinates.

  python tools/ground_sdf_time.py [--out profiles/r30_ground_sdf] [--sizes 200,512] [--worlds thin,unknown] [--rounds 5]     with --out also <out>_times.txt

Worlds of X x X x 8 voxels of 0.1 m, the ground field of the whole height:
  thin     horizontal walls one cell thick, eight rows apart: no interior obstacle column, the gate closes;
  unknown  the same walls, a never-seen third of the columns (x < X / 3) and a few 20 x 20 boxes, computed with
           GIE_GROUND_UNKNOWN_BLOCKS: the exact transform runs.
Every figure is the MEDIAN of `rounds` rounds of 20 _dev calls, each call's device time read from gie_profile_read (the kernels'
own events; a memset is not in it):
  compute        gie_ground_compute_dev: the projection and k_ground_line, the "ground" entry;
  inside pass    the "ground" entry of the FIRST gie_ground_query_sdf_dev (one point) after each of those computes: the count and the
                 transform.  It does k_ground_line's work on the complement and stores less; `compute` holds that kernel and the
                 projection (a kernel trace splits them: DESIGN.md 30);
  query          gie_ground_query_sdf_dev, 10^5 and 10^6 points along coherent trajectories (arcs with steps of a fifth of a cell);
  rollouts       gie_ground_sdf_rollouts_dev, 4 096 x 32 and 65 536 x 32, records only and with both per-point outputs, beside ONE
                 gie_ground_query_sdf_dev over the same n * T points.
The host route is timed once per world with time.perf_counter: read_ground (with its copy), the two scipy calls on 10^5 points."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

W = 0.1
CALLS = 20


def world(X, kind, rng):
    lab = np.ones((X, X), np.int8)
    for y in range(4, X - 4, 8):
        x0 = int(rng.integers(2, X // 2))
        lab[y, x0:x0 + int(rng.integers(X // 8, X // 2))] = 2
    if kind == "unknown":
        for _ in range(max(X // 50, 2)):
            x, y = rng.integers(X // 3, X - 24, 2)
            lab[y:y + 20, x:x + 20] = 2
        lab[:, :X // 3] = 0
    return lab


def arcs(n, T, X, rng, step=0.2):
    k = np.arange(T)[None, :]
    th = rng.uniform(0, 2 * np.pi, (n, 1)) + rng.uniform(-0.02, 0.02, (n, 1)) * k
    d = np.stack([np.cos(th), np.sin(th)], 2) * step
    return rng.uniform(8, X - 8, (n, 1, 2)) + np.concatenate([np.zeros((n, 1, 2)), np.cumsum(d[:, :-1], 1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="200,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default="thin,unknown")
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    import gie
    import ground_sdf_ref as S
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def med(fn, key):
        """median over the rounds of the mean device time (us) of CALLS calls of fn under profile entry `key`"""
        out = []
        for _ in range(a.rounds):
            tot = 0.0
            for _ in range(CALLS):
                m.profile_read()
                fn()
                tot += m.profile_read()[key][0]
            out.append(tot / CALLS * 1000.0)
        return float(np.median(out))

    for X in [int(v) for v in a.sizes.split(",")]:
        size = (X, X, 8)
        for kind in a.worlds.split(","):
            rng = np.random.default_rng(X)
            lab = world(X, kind, rng)
            m = gie.Mapper(gie.make_config(W, size, cutoff_dist=1.0, fast_mode=False))
            for _ in range(2):
                m.set_pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
                m.ogm_labels(np.repeat(lab[None], 8, axis=0))
                m.step()
            pvt = m.pivot()
            blocks = kind == "unknown"
            st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)

            def xy(cells):
                return ((np.asarray(cells, np.float64) + np.array(pvt[:2])).astype(np.float32) * np.float32(W)).astype(np.float32)
            m.ground_compute(pvt[2], pvt[2] + 7, 1, blocks)
            g = m.read_ground()
            f = S.field(g, size, blocks)
            got = m.read_ground_sdf()
            same = np.array_equal(got["inside_dist_sq"], f["inside_dist_sq"]) and got["sdf"].tobytes() == f["sdf"].tobytes()
            say("%d x %d, %s: %d obstacle columns, %d interior, largest inside_dist_sq %d; the device's planes equal the reference: %s" %
                (X, X, kind, f["obs"].sum(), S.interior(f["obs"]).sum(), f["inside_dist_sq"].max(), same))
            with torch.cuda.stream(st):
                one = torch.from_numpy(xy([[X // 2, X // 2]])).to(dev)
                dd1 = torch.zeros(4, dtype=torch.float32, device=dev)
            m.sync()
            m.profile_enable(True)
            t_compute = med(lambda: m.ground_compute_dev(pvt[2], pvt[2] + 7, 1, blocks, 0), "ground")

            def first():
                m.ground_compute_dev(pvt[2], pvt[2] + 7, 1, blocks, 0)
                m.profile_read()
                m.ground_query_sdf_dev(one.data_ptr(), 1, dd1.data_ptr(), 0, 0)
            t_inside = med(first, "ground")
            say("    compute (projection + k_ground_line) %8.1f us; inside pass (count + transform) %8.1f us" % (t_compute, t_inside))
            for n in (100000, 1000000):
                pts = xy(arcs(n // 100, 100, X, np.random.default_rng(n)))
                with torch.cuda.stream(st):
                    dxy = torch.from_numpy(pts).to(dev)
                    dd = torch.zeros(n, dtype=torch.float32, device=dev)
                    dg = torch.zeros(2 * n, dtype=torch.float32, device=dev)
                    df = torch.zeros(n, dtype=torch.uint8, device=dev)
                m.sync()
                t = med(lambda: m.ground_query_sdf_dev(dxy.data_ptr(), n, dd.data_ptr(), dg.data_ptr(), df.data_ptr()), "ground_query")
                say("    query %7d points %8.1f us (%.2f ns a point)" % (n, t, t * 1000.0 / n))
                if n == 100000:                                 # the host route on the same points
                    t0 = time.perf_counter()
                    gh = m.read_ground()
                    t1 = time.perf_counter()
                    obs = S.obstacles(gh, blocks)
                    pos = ndimage.distance_transform_edt(~obs) if obs.any() else np.full(obs.shape, np.inf)
                    neg = ndimage.distance_transform_edt(obs) if not obs.all() else np.full(obs.shape, np.inf)
                    sd = np.where(obs, 1.0 - neg, pos)
                    t2 = time.perf_counter()
                    u = pts.reshape(-1, 2).astype(np.float64) / W - np.array(pvt[:2])
                    ndimage.map_coordinates(sd, [u[:, 1], u[:, 0]], order=1, mode="nearest")
                    t3 = time.perf_counter()
                    say("    host route: read_ground %8.1f us + scipy distance transforms %8.1f us + map_coordinates of 100000 points %8.1f us" %
                        ((t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6))
            for n, T in ((4096, 32), (65536, 32)):
                pts = xy(arcs(n, T, X, np.random.default_rng(n), 1.0))
                with torch.cuda.stream(st):
                    dxy = torch.from_numpy(pts).to(dev)
                    drec = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
                    dd = torch.zeros(n * T, dtype=torch.float32, device=dev)
                    dg = torch.zeros(2 * n * T, dtype=torch.float32, device=dev)
                    df = torch.zeros(n * T, dtype=torch.uint8, device=dev)
                m.sync()
                t_rec = med(lambda: m.ground_sdf_rollouts_dev(dxy.data_ptr(), n, T, drec.data_ptr(), 0, 0, 0.3), "ground_query")
                t_all = med(lambda: m.ground_sdf_rollouts_dev(dxy.data_ptr(), n, T, drec.data_ptr(), dd.data_ptr(), dg.data_ptr(), 0.3), "ground_query")
                t_qry = med(lambda: m.ground_query_sdf_dev(dxy.data_ptr(), n * T, dd.data_ptr(), dg.data_ptr(), df.data_ptr()), "ground_query")
                rec = np.frombuffer(drec.cpu().numpy().tobytes(), gie.GROUND_SDF_ROLLOUT_DTYPE)
                say("    rollouts %5d x %2d: records only %8.1f us, with dist and grad %8.1f us; one query of the %d points %8.1f us; mean prefix %.1f points, %d with a point inside" %
                    (n, T, t_rec, t_all, n * T, t_qry, rec["points"].mean(), (rec["first_in"] >= 0).sum()))
            m.profile_enable(False)
            m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + "_times.txt", "w") as fh:
            fh.write("# python tools/ground_sdf_time.py   (MI355X; medians of %d rounds of %d _dev calls, device times from gie_profile_read)\n" % (a.rounds, CALLS))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the ground costmap costs on an MI355X, beside the host route it replaces.

  python tools/ground_time.py [--out profiles/r18_ground_times.txt] [--host-route]

Two sizes (include/gie.h "ground costmap"):
  ugv   the reference's UGV configuration, 200 x 200 x 24 at 0.05 m (cfg/ugv_laser3D_params.yaml), a room of boxes, band = the
        whole height;
  c5    the headline workload as bench.py builds it (the hash world at 512^3; its helpers are imported, bench.py itself is not
        touched), with a band of 24 layers and with the full height.
Per case, through the _dev forms: device time of compute, read and CostMap from the "ground" entry of gie_profile_read (median of
five rounds of 20 calls), the stream time of a compute (device events around 20 calls enqueued back to back, profile off: the
memset and the gaps between the launches too), and 100 000 queries ("ground_query").  The host route — gie_read_local of the
types, the projection in numpy, scipy's distance transform with indices — is timed on the wall clock, median of five;
--host-route measures only that, so that it can be taken on another build of the library (GIE_LIB) in the same session.
The split of a compute into its two kernels comes from a kernel trace (rocprofv3 --kernel-trace --stats) of the same calls."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-route", action="store_true", help="only the host route (any build of the library)")
    ap.add_argument("--cases", default="ugv,c5")
    a = ap.parse_args()
    import torch
    import bench
    import gie
    import ground_ref as R
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def host_route(m, pvt, lo, hi):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            vtype = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
            t1 = time.perf_counter()
            R.field(vtype, pvt, lo, hi)
            ts.append((t1 - t0, time.perf_counter() - t1))
        rd, cpu = np.median([t[0] for t in ts]), np.median([t[1] for t in ts])
        return rd * 1e3, cpu * 1e3

    def measure(tag, m, size, lo, hi):
        pvt = m.pivot()
        z0, z1 = R.band(pvt[2], size[2], lo, hi)
        rd, cpu = host_route(m, pvt, lo, hi)
        say(f"{tag}: host route  gie_read_local(types) {rd:.2f} ms + numpy projection and scipy transform {cpu:.2f} ms = {rd + cpu:.2f} ms   [{os.path.basename(gie.mapper._lib._name)}]")
        if a.host_route:
            return
        n = size[0] * size[1]
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        bufs = {k: torch.empty(n * c, dtype=torch.int32, device=dev) for k, c in (("dist", 1), ("coc", 2), ("top", 1), ("pay", 2))}
        dtype = torch.empty(n, dtype=torch.int8, device=dev)
        dcnt = torch.zeros(4, dtype=torch.int32, device=dev)
        xy = ((np.random.default_rng(0).uniform(-2, np.array(size[:2]) + 2, (100000, 2)) + np.array(pvt[:2])) * m.cfg.voxel_width).astype(np.float32)
        dxy, dq = torch.from_numpy(xy).to(dev), torch.empty(4 * len(xy), dtype=torch.int32, device=dev)
        calls = {"compute": lambda: m.ground_compute_dev(lo, hi, 1, False, dcnt.data_ptr()),
                 "read": lambda: m.read_ground_dev(dtype.data_ptr(), bufs["dist"].data_ptr(), bufs["coc"].data_ptr(), bufs["top"].data_ptr()),
                 "costmap": lambda: m.read_costmap_ground_dev(bufs["pay"].data_ptr()),
                 "query": lambda: m.ground_query_dev(dxy.data_ptr(), len(xy), dq.data_ptr())}
        us = {}
        for name, run in calls.items():
            for _ in range(3):
                run()
            m.sync()
            med = []
            m.profile_enable(True)
            for _ in range(5):
                m.profile_read()
                for _ in range(20):
                    run()
                tot, k = m.profile_read()["ground_query" if name == "query" else "ground"]
                assert k == 20
                med.append(tot / k * 1e3)
            m.profile_enable(False)
            us[name] = float(np.median(med))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(20):
            calls["compute"]()
        e1.record(st)
        e1.synchronize()
        stream_us = e0.elapsed_time(e1) / 20 * 1e3
        counts = dcnt.cpu().numpy()
        vol = n * (z1 - z0)
        say(f"{tag}: device      compute {us['compute']:.1f} us ({stream_us:.1f} us on the stream), read {us['read']:.1f} us, CostMap {us['costmap']:.1f} us, "
            f"100 000 queries {us['query']:.1f} us; band of {z1 - z0} layers = {vol / 1e6:.2f} MB of types; columns U/F/O/FNT {counts.tolist()}")
        say(f"{tag}: device route (compute + CostMap) {us['compute'] + us['costmap']:.1f} us = 1 / {(rd + cpu) * 1e3 / (us['compute'] + us['costmap']):.0f} of the host route")

    if "ugv" in a.cases:
        size, w = (200, 200, 24), 0.05
        m = gie.Mapper(gie.make_config(w, size, cutoff_dist=2.0, fast_mode=False))
        rng = np.random.default_rng(18)
        lab = np.ones((size[2], size[1], size[0]), np.int8)
        lab[0] = 2
        for _ in range(40):
            x, y, sx, sy, h = rng.integers(0, 190), rng.integers(0, 190), rng.integers(2, 12), rng.integers(2, 12), rng.integers(2, 24)
            lab[:h, y:y + sy, x:x + sx] = 2
        lab[:, :, :6] = 0
        for _ in range(2):
            m.set_pose((0.0, 0.0, 0.0))
            m.ogm_labels(lab)
            m.step()
        z = m.pivot()[2]
        measure("ugv 200x200x24, whole height", m, size, z, z + 23)
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
        measure("c5 512^3, 24 layers", m, size, z + 244, z + 267)
        measure("c5 512^3, full height", m, size, z, z + 511)
        m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ground_time.py   (MI355X; gie_profile_read for the kernels, device events on the mapper's stream, wall clock for the host route)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

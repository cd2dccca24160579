#!/usr/bin/env python3
"""Device time of the signed distance field (include/gie.h gie_read_sdf_dev / gie_query_sdf_dev) at 512^3, on an MI355X.

  python tools/sdf_time.py [--size 512] [--out profiles/r08_sdf]      events + rocprofv3 run, writes <out>_times.txt, <out>_kernels.txt
  python tools/sdf_time.py --inner                                    (the workload alone: what the rocprofv3 run traces)

Worlds: "c5" = BASELINE config 5's hash world (1 % occupancy, no voxel deeper than an obstacle's surface); "boxes" = solid boxes
4 - 80 voxels on a side plus an external fence box that leaves occupied slabs 24 voxels thick (the exact pass runs).
Cases, after a warm-up, each in synchronised windows of at least 0.2 s timed with device events on the mapper's stream:
  first call   the computation of the inside distances that the first SDF call after a map update enqueues: per-kernel device
               time through gie_profile_enable (bracket "sdf"), summed over the updates of the window; the map updates in
               between are not counted;
  read_sdf_dev 512^3 sdf plane into a device buffer (cache warm);
  query_dev    10^6 random points of the volume (cache warm)."""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _world(kind, size, w, frame):
    from gie import scenes
    pvt = scenes.local_pivot((0.0, 0.0, 0.0), w, size)
    if kind == "c5":
        return pvt, scenes.hash_world_labels(pvt, size, frame).astype(np.int8), None
    X, Y, Z = size
    lab = np.ones((Z, Y, X), np.int8)
    rng = np.random.default_rng(11)
    for k in range(40):
        s = rng.integers(4, 80, size=3)
        lo = rng.integers(0, np.array(size) - s)
        if (frame + k) % 4 == 3:
            continue
        lab[lo[2]:lo[2] + s[2], lo[1]:lo[1] + s[1], lo[0]:lo[0] + s[0]] = 2
    ll = (np.array(pvt) + 24) * w
    ur = (np.array(pvt) + np.array(size) - 24) * w
    return pvt, lab, (np.array([ll], np.float32), np.array([ur], np.float32), np.array([1], np.uint8))


class Rig:
    def __init__(self, kind, n):
        import torch
        import gie
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.size, self.w = (n, n, n), 0.05
        self.m = gie.Mapper(gie.make_config(self.w, self.size, cutoff_dist=2.0, fast_mode=False, wave_workgroups=160))
        self.labels = []
        for f in range(2):
            _, lab, boxes = _world(kind, self.size, self.w, f)
            self.labels.append(torch.from_numpy(lab).to(self.dev))
        if boxes is not None:
            self.m.set_ext_boxes(*boxes)
        torch.cuda.synchronize()
        self.k = 0
        self.st = torch.cuda.ExternalStream(self.m.stream_handle(), device=self.dev)
        npts = 1000000
        rng = np.random.default_rng(1)
        from gie import scenes
        pvt = np.array(scenes.local_pivot((0.0, 0.0, 0.0), self.w, self.size), np.float32)
        u = rng.uniform(0, n - 1, size=(npts, 3)).astype(np.float32)
        self.npts = npts
        self.xyz = torch.from_numpy(((u + pvt) * np.float32(self.w)).astype(np.float32)).to(self.dev)
        self.dist = torch.empty(npts, dtype=torch.float32, device=self.dev)
        self.grad = torch.empty((npts, 3), dtype=torch.float32, device=self.dev)
        self.flags = torch.empty(npts, dtype=torch.uint8, device=self.dev)
        self.plane = torch.empty(self.size[::-1], dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()

    def update(self):
        self.m.set_pose((0.0, 0.0, 0.0))
        self.m.ogm_labels_dev(self.labels[self.k & 1].data_ptr())
        self.m.step()
        self.k += 1

    def query(self, n=None):
        self.m.query_sdf_dev(self.xyz.data_ptr(), n or self.npts, self.dist.data_ptr(), self.grad.data_ptr(), self.flags.data_ptr())

    def read(self):
        self.m.read_sdf_dev(self.plane.data_ptr(), 0)

    def window(self, fn, min_s=0.2):
        """ms per call of fn over synchronised windows of >= min_s (device events on the mapper's stream)"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        calls, ms, t0 = 0, 0.0, time.time()
        while time.time() - t0 < min_s or calls < 3:
            self.m.sync()
            e0.record(self.st)
            for _ in range(20):
                fn()
            e1.record(self.st)
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            calls += 20
        return ms / calls

    def first_call(self, min_s=0.2):
        """device time of the inside-distance computation per update (profile bracket "sdf"), ms"""
        self.m.profile_enable(True)
        self.m.profile_read()
        tot, n, t0 = 0.0, 0, time.time()
        while time.time() - t0 < min_s or n < 5:
            self.update()
            self.m.profile_read()                                  # drop the update's own kernels
            self.query(1)                                          # the first SDF call after the update
            p = self.m.profile_read()
            tot += p["sdf"][0]
            n += p["sdf"][1]
        self.m.profile_enable(False)
        return tot / n


def measure(n):
    lines = []
    for kind in ("c5", "boxes"):
        r = Rig(kind, n)
        for _ in range(3):                                         # warm-up
            r.update(); r.query(); r.read()
        r.m.sync()
        first = r.first_call()
        r.update(); r.query(1); r.m.sync()
        rd = r.window(r.read)
        q = r.window(r.query)
        sd = r.m.read_sdf()
        deep = int((sd["inside_dist_sq"] > 1).sum())
        lines.append("%-6s %d^3: first SDF call after an update %.4f ms (device time of its kernels); read_sdf_dev %.4f ms; "
                     "query_sdf_dev 1e6 points %.4f ms; voxels deeper than the surface %d, deepest inside_dist_sq %d"
                     % (kind, n, first, rd, q, deep, int(sd["inside_dist_sq"].max())))
        print(lines[-1], flush=True)
        r.m.close()
    return lines


def inner(n):
    for kind in ("c5", "boxes"):
        r = Rig(kind, n)
        for _ in range(6):
            r.update(); r.query(); r.read()
        r.m.sync()
        r.m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_sdf"))
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.inner:
        inner(a.size)
        return
    lines = measure(a.size)
    with open(a.out + "_times.txt", "w") as f:
        f.write("# python tools/sdf_time.py --size %d   (MI355X; windows of >= 0.2 s, device events / gie_profile_enable)\n" % a.size)
        f.write("\n".join(lines) + "\n")
    if a.no_trace:
        return
    with tempfile.TemporaryDirectory() as d:                      # a run of its own: the tracer adds nothing to the times above
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sdf", "--", sys.executable, os.path.abspath(__file__),
                        "--inner", "--size", str(a.size)], check=True, timeout=600)
        db = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocpd_summary.py"), "stats", db[0]], capture_output=True,
                             text=True, check=True).stdout
    with open(a.out + "_kernels.txt", "w") as f:
        f.write("# rocprofv3 --kernel-trace --stats -- python tools/sdf_time.py --inner --size %d   (MI355X; c5 and boxes worlds, 6 "
                "updates each, every update followed by a 10^6-point query and a read_sdf_dev)\n" % a.size)
        f.write(out)
    print(out)


if __name__ == "__main__":
    main()

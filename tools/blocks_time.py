#!/usr/bin/env python3
"""Device time of the global block summaries (include/gie.h "global block summaries") on an MI355X, beside the route they replace on
the same mapper: gie_cloud_global_dev with the known mask and GIE_CLOUD_TYPE — one 16-byte record per known voxel of the map, which
a host would then have to bin into blocks.

  python tools/blocks_time.py [--out profiles/r34_blocks_time.txt] [--size 512] [--updates 10]

The headline workload as bench.py builds it (BASELINE config 5: the hash world at 512^3, bench's pool, wave grid and placement
draws; its helpers are imported, bench.py itself is not touched), after `updates` steady-state updates.  Every figure is stream
time: device events on the mapper's stream around 20 calls enqueued back to back after 5 warm-up calls, so it holds the memsets and
the gaps between the launches too.
  types     gie_blocks_summary_dev, flags 0, the open box, min_fnt 0, every record into a device buffer of exactly its size;
  dist      the same with GIE_BLOCKS_DIST;
  frontier  flags 0 and min_fnt 1: the call an explorer makes (fewer records);
  grid      flags 0 with the grid of the data's block box, no list;
  cloud     gie_cloud_global_dev, FREE | OCCUPIED | FNT, GIE_CLOUD_TYPE, every point into a device buffer of exactly its size.
Bytes per call are the stage's own traffic by its definition: 8 bytes per slot handed out (the key) + 512 per live block (the types)
+ 8 per FREE or FNT voxel with distances + 32 per record; the fraction is of the 8 TB/s HBM peak."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

CALLS, WARM = 20, 5
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help="cube side (default: the preset's 512)")
    ap.add_argument("--updates", type=int, default=10)
    a = ap.parse_args()
    import torch
    import bench
    import gie
    from gie import scenes
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    pre = bench.PRESETS["c5"]
    size = (a.size,) * 3 if a.size else pre["size"]
    w, total = pre["voxel"], a.updates + 4
    cfg = gie.make_config(w, size, cutoff_dist=pre["cutoff"], fast_mode=pre["fast"], max_blocks=bench.pool_blocks("c5", size, total),
                          wave_workgroups=bench.WAVE_GRID["wgs"], place_tries=bench.PLACE_TRIES)
    m = gie.Mapper(cfg)
    feed = bench.HashWorldFeed(torch, scenes, dev, w, size, (0, 0, 0))
    feed.prepare(0, total)
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    for k in range(a.updates):
        feed.step_input(m, k)
        m.step()
    m.sync()
    handed = m.stats()["blocks_total"]

    def timed(run):
        for _ in range(WARM):
            run()
        m.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(CALLS):
            run()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS * 1e3                  # us per call

    rec, count = m.blocks_summary(dist=True)
    assert count == len(rec)
    passable = int(rec["n_free"].astype(np.int64).sum() + rec["n_fnt"].astype(np.int64).sum())
    known = passable + int(rec["n_occupied"].astype(np.int64).sum())
    n_front = int((rec["n_fnt"] > 0).sum())
    say(f"workload  c5 hash world {size[0]}^3, voxel {w} m, pool {cfg.max_blocks} slots, {handed} handed out after {a.updates} updates; "
        f"{count} blocks with a known voxel, {n_front} of them with FNT voxels, {known} known voxels ({passable} FREE or FNT)")
    lo, hi = rec["key"].min(0), rec["key"].max(0)
    cells = int(np.prod(hi - lo + 1))
    dcnt = torch.zeros(4, dtype=torch.int32, device=dev)
    dout = torch.empty((max(count, 1), 8), dtype=torch.int32, device=dev)
    dgrid = torch.empty((cells,), dtype=torch.int32, device=dev)
    base = 8 * handed + 512 * count                              # (a block without a known voxel is read too: `count` is a lower bound)
    forms = [("types", lambda: m.blocks_summary_dev(dout.data_ptr(), dcnt.data_ptr(), 0, max_records=count), base + 32 * count),
             ("dist", lambda: m.blocks_summary_dev(dout.data_ptr(), dcnt.data_ptr(), 0, dist=True, max_records=count), base + 32 * count + 8 * passable),
             ("frontier", lambda: m.blocks_summary_dev(dout.data_ptr(), dcnt.data_ptr(), 0, min_fnt=1, max_records=count), base + 32 * n_front),
             ("grid", lambda: m.blocks_summary_dev(0, 0, dgrid.data_ptr(), tuple(lo), tuple(hi)), base + 8 * cells)]
    us = {}
    for name, run, nbytes in forms:
        us[name] = timed(run)
        say(f"{name:9s} {us[name]:8.1f} us per call; {nbytes / 1e6:8.1f} MB per call = {nbytes / us[name] / 1e6:6.2f} TB/s = "
            f"{nbytes / (us[name] * 1e-6) / PEAK:5.3f} of the 8 TB/s peak")
    mask = (1 << gie.VOX_FREE) | (1 << gie.VOX_OCCUPIED) | (1 << gie.VOX_FNT)
    _, points = m.cloud_global(mask, gie.CLOUD_TYPE, max_points=0)
    dpts = torch.empty((max(points, 1), 4), dtype=torch.float32, device=dev)
    us["cloud"] = timed(lambda: m.cloud_global_dev(dpts.data_ptr(), dcnt.data_ptr(), mask, gie.CLOUD_TYPE, max_points=points))
    nbytes = base + 16 * points
    say(f"cloud     {us['cloud']:8.1f} us per call; {points} points, {nbytes / 1e6:8.1f} MB per call (16 bytes a point, which the host then bins)")
    say(f"ratio     cloud / types {us['cloud'] / us['types']:.1f}, cloud / dist {us['cloud'] / us['dist']:.1f}, dist / types {us['dist'] / us['types']:.2f}")
    assert points == known
    m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# python tools/blocks_time.py   (MI355X; device events on the mapper's stream around %d calls after %d warm-up calls)\n" % (CALLS, WARM))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

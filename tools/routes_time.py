#!/usr/bin/env python3
"""Device time of the global block routes (include/gie.h "global block routes") on an MI355X, beside the grid-only form of the block
summaries on the same mapper and beside the route they replace: gie_blocks_summary with a grid to the host and a host BFS on it.

  python tools/routes_time.py [--out profiles/r35_routes_time.txt] [--size 512] [--updates 10]

The headline workload as bench.py builds it (BASELINE config 5: the hash world at 512^3, bench's pool, wave grid and placement
draws; its helpers are imported, bench.py itself is not touched), after `updates` steady-state updates.  Device figures are stream
time: device events on the mapper's stream around 20 calls enqueued back to back after 5 warm-up calls, so they hold the memsets and
the gaps between the launches too.  Two boxes: the data's block box (more than 3072 words a plane at 512^3: the propagation keeps
five planes in global memory) and a box cut out of it around the robot with nx <= 64 and ny * nz <= 3072 (all six planes in LDS).
  grid      gie_blocks_summary_dev, flags 0, the grid of the box, no list: the same walk of the pool, 520 bytes per block;
  nosource  gie_routes_compute_dev without a goal and without GIE_ROUTES_FROM_FRONTIERS: two memsets, the links, the prep and a
            propagation that counts the planes and ends after one empty level;
  robot     the same with the robot's position as the goal: the whole compute; (robot - nosource) / max_steps is a level;
  frontier  GIE_ROUTES_FROM_FRONTIERS and no goal: many sources, few levels;
  query     gie_routes_query_dev at the first FNT voxel of every frontier block.
The route replaced: gie_blocks_summary's grid to the HOST (wall clock, with the copy) and a numpy BFS on it — 6-connected dilation
of the cells with min_free passable voxels, which cannot see the face links at all (wall clock).
Bytes per compute are the links' own traffic by their definition: 8 bytes per slot handed out (the key) + 512 per live block of the
box (the types) + 3 x 64 for the three faces beyond it; the fraction is of the 8 TB/s HBM peak."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

CALLS, WARM = 20, 5
PEAK = 8.0e12


def host_bfs(grid, src, min_free=1):
    """steps over the 6-connected cells with at least min_free FREE or FNT voxels, by dilation of boolean planes"""
    g = grid.astype(np.int64)
    node = ((g >> 31) & 1).astype(bool) & (((g & 0x3ff) + ((g >> 20) & 0x3ff)) >= min_free)
    steps = np.full(grid.shape, -1, np.int32)
    f = np.zeros(grid.shape, bool)
    if node[src]:
        f[src] = True
    seen = f.copy()
    level = 0
    while f.any():
        steps[f] = level
        d = np.zeros_like(f)
        d[1:] |= f[:-1]; d[:-1] |= f[1:]
        d[:, 1:] |= f[:, :-1]; d[:, :-1] |= f[:, 1:]
        d[:, :, 1:] |= f[:, :, :-1]; d[:, :, :-1] |= f[:, :, 1:]
        f = d & node & ~seen
        seen |= f
        level += 1
    return steps


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

    rec, count = m.blocks_summary(min_fnt=1)
    allrec, nall = m.blocks_summary()
    lo, hi = allrec["key"].min(0).astype(np.int64), allrec["key"].max(0).astype(np.int64)
    pv = np.array(m.pivot(), np.int64)
    robot_vox = pv + np.array(size) // 2
    robot = (robot_vox.astype(np.float32) * np.float32(w)).astype(np.float32)
    rb = robot_vox >> 3
    # the LDS box: at most 64 x 48 x 64 cells around the robot's block, inside the data's box
    half = np.array([32, 24, 32])
    llo = np.maximum(lo, rb - half)
    lhi = np.minimum(hi, llo + 2 * half - 1)
    say(f"workload  c5 hash world {size[0]}^3, voxel {w} m, pool {cfg.max_blocks} slots, {handed} handed out after {a.updates} updates; "
        f"{nall} blocks with a known voxel, {count} of them with FNT voxels")
    v = rec["fnt_voxel"].astype(np.int64)
    fpos = ((rec["key"].astype(np.int64) * 8 + np.stack([v >> 6, (v >> 3) & 7, v & 7], -1)).astype(np.float32) * np.float32(w)).astype(np.float32)
    dgoal = torch.from_numpy(robot.reshape(1, 3)).to(dev)
    dpos = torch.from_numpy(fpos).to(dev)
    dsteps = torch.empty((max(count, 1),), dtype=torch.int32, device=dev)
    for name, blo, bhi in (("data box", lo, hi), ("cut box", llo, lhi)):
        blo, bhi = tuple(int(x) for x in blo), tuple(int(x) for x in bhi)
        n = [bhi[k] - blo[k] + 1 for k in range(3)]
        cells, words = n[0] * n[1] * n[2], (n[0] + 63) // 64 * n[1] * n[2]
        form = "all six planes in LDS" if words <= 3072 else "next in LDS, five planes in global memory"
        info = m.routes_compute(blo, bhi, [tuple(robot)])
        finfo = m.routes_compute(blo, bhi, (), from_frontiers=True)
        say(f"--- {name}: {n[0]} x {n[1]} x {n[2]} cells, {words} words a plane ({form}); {info['n_nodes']} nodes, {info['n_links']} links, "
            f"{info['n_frontier']} frontier blocks; from the robot {info['n_reached']} reached, max_steps {info['max_steps']}; from the frontier blocks "
            f"{finfo['n_reached']} reached, max_steps {finfo['max_steps']}")
        dgrid = torch.empty((cells,), dtype=torch.int32, device=dev)
        us = {}
        us["grid"] = timed(lambda: m.blocks_summary_dev(0, 0, dgrid.data_ptr(), blo, bhi))
        us["nosource"] = timed(lambda: m.routes_compute_dev(0, 0, blo, bhi))
        us["robot"] = timed(lambda: m.routes_compute_dev(dgoal.data_ptr(), 1, blo, bhi))
        us["frontier"] = timed(lambda: m.routes_compute_dev(0, 0, blo, bhi, from_frontiers=True))
        m.routes_compute(blo, bhi, [tuple(robot)])
        us["query"] = timed(lambda: m.routes_query_dev(dpos.data_ptr(), count, dsteps.data_ptr()))
        nbytes = 8 * handed + (512 + 192) * int(info["n_nodes"])
        gbytes = 8 * handed + 512 * int(info["n_nodes"]) + 4 * cells
        say(f"grid      {us['grid']:8.1f} us per call; {gbytes / 1e6:8.1f} MB = {gbytes / (us['grid'] * 1e-6) / PEAK:5.3f} of the 8 TB/s peak")
        say(f"nosource  {us['nosource']:8.1f} us per call; {nbytes / 1e6:8.1f} MB = {nbytes / (us['nosource'] * 1e-6) / PEAK:5.3f} of the 8 TB/s peak; "
            f"nosource / grid {us['nosource'] / us['grid']:.2f}")
        lv = max(int(info["max_steps"]), 1)
        say(f"robot     {us['robot']:8.1f} us per call; {int(info['max_steps'])} levels: {(us['robot'] - us['nosource']) / lv:6.2f} us a level")
        flv = max(int(finfo["max_steps"]), 1)
        say(f"frontier  {us['frontier']:8.1f} us per call; {int(finfo['max_steps'])} levels: {(us['frontier'] - us['nosource']) / flv:6.2f} us a level")
        say(f"query     {us['query']:8.1f} us per call; {count} points")
        # the route replaced, wall clock
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            _, _, grid = m.blocks_summary(blo, bhi, max_records=0, grid=True)
            t.append(time.perf_counter() - t0)
        src = tuple(int(rb[k] - blo[k]) for k in (2, 1, 0))
        t0 = time.perf_counter()
        hsteps = host_bfs(grid, src)
        tb = time.perf_counter() - t0
        dsteps_h, _ = m.routes_read()
        say(f"host      grid to the host {min(t) * 1e6:8.1f} us, numpy BFS on it {tb * 1e6:8.1f} us ({int((hsteps >= 0).sum())} cells reached without face links, "
            f"{int((dsteps_h >= 0).sum())} with them); (grid + BFS) / robot {(min(t) + tb) * 1e6 / us['robot']:.0f}")
    m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# python tools/routes_time.py   (MI355X; device events on the mapper's stream around %d calls after %d warm-up calls)\n" % (CALLS, WARM))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

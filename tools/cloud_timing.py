#!/usr/bin/env python3
"""What the display clouds cost on an MI355X, beside what the same display costs through the CPU mirror.

  python tools/cloud_timing.py [--out profiles/r17_cloud_timing.txt]

The headline workload as bench.py builds it (BASELINE config 5: the hash world at 512^3, bench's pool, wave grid and placement
draws; its helpers are imported, bench.py itself is not touched).
 (a) after a steady-state update with the stream off, each of the reference's four clouds (include/gie.h "display clouds") through
     the _dev forms into a device buffer of exactly its size: device time from the "cloud" entry of gie_profile_read over 20
     calls, and stream time (device events around 20 calls enqueued back to back, profile off), which holds the memset of the counter
     and the gaps between the launches too.  Beside them the host form (count, then fetch: two calls and the copy back).
 (b) the price of the mirror: ms per update with gie_stream_enable(1) minus ms per update with it off, plus the drain
     (gie_stream_changed of every flagged block into host memory) — what a node pays today to have anything to build the global
     clouds from, before its host loops over the mirrored blocks."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gie-mapping_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help="cube side (default: the preset's 512)")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--vis-height", type=float, default=1.0)
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
    w, U, W = pre["voxel"], a.updates, 5
    total = W + 3 * U + 4
    cfg = gie.make_config(w, size, cutoff_dist=pre["cutoff"], fast_mode=pre["fast"], max_blocks=bench.pool_blocks("c5", size, total),
                          wave_workgroups=bench.WAVE_GRID["wgs"], place_tries=bench.PLACE_TRIES)
    m = gie.Mapper(cfg)
    feed = bench.HashWorldFeed(torch, scenes, dev, w, size, (0, 0, 0))
    feed.prepare(0, total)
    st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
    nxt = [0]

    def updates(n, after=None):
        """ms per update over n updates (device events on the mapper's stream); after(): called behind every update, outside the window"""
        ms = 0.0
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            feed.step_input(m, nxt[0])
            e0.record(st)
            m.step()
            e1.record(st)
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            nxt[0] += 1
            if after:
                after()
        return ms / n

    updates(W)
    off = updates(U)
    say(f"workload  c5 hash world {size[0]}^3, voxel {w} m, pool {cfg.max_blocks} blocks ({m.stats()['blocks_total']} live); "
        f"map update, stream off: {off:.3f} ms per update ({U} updates after {W})")

    # ---- (a) the four clouds, stream off
    slice_z = scenes.pos2coord(a.vis_height, w)
    occ, known = 1 << gie.VOX_OCCUPIED, (1 << gie.VOX_FREE) | (1 << gie.VOX_OCCUPIED) | (1 << gie.VOX_FNT)
    clouds = [("local OGM", m.cloud_local, m.cloud_local_dev, (occ, gie.CLOUD_TYPE, None, None)),
              ("local EDT", m.cloud_local, m.cloud_local_dev, (known, gie.CLOUD_DIST, None, None)),
              ("global OGM", m.cloud_global, m.cloud_global_dev, (occ, gie.CLOUD_TYPE, None, None)),
              ("global EDT", m.cloud_global, m.cloud_global_dev, (known, gie.CLOUD_DIST, slice_z, slice_z))]
    dcnt = torch.zeros(4, dtype=torch.int32, device=dev)
    dev_ms = {}
    for name, host, fdev, args in clouds:
        _, count = host(*args, max_points=0)
        dout = torch.empty((max(count, 1), 4), dtype=torch.float32, device=dev)
        run = lambda: fdev(dout.data_ptr(), dcnt.data_ptr(), *args, max_points=count)      # noqa: E731
        for _ in range(3):
            run()
        m.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(20):
            run()
        e1.record(st)
        e1.synchronize()
        stream_ms = e0.elapsed_time(e1) / 20
        m.profile_enable(True)
        m.profile_read()
        for _ in range(20):
            run()
        tot, n = m.profile_read()["cloud"]
        m.profile_enable(False)
        assert n == 20 and int(dcnt.cpu()[0]) == count
        t0 = time.perf_counter()
        pts, c2 = host(*args)
        host_ms = (time.perf_counter() - t0) * 1e3
        assert c2 == count == len(pts)
        dev_ms[name] = tot / n
        say(f"(a) {name:10s} {count:10d} points ({16 * count / 1e6:8.1f} MB of records): device {tot / n * 1e3:8.1f} us per call, "
            f"{stream_ms * 1e3:8.1f} us on the stream; host form (count + fetch) {host_ms:8.2f} ms")
        del dout, pts

    # ---- (b) the same display through the mirror: the stream on, every update drained
    m.stream_enable(True)
    keys = blocks = None
    drain = []

    def drain_all():
        nonlocal keys, blocks
        n = m.stream_count()
        if keys is None or len(keys) < n:
            keys, blocks = np.empty((n, 3), np.int32), np.empty((n, 512), gie.mapper.VOXEL_DTYPE)
        got = C.c_int32(0)
        t0 = time.perf_counter()
        if n:
            m._chk(m._f["stream_changed"](m._h, keys.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p), n, C.byref(got)))
        m.sync()
        drain.append(((time.perf_counter() - t0) * 1e3, n))

    updates(2, drain_all)                                      # the switch of kernel order and the first drain (every block of the map)
    drain.clear()
    on = updates(U, drain_all)
    dms, dn = np.mean([d[0] for d in drain]), np.mean([d[1] for d in drain])
    price = on - off + dms
    say(f"(b) mirror: map update, stream on: {on:.3f} ms per update (+{on - off:.3f} ms); drain of {dn:.0f} flagged blocks per update "
        f"({dn * 512 * 20 / 1e6:.0f} MB): {dms:.2f} ms; price of the display per update: {price:.2f} ms, before the host loops")
    both = dev_ms["global OGM"] + dev_ms["global EDT"]
    say(f"    the two global clouds on the device: {both * 1e3:.1f} us per display = 1 / {price / both:.0f} of (b); "
        f"all four: {sum(dev_ms.values()) * 1e3:.1f} us")
    m.stream_enable(False)
    updates(2)
    again = updates(U)
    say(f"    map update, stream off again: {again:.3f} ms per update")
    m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/cloud_timing.py   (MI355X; device events on the mapper's stream, gie_profile_read for the kernels)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

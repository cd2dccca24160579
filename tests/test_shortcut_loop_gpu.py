"""The planner's chain with the shortcut in its place, on the device: frontier clusters -> goals -> NF1 -> descent paths -> opaque
plane -> waypoints -> signed distance at the waypoints, every step enqueued on the mapper's stream through the _dev forms with one
sync per update, over 6 updates of the drive of tests/test_planner_loop_gpu.py.  The path buffers go from gie_nf1_path_dev to
gie_path_shortcut_dev and the waypoints from there to gie_query_sdf_dev without leaving the device.  Every output is compared with
the CPU references on one read_local taken after the sync: bytes, and the signed distance as tests/test_sdf_gpu.py compares it."""
import numpy as np
import pytest

import frontier_ref as fr
import los_ref as lr
import nf1_ref
import path_ref as pr
import sdf_ref
import test_planner_loop_gpu as pl
from gie import scenes
from stage_common import bits, mapper, update

pytestmark = pytest.mark.gpu

UPDATES = 6
LOOKAHEAD = 48
MAX_WP = 10


def _reference(loc, pvt, w):
    ty, edt = loc["type"], loc["edt"]
    c = np.float32(pl.CLEARANCE) / np.float32(w)
    cl = fr.clusters(fr.members(ty, edt, c), 26, pl.MIN_SIZE, pl.CAP, pvt, w)
    f, _, src = nf1_ref.field(ty, edt, c, 0, cl["goals"], w, pvt)
    pts, lens = nf1_ref.paths(f, pl.start_points(pvt, w), w, pvt, pl.MAX_LEN)
    path = np.zeros((pl.N_STARTS, pl.MAX_LEN, 3), np.int32)
    for i, p in enumerate(pts):
        path[i, :len(p)] = p
    opq = lr.opaque(ty, edt, c, 0)
    legs = []
    wp, info = pr.shortcut(edt, opq, path, lens, pvt, LOOKAHEAD, MAX_WP, legs=legs)
    xyz = (wp["xyz"].reshape(-1, 3).astype(np.float32) * np.float32(w)).astype(np.float32)
    return dict(goals=cl["goals"], n_clusters=cl["n_clusters"], n_sources=int(src.sum()), path=path, lens=lens, n_opaque=int(opq.sum()),
                wp=wp, info=info, legs=legs, xyz=xyz)


def _dev_chain(m, torch, st, dev, pvt, w):
    t = {}
    with torch.cuda.stream(st):
        t["goals"] = torch.zeros((pl.CAP, 3), dtype=torch.float32, device=dev)
        t["counts"] = torch.full((2,), -7, dtype=torch.int32, device=dev)
        m.frontier_compute_dev(pl.CLEARANCE, pl.MIN_SIZE, 26, pl.CAP, t["counts"].data_ptr())
        m.read_frontier_clusters_dev(0, t["goals"].data_ptr(), 0)
        t["n_sources"] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        m.nf1_compute_dev(t["goals"].data_ptr(), pl.CAP, pl.CLEARANCE, d_n_sources=t["n_sources"].data_ptr())
        starts = torch.from_numpy(pl.start_points(pvt, w)).to(dev)
        t["path"] = torch.zeros((pl.N_STARTS, pl.MAX_LEN, 3), dtype=torch.int32, device=dev)
        t["lens"] = torch.zeros(pl.N_STARTS, dtype=torch.int32, device=dev)
        m.nf1_path_dev(starts.data_ptr(), pl.N_STARTS, pl.MAX_LEN, t["path"].data_ptr(), t["lens"].data_ptr())
        t["n_opaque"] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        m.los_prepare_dev(pl.CLEARANCE, 0, t["n_opaque"].data_ptr())
        t["wp"] = torch.zeros((pl.N_STARTS, MAX_WP, 6), dtype=torch.int32, device=dev)          # 24-byte records: xyz is words 0..2
        t["info"] = torch.zeros((pl.N_STARTS, 4), dtype=torch.int32, device=dev)
        m.path_shortcut_dev(t["path"].data_ptr(), t["lens"].data_ptr(), pl.N_STARTS, pl.MAX_LEN, t["wp"].data_ptr(), t["info"].data_ptr(),
                            LOOKAHEAD, MAX_WP)
        t["xyz"] = (t["wp"][:, :, :3].to(torch.float32) * w).reshape(-1, 3).contiguous()        # (zeros beyond a path's records)
        n = pl.N_STARTS * MAX_WP
        t["dist"] = torch.empty(n, dtype=torch.float32, device=dev)
        t["grad"] = torch.empty((n, 3), dtype=torch.float32, device=dev)
        t["flags"] = torch.empty(n, dtype=torch.uint8, device=dev)
        m.query_sdf_dev(t["xyz"].data_ptr(), n, t["dist"].data_ptr(), t["grad"].data_ptr(), t["flags"].data_ptr())
        t["keep"] = starts
    return t


def test_shortcut_in_the_planner_chain():
    import torch
    w = 0.1
    d = pl.loop_drive()
    m = mapper(pl.SIZE)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        shorter = long_legs = paths = 0
        for k in range(UPDATES):
            pos, q, lab = d.frame(k)
            update(m, pos, q, lab)
            pvt = scenes.local_pivot(pos, w, pl.SIZE)
            t = _dev_chain(m, torch, st, dev, pvt, w)
            m.sync()                                                      # the one sync of the update
            assert tuple(m.pivot()) == tuple(pvt)
            loc = m.read_local()
            g = {key: v.cpu().numpy() for key, v in t.items() if key != "keep"}
            ref = _reference(loc, pvt, w)
            assert int(g["counts"][0]) == ref["n_clusters"] and np.array_equal(bits(g["goals"]), bits(ref["goals"])), k
            assert int(g["n_sources"][0]) == ref["n_sources"] and int(g["n_opaque"][0]) == ref["n_opaque"], k
            assert np.array_equal(g["lens"], ref["lens"]) and g["path"].tobytes() == ref["path"].tobytes(), k
            # the waypoints: every byte, also of the records that were not written
            assert g["wp"].tobytes() == ref["wp"].tobytes() and g["info"].tobytes() == ref["info"].tobytes(), k
            # the signed distance at them, as tests/test_sdf_gpu.py: the plane against the reference, the queries against the
            # interpolant of the plane
            assert g["xyz"].tobytes() == ref["xyz"].tobytes(), k
            r = m.read_sdf()
            ids = sdf_ref.inside_dist_sq(loc["type"])
            assert np.array_equal(r["inside_dist_sq"], ids), k
            assert np.allclose(r["sdf"], sdf_ref.sdf(ids, loc["edt"], pl.SIZE), rtol=1e-6, atol=0), k
            rd, rg, rf = sdf_ref.query(r["sdf"], loc["type"], pl.SIZE, pvt, w, ref["xyz"])
            assert np.array_equal(g["flags"], rf) and np.array_equal(np.isnan(g["dist"]), np.isnan(rd)), k
            ok = ~np.isnan(rd)
            assert np.allclose(g["dist"][ok], rd[ok], rtol=1e-5, atol=1e-5) and np.allclose(g["grad"], rg, rtol=1e-5, atol=1e-5), k
            # a clear leg keeps the plane's clearance: its min_edt is not below it
            info, wp = ref["info"], ref["wp"]
            ms = np.clip(ref["lens"], 0, pl.MAX_LEN)
            for i in range(pl.N_STARTS):
                rec = wp[i, 1:min(int(info["count"][i]), MAX_WP)]
                assert (rec["min_edt"][rec["forced"] == 0] >= np.float32(pl.CLEARANCE) / np.float32(w)).all(), (k, i)
            paths += int((ms > 0).sum())
            shorter += int(((info["count"] * 2 < ms) & (ms > 0)).sum())
            long_legs += sum(int(np.flatnonzero(c)[-1]) + 1 >= 8 for win in ref["legs"] for _, _, c in win if c.any())
        # the drive gives the chain something to do: paths, most of them much shorter as waypoints, legs over many points
        print("shortcut loop: paths %d, of them with fewer than half as many waypoints as points %d, legs over 8 points or more %d" % (paths, shorter, long_legs))
        assert paths >= 16 and shorter >= 4 and long_legs >= 4, (paths, shorter, long_legs)
    finally:
        m.close()

"""The loop a planner runs at every map update, on the device: frontier clusters -> goals -> NF1 -> descent paths -> opaque plane ->
shortcut segments between path points -> view gain at the cluster goals -> signed distance at the path points, every step
enqueued on the mapper's stream through the _dev forms with no host synchronisation in between, over a drive of 12 updates.
The stages share the stream, the device allocations, the two scratch slots of the host forms and (through NF1) the grid
barrier; each has its own tests, this one runs them back to back.  Every output is compared with the CPU references
(frontier_ref, nf1_ref, los_ref, sdf_ref) on one read_local taken after the single sync, by each stage's own standard: bytes, and
the signed distance queries as tests/test_sdf_gpu.py compares them.  Also: update k's path fed to update k + 1's opaque plane
(another pivot), a twin mapper that runs none of the loop, and the host forms in the same order at update 6."""
import numpy as np
import pytest

import frontier_ref as fr
import gie
import los_ref as lr
import nf1_ref
import sdf_ref
from gie import scenes
from stage_common import BoxDrive, bits, cv, mapper, probe, update

pytestmark = pytest.mark.gpu

SIZE = (80, 72, 64)
UPDATES = 12
CAP = 12                        # clusters kept = goals = views
MIN_SIZE = 3
CLEARANCE = 0.15                # metres: frontier members, NF1 and the opaque plane alike (a shortcut has to keep the path's clearance)
N_STARTS = 16
MAX_LEN = 64
STRIDE = 8                      # a shortcut from a path's first point to its points 8, 16, 24 ...
GAIN = (0.0, 1.2, 0.7)          # r_min, r_max (metres), tan2_elev
HOST_AT = 6


UNSEEN = [((20, -15, -8), 3), ((30, 12, 9), 3), ((24, 14, -14), 4), ((34, -18, 6), 3)]        # (low corner in global voxels, side)
DELTA = 5                       # voxels per update: the plane x = 4 of one update (the frontier of the never-seen slab) has left the next


class LoopDrive(BoxDrive):
    """the box drive with never-seen blocks fixed in the world, inside the volume at every update of the drive and never labelled:
    their shells are frontier clusters of their own beside the slab's (which alone is one component)"""

    def frame(self, k):
        pos, q, lab = super().frame(k)
        pvt = scenes.local_pivot(pos, self.w, self.size)
        for lo, side in UNSEEN:
            x, y, z = (int(c) - int(p) for c, p in zip(lo, pvt))
            assert min(x, y, z) >= 4 and all(c + side <= s for c, s in zip((x, y, z), self.size))
            blk = lab[z:z + side, y:y + side, x:x + side]
            blk[blk == 1] = 0
        return pos, q, lab


def loop_drive():
    return LoopDrive(SIZE, seed=4, delta=DELTA)


def start_points(pvt, w):
    """16 world points around the robot (the middle of the volume): a 4 x 4 grid across y and z, five voxels apart"""
    c = np.array(SIZE) // 2
    v = np.array([(c[0] + (i + j) % 3, c[1] + 5 * (i - 2) + 2, c[2] + 5 * (j - 2) + 2) for i in range(4) for j in range(4)], np.float32)
    return ((v + np.asarray(pvt, np.float32)) * np.float32(w)).astype(np.float32)


def shortcut_points(path, w):
    """(a, b) world points [n * k, 3] float32 of the shortcuts along a path buffer [n, MAX_LEN, 3] int32 of global voxels: from each
    path's first point to its points STRIDE, 2 * STRIDE ... (zeros beyond a path's length: whatever voxel that is)"""
    idx = np.arange(STRIDE, MAX_LEN, STRIDE)
    b = path[:, idx, :].astype(np.float32) * np.float32(w)
    a = np.broadcast_to(path[:, :1, :].astype(np.float32) * np.float32(w), b.shape)
    return np.ascontiguousarray(a).reshape(-1, 3), np.ascontiguousarray(b).reshape(-1, 3)


def loop_reference(loc, pvt, w, old_path=None):
    """the whole loop on read_local's planes at pivot pvt, by the CPU references: a dict of what the device must give"""
    ty, edt = loc["type"], loc["edt"]
    c = np.float32(CLEARANCE) / np.float32(w)
    cl = fr.clusters(fr.members(ty, edt, c), 26, MIN_SIZE, CAP, pvt, w)
    f, trav, src = nf1_ref.field(ty, edt, c, 0, cl["goals"], w, pvt)
    starts = start_points(pvt, w)
    pts, lens = nf1_ref.paths(f, starts, w, pvt, MAX_LEN)
    path = np.zeros((N_STARTS, MAX_LEN, 3), np.int32)
    for i, p in enumerate(pts):
        path[i, :len(p)] = p
    opq = lr.opaque(ty, edt, c, 0)
    a, b = shortcut_points(path, w)
    out = dict(goals=cl["goals"], n_clusters=cl["n_clusters"], n_sources=int(src.sum()), path=path, lens=lens, n_opaque=int(opq.sum()),
               seg_a=a, seg_b=b, seg=lr.segments(edt, opq, a, b, w, pvt),
               gain=lr.view_gain(ty, opq, gie.make_views(cl["goals"]), GAIN[0], GAIN[1], GAIN[2], w, pvt),
               xyz=(path.reshape(-1, 3).astype(np.float32) * np.float32(w)).astype(np.float32))
    if old_path is not None:
        oa, ob = shortcut_points(old_path, w)
        out["old_seg"] = lr.segments(edt, opq, oa, ob, w, pvt)
    return out


def drive_properties(refs):
    """what the drive has to give the loop, from the references of its updates"""
    idx = np.arange(STRIDE, MAX_LEN, STRIDE)
    clear = blocked = 0
    for r in refs:
        real = (r["lens"][:, None] > idx[None, :]).reshape(-1)              # shortcuts to points the path has
        clear += int((r["seg"]["first"][real] == -1).sum())
        blocked += int((r["seg"]["first"][real] >= 0).sum())
    return dict(two_clusters=sum(r["n_clusters"] >= 2 for r in refs), long_path=sum(int(r["lens"].max()) >= 25 for r in refs),
                clear=clear, blocked=blocked)


def _dev_loop(m, torch, st, dev, pvt, w, old_path):
    """steps 1-8 through the _dev forms on the mapper's stream, no host wait; the tensors of the results"""
    t = {}
    with torch.cuda.stream(st):
        t["goals"] = torch.zeros((CAP, 3), dtype=torch.float32, device=dev)
        t["counts"] = torch.full((2,), -7, dtype=torch.int32, device=dev)
        m.frontier_compute_dev(CLEARANCE, MIN_SIZE, 26, CAP, t["counts"].data_ptr())
        m.read_frontier_clusters_dev(0, t["goals"].data_ptr(), 0)
        t["n_sources"] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        m.nf1_compute_dev(t["goals"].data_ptr(), CAP, CLEARANCE, d_n_sources=t["n_sources"].data_ptr())
        starts = torch.from_numpy(start_points(pvt, w)).to(dev)
        t["path"] = torch.zeros((N_STARTS, MAX_LEN, 3), dtype=torch.int32, device=dev)
        t["lens"] = torch.zeros(N_STARTS, dtype=torch.int32, device=dev)
        m.nf1_path_dev(starts.data_ptr(), N_STARTS, MAX_LEN, t["path"].data_ptr(), t["lens"].data_ptr())
        t["n_opaque"] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        m.los_prepare_dev(CLEARANCE, 0, t["n_opaque"].data_ptr())

        def shortcuts(path):
            world = path.to(torch.float32) * w                            # global voxels -> world floats, on the device
            b = world[:, STRIDE::STRIDE, :].contiguous()
            a = world[:, :1, :].expand_as(b).contiguous()
            hits = torch.zeros(b.shape[0] * b.shape[1] * 24, dtype=torch.uint8, device=dev)
            m.los_segments_dev(a.data_ptr(), b.data_ptr(), b.shape[0] * b.shape[1], hits.data_ptr())
            return a, b, hits
        t["seg_a"], t["seg_b"], t["seg"] = shortcuts(t["path"])
        if old_path is not None:
            _, _, t["old_seg"] = shortcuts(old_path)
        views = torch.zeros((CAP, 16), dtype=torch.float32, device=dev)
        views[:, :3] = t["goals"]
        t["gain"] = torch.full((CAP, 4), -7, dtype=torch.int32, device=dev)
        m.view_gain_dev(views.data_ptr(), CAP, t["gain"].data_ptr(), *GAIN)
        t["xyz"] = (t["path"].to(torch.float32) * w).reshape(-1, 3).contiguous()
        n = N_STARTS * MAX_LEN
        t["dist"] = torch.empty(n, dtype=torch.float32, device=dev)
        t["grad"] = torch.empty((n, 3), dtype=torch.float32, device=dev)
        t["flags"] = torch.empty(n, dtype=torch.uint8, device=dev)
        m.query_sdf_dev(t["xyz"].data_ptr(), n, t["dist"].data_ptr(), t["grad"].data_ptr(), t["flags"].data_ptr())
        t["keep"] = (starts, views)                                       # (alive until the sync)
    return t


def _host_loop(m, pvt, w):
    """the same steps in the same order through the host forms: back to back over the two scratch slots"""
    h = {}
    nc, _ = m.frontier_compute(CLEARANCE, MIN_SIZE, 26, CAP)
    _, h["goals"], _ = m.read_frontier_clusters()
    h["n_sources"] = m.nf1_compute(h["goals"], CLEARANCE)
    pts, h["lens"] = m.nf1_path(start_points(pvt, w), MAX_LEN)
    h["path"] = np.zeros((N_STARTS, MAX_LEN, 3), np.int32)
    for i, p in enumerate(pts):
        h["path"][i, :len(p)] = p
    h["n_opaque"] = m.los_prepare(CLEARANCE, 0)
    a, b = shortcut_points(h["path"], w)
    h["seg"] = m.los_segments(a, b)
    h["gain"] = m.view_gain(gie.make_views(h["goals"]), *GAIN)
    xyz = (h["path"].reshape(-1, 3).astype(np.float32) * np.float32(w)).astype(np.float32)
    h["dist"], h["grad"], h["flags"] = m.query_sdf(xyz)
    h["n_clusters"] = nc
    return h


def test_planner_loop_over_a_drive():
    import torch
    w = 0.1
    d = loop_drive()
    m, twin = mapper(SIZE), mapper(SIZE)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        refs, old_path, crossed = [], None, 0
        for k in range(UPDATES):
            pos, q, lab = d.frame(k)
            for mm in (m, twin):
                update(mm, pos, q, lab)
            pvt = scenes.local_pivot(pos, w, SIZE)
            t = _dev_loop(m, torch, st, dev, pvt, w, old_path)
            m.sync()                                                      # the one sync of the update
            assert tuple(m.pivot()) == tuple(pvt)
            loc = m.read_local()
            g = {key: v.cpu().numpy() for key, v in t.items() if key != "keep"}
            ref = loop_reference(loc, pvt, w, None if old_path is None else old_path.cpu().numpy())
            refs.append(ref)
            # 1-3: clusters -> goals -> field
            assert int(g["counts"][0]) == ref["n_clusters"] and np.array_equal(bits(g["goals"]), bits(ref["goals"])), k
            assert int(g["n_sources"][0]) == ref["n_sources"], k
            # 4: paths (points beyond a path's length stay as the buffer was: zeros)
            assert np.array_equal(g["lens"], ref["lens"]) and g["path"].tobytes() == ref["path"].tobytes(), k
            # 5-6: the plane and the shortcuts; torch's int32 -> float32 -> * w is the CPU's
            assert int(g["n_opaque"][0]) == ref["n_opaque"], k
            assert g["seg_a"].tobytes() == ref["seg_a"].tobytes() and g["seg_b"].tobytes() == ref["seg_b"].tobytes(), k
            assert g["seg"].tobytes() == ref["seg"].tobytes(), k
            # 7: the gain at the goals (-1 beyond the clusters)
            assert g["gain"].tobytes() == ref["gain"].tobytes(), k
            # 8: the signed distance at the path points, as tests/test_sdf_gpu.py: the plane against the reference, the queries
            # against the interpolant of the plane
            r = m.read_sdf()
            ids = sdf_ref.inside_dist_sq(loc["type"])
            assert np.array_equal(r["inside_dist_sq"], ids), k
            assert np.allclose(r["sdf"], sdf_ref.sdf(ids, loc["edt"], SIZE), rtol=1e-6, atol=0), k
            assert g["xyz"].tobytes() == ref["xyz"].tobytes(), k
            rd, rg, rf = sdf_ref.query(r["sdf"], loc["type"], SIZE, pvt, w, ref["xyz"])
            assert np.array_equal(g["flags"], rf) and np.array_equal(np.isnan(g["dist"]), np.isnan(rd)), k
            ok = ~np.isnan(rd)
            assert np.allclose(g["dist"][ok], rd[ok], rtol=1e-5, atol=1e-5) and np.allclose(g["grad"], rg, rtol=1e-5, atol=1e-5), k
            # update k - 1's path on this update's plane, at this update's pivot: the same world points, some now outside
            if old_path is not None:
                assert g["old_seg"].tobytes() == ref["old_seg"].tobytes(), k
                crossed += int((ref["old_seg"]["first"] == -2).sum())
            old_path = t["path"]
            # the host forms, once: the same outputs byte for byte
            if k == HOST_AT:
                h = _host_loop(m, pvt, w)
                assert h["n_clusters"] == ref["n_clusters"] and h["n_sources"] == ref["n_sources"] and h["n_opaque"] == ref["n_opaque"]
                for key in ("goals", "lens", "path", "seg", "gain", "dist", "grad", "flags"):
                    assert bits(h[key]).tobytes() == bits(g[key]).tobytes(), key
            # the twin that ran none of it: the same maps, stats and global map
            lt = twin.read_local()
            for key in loc:
                assert np.array_equal(loc[key], lt[key]), (k, key)
            assert m.stats() == twin.stats(), k
            assert np.array_equal(probe(m, SIZE, np.random.default_rng(k)), probe(twin, SIZE, np.random.default_rng(k))), k
        p = drive_properties(refs)
        assert p["two_clusters"] >= 8 and p["long_path"] >= 8 and p["clear"] >= 1 and p["blocked"] >= 1, p
        assert crossed >= 1, crossed                                      # old path points that left the volume: first == -2
        assert cv(m, CLEARANCE) > 1
    finally:
        m.close()
        twin.close()

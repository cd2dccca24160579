"""Global block routes on the device (include/gie.h "global block routes", gie_routes.inc.h) against the numpy reference of
tests/routes_ref.py over Mapper.query_global.  Every comparison is exact: cell bytes and info by bytes, field, gather and paths by
array_equal.

Which form of the propagation a box takes is decided by its size alone (no hook reports it): up to 3072 words of 64 cells a plane —
every box around the data of these scenes — all six bit planes lie in LDS; above that, up to 16384 words, five of them stay in global
memory (the padded boxes of test_both_forms_of_the_propagation)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import blocks_ref as B
import gie
import routes_ref as R
from gie import scenes
from stage_common import BoxDrive, W, build_host_probe, lidar_frames, mapper, scene, stage_calls_change_nothing, update

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # GIE_ERR_INVALID
FILL = 0x5a


def block_points(keys, at=3, w=W):
    """a world point inside each block: voxel key * 8 + at, coord2pos in fp32"""
    return ((np.asarray(keys, np.int64).reshape(-1, 3) * 8 + at).astype(np.float32) * np.float32(w)).astype(np.float32)


def run(tag, m, ref, lo, hi, goals=(), min_free=1, min_open=1, min_fnt=1, from_frontiers=False):
    """one compute against the reference of the checkpoint: cell bytes, field and info -> the reference's graph"""
    lo, hi = tuple(int(v) for v in lo), tuple(int(v) for v in hi)
    g = R.Graph(ref.table, lo, hi, min_free, min_open, min_fnt)
    gb, ok = R.point_blocks(np.asarray(goals, np.float32).reshape(-1, 3), m.cfg.voxel_width)
    g.solve(gb, ok, R.FROM_FRONTIERS if from_frontiers else 0)
    info = m.routes_compute(lo, hi, goals, min_free, min_open, min_fnt, from_frontiers)
    steps, cells = m.routes_read()
    assert cells.shape == g.cells.shape and cells.tobytes() == g.cells.tobytes(), tag
    assert np.array_equal(steps, g.steps), tag
    assert info.tobytes() == g.info.tobytes(), (tag, info, g.info)
    return g


def check_points(tag, m, g, rng, n=300, max_len=4):
    """the gather at n points inside and outside the box, on nodes and not, and the descents from every frontier block"""
    w = m.cfg.voxel_width                                        # (the deferred-record drive has its own)
    lo, hi = (g.lo - 2) * 8 * w, (g.hi + 3) * 8 * w
    nz, ny, nx = np.nonzero(g.node)
    on = np.stack([nx, ny, nz], -1)[::max(len(nx) // 64, 1)] + g.lo           # some sixty points on nodes for certain
    pts = np.concatenate([block_points(on, rng.integers(0, 8, 3), w), rng.uniform(lo, hi, (n, 3)).astype(np.float32)])
    pts[-1, 1] = np.nan
    pts[-2, 0] = np.inf
    want = g.query(pts, w)
    assert np.array_equal(m.routes_query(pts), want), tag
    fz, fy, fx = np.nonzero(g.frontier)
    starts = np.concatenate([block_points(np.stack([fx, fy, fz], -1) + g.lo, w=w), pts[-8:]])
    path, ln = m.routes_path(starts, max_len, path=np.full((len(starts), max_len, 3), -7, np.int32))
    wpath, wln = g.path(starts, w, max_len, fill=-7)
    assert np.array_equal(ln, wln) and np.array_equal(path, wpath), tag
    return ln


def cut_and_unreached(g):
    """(node pairs next to each other without a link, nodes without a route)"""
    n = g.node
    cut = (n[:, :, :-1] & n[:, :, 1:] & ~g.link[0][:, :, :-1]).sum() + (n[:, :-1] & n[:, 1:] & ~g.link[1][:, :-1]).sum() + (n[:-1] & n[1:] & ~g.link[2][:-1]).sum()
    return int(cut), int((n & (g.steps < 0)).sum())


def three_boxes(ref):
    """around the data, cutting it, wider than it"""
    blo, bhi = [int(v) for v in ref.blo], [int(v) for v in ref.bhi]
    cut_lo = (blo[0] + 2, blo[1] + 1, blo[2] + 1)
    cut_hi = (max(bhi[0] - 3, cut_lo[0]), max(bhi[1] - 1, cut_lo[1]), bhi[2])
    return [(tuple(blo), tuple(bhi)), (cut_lo, cut_hi), (tuple(v - 2 for v in blo), tuple(v + 3 for v in bhi))]


def check_all(tag, m, ref, pos, rng, boxes=None, min_frees=(1, 200), min_opens=(1, 9, 64)):
    """both source modes, the boxes, min_free and min_open of one checkpoint -> (cut links, unreached nodes, longest path) seen"""
    cut = unreached = longest = 0
    for bi, (lo, hi) in enumerate(three_boxes(ref) if boxes is None else boxes):
        for min_free in min_frees:
            for min_open in min_opens:
                for ff in (False, True):
                    goals = [tuple(pos)] if not ff else [tuple(pos), (1.0e4, 0.0, 0.0), (float("nan"), 0.0, 0.0)]
                    t = (tag, bi, min_free, min_open, ff)
                    g = run(t, m, ref, lo, hi, goals, min_free, min_open, 1 if ff else 3, ff)
                    ln = check_points(t, m, g, rng)
                    c, u = cut_and_unreached(g)
                    cut, unreached, longest = cut + c, unreached + u, max(longest, int(ln.max()) if len(ln) else 0)
    return cut, unreached, longest


# ---------------------------------------------------------------------------------------------------------- 1. a drive
@pytest.mark.parametrize("size", [(48, 40, 33), (21, 19, 10)])
def test_routes_on_a_drive(size):
    d = BoxDrive(size)
    m = mapper(size)
    ref = B.GlobalRef(size)
    rng = np.random.default_rng(7)
    try:
        cut = unreached = longest = 0
        for k in range(20):
            pos, q, lab = d.frame(k)
            m.set_pose(pos, q)
            m.ogm_labels(lab)
            m.fuse()
            ref.add(m)
            seen = (0, 0, 0)
            if k == 12:                                          # between gie_fuse and gie_batch_edt, against query_global at the same point
                ref.take(m)
                seen = check_all(("after fuse", k), m, ref, pos, rng, boxes=three_boxes(ref)[:2], min_opens=(1, 9))
            m.batch_edt()
            m.merge()
            if k + 1 in (1, 9, 20):
                ref.take(m)
                seen = check_all(("merge", k), m, ref, pos, rng)
            cut, unreached, longest = cut + seen[0], unreached + seen[1], max(longest, seen[2])
        assert cut > 0 and unreached > 0, (cut, unreached)       # links are cut somewhere and some block has no route: otherwise this covers nothing
        assert longest > 4                                       # some descent is longer than its buffer
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. a door
def test_a_wall_on_a_block_face_with_a_door_of_one_voxel():
    size = (40, 24, 16)
    m = mapper(size)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        pvt = np.array(scenes.local_pivot(pos, W, size))
        gx = np.arange(size[0]) + pvt[0]
        wall = int(np.nonzero((gx & 7) == 7)[0][2])              # local x of the third plane of voxels at in-block coordinate 7: a block's +x face
        lab = np.ones(size[::-1], np.int8)
        lab[:, :, wall] = 2
        door = (5, 9)                                            # (z, y) of the door, local
        lab[door[0], door[1], wall] = 1
        for _ in range(2):
            update(m, pos, q, lab)
        assert np.array_equal(np.array(m.pivot()), pvt)
        ref = B.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        t = m.query_global((pvt + np.array([[wall, 3, 3], [wall, door[1], door[0]]])).astype(np.int32))["vox_type"]
        assert t[0] == R.OCCUPIED and t[1] in (R.FREE, R.FNT)
        wall_block = (pvt[0] + wall) >> 3
        door_block = np.array([wall_block, (pvt[1] + door[1]) >> 3, (pvt[2] + door[0]) >> 3])
        start = block_points([door_block - (1, 0, 0)])[0]        # the source: the block in front of the door's block
        lo, hi = ref.blo, ref.bhi
        g = run("door", m, ref, lo, hi, [tuple(start)])
        far = np.zeros(g.shape, bool)
        far[:, :, wall_block + 1 - int(lo[0]):] = True
        assert (g.node & far).sum() > 4 and (g.steps[g.node & far] > 0).all()         # every block behind the wall is reached ...
        c = lambda k: tuple(int(k[2 - i] - lo[2 - i]) for i in range(3))              # noqa: E731
        assert g.steps[c(door_block)] == 1 and g.steps[c(door_block + (1, 0, 0))] == 2                            # ... through the door
        beside = door_block + (0, 1 if door_block[1] + 1 <= hi[1] and g.node[c(door_block + (1, 1, 0))] else -1, 0)
        assert g.steps[c(beside - (1, 0, 0))] == 1 and g.steps[c(beside)] == 2 and g.steps[c(beside + (1, 0, 0))] == 3      # next to the source, but round through the door beyond the wall
        path, ln = m.routes_path(block_points([beside + (1, 0, 0)]), 8)
        assert ln[0] == 4 and path[0, 1].tolist() == (door_block + (1, 0, 0)).tolist() and path[0, 2].tolist() == door_block.tolist()
        check_points("door", m, g, np.random.default_rng(1))
        g = run("door, two pairs wanted", m, ref, lo, hi, [tuple(start)], min_open=2)
        assert (g.node & far).sum() > 4 and (g.steps[g.node & far] == -1).all() and (g.steps[g.node & ~far] >= 0).all()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. word carries
def test_links_across_the_words_of_a_row_and_a_box_one_cell_wide():
    size = (48, 40, 33)
    m = mapper(size)
    try:
        scene(m, size)
        ref = B.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        blo, bhi = [int(v) for v in ref.blo], [int(v) for v in ref.bhi]
        lo = (blo[0] + 4 - 64, blo[1], blo[2])                   # nx = 70: the data's blocks straddle cells 63 | 64 of every row
        hi = (lo[0] + 69, bhi[1], bhi[2])
        g0 = R.Graph(ref.table, lo, hi)
        assert g0.link[0][:, :, 63].any() and g0.node[:, :, 61].any() and g0.node[:, :, 66].any()
        for side in (61, 66):                                    # a source left of the word boundary, then right of it: both carries
            z, y = np.argwhere(g0.node[:, :, side])[0]
            g = run(("carry", side), m, ref, lo, hi, block_points([(lo[0] + side, lo[1] + y, lo[2] + z)]))
            assert (g.steps[:, :, 63] > 0).any() and (g.steps[:, :, 64] > 0).any() and g.info["n_sources"] == 1
            check_points(("carry", side), m, g, np.random.default_rng(side))
        run("carry, frontiers", m, ref, lo, hi, (), 100, 9, 2, True)
        for x in (blo[0] + 3, bhi[0] + 4):                       # nx = 1: inside the data, and beside it
            g = run(("nx = 1", x), m, ref, (x, blo[1], blo[2]), (x, bhi[1], bhi[2]), (), 1, 1, 1, True)
            assert g.node.any() == (x <= bhi[0]) and not g.link[0].any()
            check_points(("nx = 1", x), m, g, np.random.default_rng(3))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. both forms, the limit
def test_both_forms_of_the_propagation_and_the_size_limit():
    size = (48, 40, 33)
    m = mapper(size)
    try:
        scene(m, size)
        ref = B.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        pos, _ = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        blo, bhi = np.array(ref.blo), np.array(ref.bhi)
        assert R.words(blo, bhi) <= R.LDS_WORDS
        mid = (blo + bhi) // 2
        wide_lo, wide_hi = mid - (32, 32, 24), mid - (32, 32, 24) + (63, 63, 48)      # 64 x 64 x 49 cells: 3136 words, just over the LDS form's 3072
        assert R.LDS_WORDS < R.words(wide_lo, wide_hi) <= R.MAX_WORDS and (wide_lo < blo).all() and (wide_hi > bhi).all()
        big_lo, big_hi = mid - (64, 64, 32), mid - (64, 64, 32) + (127, 127, 63)      # 128 x 128 x 64 cells: the limit, 16384 words
        assert R.words(big_lo, big_hi) == R.MAX_WORDS
        inner = lambda g: g.steps[tuple(slice(int(blo[a] - g.lo[a]), int(bhi[a] - g.lo[a]) + 1) for a in (2, 1, 0))]      # noqa: E731
        for par in (dict(goals=[tuple(pos)]), dict(min_free=100, min_open=9, from_frontiers=True)):
            small = run(("lds", par), m, ref, blo, bhi, **par)
            assert small.info["n_reached"] > 20 and small.info["max_steps"] >= (4 if "goals" in par else 1)
            for name, lo, hi in (("global", wide_lo, wide_hi), ("limit", big_lo, big_hi)):      # (the planes grow here)
                g = run((name, par), m, ref, lo, hi, **par)
                assert np.array_equal(inner(g), small.steps) and g.info["n_reached"] == small.info["n_reached"]
                check_points((name, par), m, g, np.random.default_rng(2), n=100)
            run(("lds again", par), m, ref, blo, bhi, **par)     # (a smaller box in the grown planes)
        # over the limit: refused, and the kept result stays
        steps, cells = m.routes_read()
        for lo, hi in ((big_lo, big_hi + (1, 0, 0)), (big_lo, big_hi + (0, 1, 0)), (big_lo - (0, 0, 1), big_hi), ((0, 0, 0), (64 * 16384, 0, 0)),
                       ((-2 ** 31 + 1, 0, 0), (2 ** 31 - 2, 0, 0))):
            p = m.routes_param([int(v) for v in lo], [int(v) for v in hi])
            assert m._f["routes_compute"](m._h, None, 0, C.byref(p), None) == INVALID, (lo, hi)
        s2, c2 = m.routes_read()
        assert np.array_equal(s2, steps) and np.array_equal(c2, cells)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. pool edges
@pytest.mark.parametrize("max_blocks,per_workgroup", [(8000, 32), (40000, 128)])
def test_pool_ends_inside_a_workgroups_run(max_blocks, per_workgroup):
    """the blocks test of the same name: four units of eight slots per workgroup at 8000 slots, sixteen at 40 000, and the slots
    handed out end inside a run"""
    size = (48, 40, 33)
    m = mapper(size, max_blocks=max_blocks)
    try:
        scene(m, size)
        live = m.stats()["blocks_total"]
        assert live % per_workgroup != 0 and per_workgroup < live < max_blocks - per_workgroup, live
        ref = B.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        pos, _ = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        cut, unreached, _ = check_all(live, m, ref, pos, np.random.default_rng(4), min_frees=(1,), min_opens=(1, 64))
        assert cut > 0
    finally:
        m.close()


def test_empty_pool_before_the_first_pose():
    m = mapper((32, 24, 16))
    try:
        for ff in (False, True):
            info = m.routes_compute((-2, -2, -2), (3, 2, 1), [(0.0, 0.0, 0.0)], from_frontiers=ff)
            assert info.tolist()[:6] == (0, 0, 0, 0, 0, -1) and info["reserved"].tolist() == [0, 0]
            steps, cells = m.routes_read()
            assert steps.shape == (4, 5, 6) and (steps == -1).all() and not cells.any()
            assert m.routes_query([(0.0, 0.0, 0.0), (9.0, 9.0, 9.0)]).tolist() == [-1, -1]
            path, ln = m.routes_path([(0.0, 0.0, 0.0)], 3, path=np.full((1, 3, 3), -7, np.int32))
            assert ln.tolist() == [0] and (path == -7).all()
    finally:
        m.close()


def test_a_link_to_an_erased_neighbour_closes():
    size = (48, 40, 33)
    d = BoxDrive(size, delta=8)
    m = mapper(size, retain_radius_blocks=1, max_blocks=400)
    ref = B.GlobalRef(size)
    try:
        kept = {}
        for k in range(19):
            update(m, *d.frame(k))
            ref.add(m)
            if k == 15:                                          # the far end of the drive; three frames later the volume is three blocks back
                ref.take(m)
                box = (tuple(int(v) for v in ref.blo), tuple(int(v) for v in ref.bhi))
            if k in (15, 18):
                ref.take(m)
                kept[k] = run(k, m, ref, box[0], box[1], [tuple(d.frame(k)[0])], from_frontiers=True)
                check_points(k, m, kept[k], np.random.default_rng(k), n=100)
                live, _ = m.blocks_summary()
                kept[k, "live"] = {tuple(r) for r in live["key"].tolist()}
        was, now = kept[15], kept[18]
        # a link of the far end whose one end has been erased since (its key is gone from the pool) while the other end is still a node
        closed = 0
        for a, e in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            for z, y, x in np.argwhere(was.link[a]).tolist():
                k0 = (x + box[0][0], y + box[0][1], z + box[0][2])
                k1 = tuple(k0[i] + e[i] for i in range(3))
                gone = [k not in kept[18, "live"] for k in (k0, k1)]
                stays = [now.node[z, y, x], now.node[z + e[2], y + e[1], x + e[0]]]
                if (gone[0] and not gone[1] and stays[1]) or (gone[1] and not gone[0] and stays[0]):
                    assert not now.link[a][z, y, x]
                    closed += 1
        assert closed > 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. deferred records
def test_routes_leave_deferred_records_alone():
    """The drive of the blocks test test_blocks_read_deferred_records, with its guards: the update defers records to the pair plane
    (coc_defer == 1, tskip tiles present) and the calls store nothing of the tile state.  The stage reads types only, from g_type."""
    import lazy_bounds as L
    from hooks_py import HooksMapper
    size = (32, 24, 32)
    dr = L.Drive("blocks_32x24x32", size, 6, step=2, turn=20, p_occ=0.03, cutoff_dist=0.6)
    m = HooksMapper(dr.config())
    ref = B.GlobalRef(size)
    rng = np.random.default_rng(9)
    try:
        checked = 0
        for k, pos, q, kind, lab, _ in dr.frames():
            m.set_pose(pos, q)
            m.ogm_labels(lab)
            m.fuse()
            ref.add(m)
            if k == 4:
                ref.take(m)
                run(("after fuse", k), m, ref, ref.blo, ref.bhi, [tuple(pos)], 1, 9, 1, True)
            m.batch_edt()
            m.merge()
            if k < 2:
                continue
            st = m.debug_tile_state()
            n_tskip = int((st["tskip"] != 0).sum())
            assert st["coc_defer"] == 1 and n_tskip > 0, (k, st["coc_defer"], n_tskip)      # otherwise this covers nothing
            ref.take(m)
            g = run(("deferred", k), m, ref, ref.blo, ref.bhi, [tuple(pos)], 1, 9, 1, k % 2 == 0)
            check_points(("deferred", k), m, g, rng, n=100)
            st2 = m.debug_tile_state()
            assert (st2["tskip_count"], st2["caught_up"]) == (st["tskip_count"], st["caught_up"]), k            # the calls store nothing
            assert np.array_equal(st2["tskip"], st["tskip"]) and np.array_equal(st2["tlazy"], st["tlazy"])
            assert g.info["n_reached"] > 1
            checked += 1
        assert checked == 4
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. the _dev forms
def test_dev_forms_on_the_mappers_stream():
    import torch
    size = (64, 24, 20)
    m = mapper(size)
    try:
        scene(m, size)
        ref = B.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        pos, _ = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        blo, bhi = tuple(int(v) for v in ref.blo), tuple(int(v) for v in ref.bhi)
        box_a, box_b = (blo, bhi), (tuple(v - 1 for v in blo), tuple(v + 2 for v in bhi))
        goals = np.array([pos, (np.nan, 0, 0), (0, np.nan, 0), (np.nan,) * 3], np.float32)       # a NaN tail
        want = {}
        for name, (lo, hi) in (("a", box_a), ("b", box_b)):
            g = R.Graph(ref.table, lo, hi, 1, 2, 1)
            want[name] = g.solve(*R.point_blocks(goals, W), R.FROM_FRONTIERS if name == "a" else 0)
        cells_b = int(np.prod(want["b"].shape))
        rec, count = m.blocks_summary(min_fnt=1)
        assert count > 3
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            dgoals = torch.from_numpy(goals).to(dev)
            dinfo = torch.full((2, 8), 77, dtype=torch.int32, device=dev)
            m.routes_compute_dev(dgoals.data_ptr(), len(goals), *box_a, min_open=2, from_frontiers=True, d_info=dinfo[0].data_ptr())
            m.routes_compute_dev(dgoals.data_ptr(), len(goals), *box_b, min_open=2, d_info=0)      # back to back, no sync, info NULL: the kept box is the last
            dsteps = torch.full((cells_b + 4,), -9, dtype=torch.int32, device=dev)
            dcells = torch.full((cells_b + 4,), FILL, dtype=torch.uint8, device=dev)
            m.routes_read_dev(dsteps.data_ptr(), dcells.data_ptr())
            donly = torch.full((cells_b,), FILL, dtype=torch.uint8, device=dev)
            m.routes_read_dev(0, donly.data_ptr())
            # the frontier blocks' positions made on the device from gie_blocks_summary_dev's records, then one gather
            drec = torch.zeros((count * 8,), dtype=torch.int32, device=dev)
            dcnt = torch.zeros((1,), dtype=torch.int32, device=dev)
            m.blocks_summary_dev(drec.data_ptr(), dcnt.data_ptr(), 0, min_fnt=1, max_records=count)
            r = drec.view(count, 8)
            v = (r[:, 4] >> 16) & 0xffff                         # fnt_voxel: the upper half of the word behind the key and two counts
            vox = r[:, :3] * 8 + torch.stack([v >> 6, (v >> 3) & 7, v & 7], 1)
            dpos = (vox.to(torch.float32) * W).contiguous()
            dq = torch.full((count + 2,), -9, dtype=torch.int32, device=dev)
            m.routes_query_dev(dpos.data_ptr(), count, dq.data_ptr())
            dpath = torch.full((count, 4, 3), -7, dtype=torch.int32, device=dev)
            dlen = torch.full((count,), -9, dtype=torch.int32, device=dev)
            m.routes_path_dev(dpos.data_ptr(), count, 4, dpath.data_ptr(), dlen.data_ptr())
        m.sync()
        assert dinfo[0].cpu().numpy().tobytes() == want["a"].info.tobytes() and bool((dinfo[1] == 77).all())
        g = want["b"]
        assert np.array_equal(dsteps.cpu().numpy()[:cells_b].reshape(g.shape), g.steps) and bool((dsteps[cells_b:] == -9).all())
        assert dcells.cpu().numpy()[:cells_b].tobytes() == g.cells.tobytes() and bool((dcells[cells_b:] == FILL).all())
        assert donly.cpu().numpy().tobytes() == g.cells.tobytes()
        hs, hc = m.routes_read()                                 # the host reader sees the same kept box
        assert np.array_equal(hs, g.steps) and hc.tobytes() == g.cells.tobytes()
        got = drec.cpu().numpy().view(gie.BLOCK_SUMMARY_DTYPE)
        assert B.same(got, rec)
        hpos = dpos.cpu().numpy()
        key = got["key"].astype(np.int64) * 8
        fv = got["fnt_voxel"].astype(np.int64)
        assert np.array_equal(hpos, ((key + np.stack([fv >> 6, (fv >> 3) & 7, fv & 7], -1)).astype(np.float32) * np.float32(W)))
        wq = g.query(hpos, W)
        assert np.array_equal(dq.cpu().numpy()[:count], wq) and bool((dq[count:] == -9).all()) and (wq >= 0).any()
        wpath, wln = g.path(hpos, W, 4, fill=-7)
        assert np.array_equal(dlen.cpu().numpy(), wln) and np.array_equal(dpath.cpu().numpy(), wpath)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. refusals
def test_invalid_arguments_leave_the_buffers_alone():
    import torch
    size = (32, 24, 16)
    m, t, fresh = mapper(size), mapper(size), mapper(size)
    try:
        scene(m, size, room=False)
        scene(fresh, size, room=False)
        f = m._f
        lo, hi = (-1, -1, -1), (2, 2, 2)
        cells = 64
        goals = np.zeros((2, 3), np.float32)
        info = np.full(8, 0x5a5a5a5a, np.int32)
        steps, cb = np.full(cells, -9, np.int32), np.full(cells, FILL, np.uint8)
        qs = np.full(2, -9, np.int32)
        path, ln = np.full((2, 4, 3), -7, np.int32), np.full(2, -9, np.int32)
        dinfo = torch.full((8,), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
        dgoals = torch.zeros((2, 3), dtype=torch.float32, device="cuda:0")
        dsteps = torch.full((cells,), -9, dtype=torch.int32, device="cuda:0")
        dcb = torch.full((cells,), FILL, dtype=torch.uint8, device="cuda:0")
        dqs = torch.full((2,), -9, dtype=torch.int32, device="cuda:0")
        dpath = torch.full((2, 4, 3), -7, dtype=torch.int32, device="cuda:0")
        dln = torch.full((2,), -9, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        P = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
        D = lambda a: C.c_void_p(a.data_ptr())                   # noqa: E731
        forms = (("", P(goals), P(info), P(steps), P(cb), P(qs), P(path), P(ln)), ("_dev", D(dgoals), D(dinfo), D(dsteps), D(dcb), D(dqs), D(dpath), D(dln)))

        def par(lo=lo, hi=hi, **kw):
            p = m.routes_param(lo, hi)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p
        top, big = -2 ** 31, 2 ** 31 - 1
        bad = [par(lo=(3, -1, -1)), par(lo=(-1, 3, -1)), par(lo=(-1, -1, 3)), par(lo=(top, -1, -1)), par(hi=(2, big, 2)), par(lo=(None,) * 3, hi=(None,) * 3),
               par(min_free=0), par(min_free=513), par(min_open=0), par(min_open=65), par(min_fnt=0), par(min_fnt=513), par(min_free=-1),
               par(reserved=0), par(reserved=1), par(flags=2), par(flags=3), par(flags=-1), par(lo=(0, 0, 0), hi=(128, 127, 63)), par(lo=(0, 0, 0), hi=(63, 16384, 0))]
        for suffix, g, i, s, c, q, pa, l in forms:
            comp = f["routes_compute" + suffix]
            # read / query / path before the first compute
            for h in (m._h, fresh._h):
                if h is m._h and suffix == "_dev":
                    continue                                     # (m has its first compute by then)
                assert f["read_routes" + suffix](h, s, c) == INVALID
                assert f["routes_query" + suffix](h, g, 2, q) == INVALID
                assert f["routes_path" + suffix](h, g, 2, 4, pa, l) == INVALID
            for p in bad:
                assert comp(m._h, g, 2, C.byref(p), i) == INVALID, (suffix, list(p.lo), list(p.hi), p.min_free, p.min_open, p.min_fnt, p.flags, list(p.reserved))
            assert comp(m._h, g, 2, None, i) == INVALID          # NULL parameters
            assert comp(m._h, g, -1, C.byref(par()), i) == INVALID
            assert comp(m._h, None, 2, C.byref(par()), i) == INVALID       # NULL points with n > 0
            assert comp(None, g, 2, C.byref(par()), i) == INVALID
            m.sync()
            assert (info == 0x5a5a5a5a).all() and bool((dinfo == 0x5a5a5a5a).all())
            assert comp(m._h, g, 2, C.byref(par()), None) == 0   # a good compute; info may be NULL
            assert f["read_routes" + suffix](m._h, None, None) == INVALID
            assert f["routes_query" + suffix](m._h, g, -1, q) == INVALID and f["routes_query" + suffix](m._h, None, 2, q) == INVALID
            assert f["routes_query" + suffix](m._h, g, 2, None) == INVALID
            assert f["routes_path" + suffix](m._h, g, -1, 4, pa, l) == INVALID and f["routes_path" + suffix](m._h, g, 2, 0, pa, l) == INVALID
            assert f["routes_path" + suffix](m._h, None, 2, 4, pa, l) == INVALID and f["routes_path" + suffix](m._h, g, 2, 4, None, l) == INVALID
            assert f["routes_path" + suffix](m._h, g, 2, 4, pa, None) == INVALID
        t.set_tile((8, 0, 0), (64, 24, 16))                      # a tiled mapper: every call refuses
        for suffix, g, i, s, c, q, pa, l in forms:
            assert f["routes_compute" + suffix](t._h, g, 2, C.byref(par()), i) == INVALID
            assert f["read_routes" + suffix](t._h, s, c) == INVALID and f["routes_query" + suffix](t._h, g, 2, q) == INVALID
            assert f["routes_path" + suffix](t._h, g, 2, 4, pa, l) == INVALID
        m.sync()
        assert (info == 0x5a5a5a5a).all() and (steps == -9).all() and (cb == FILL).all() and (qs == -9).all() and (path == -7).all() and (ln == -9).all()
        assert bool((dinfo == 0x5a5a5a5a).all()) and bool((dsteps == -9).all()) and bool((dcb == FILL).all()) and bool((dqs == -9).all())
        assert bool((dpath == -7).all()) and bool((dln == -9).all())
        # (the same calls with good arguments work; either output of the reader alone, n == 0)
        for suffix, g, i, s, c, q, pa, l in forms:
            assert f["routes_compute" + suffix](m._h, g, 2, C.byref(par()), i) == 0 and f["routes_compute" + suffix](m._h, None, 0, C.byref(par()), None) == 0
            assert f["read_routes" + suffix](m._h, s, None) == 0 and f["read_routes" + suffix](m._h, None, c) == 0
            assert f["routes_query" + suffix](m._h, g, 2, q) == 0 and f["routes_path" + suffix](m._h, g, 2, 4, pa, l) == 0
            assert f["routes_query" + suffix](m._h, None, 0, None) == 0 and f["routes_path" + suffix](m._h, None, 0, 4, None, None) == 0
        m.sync()
        assert info[6] == 0 and info[0] >= 0 and not (steps == -9).any() and not (cb == FILL).any() and not (qs == -9).any() and not (ln == -9).any()
        assert int(dinfo.cpu()[6]) == 0 and not bool((dsteps == -9).any()) and not bool((dqs == -9).any()) and not bool((dln == -9).any())
    finally:
        m.close()
        t.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------- 9. the update does not notice
def test_routes_calls_change_nothing_of_the_map_update():
    size = (48, 40, 33)
    d = BoxDrive(size, seed=5)

    def calls(a, k, phase, pos):
        pv = np.array(a.pivot()) >> 3
        a.routes_compute(tuple(pv - 2), tuple(pv + 7), [tuple(pos)], min_free=1 + 50 * (k % 3), min_open=1 + 8 * (len(phase) % 3), from_frontiers=k % 2 == 0)
        a.routes_read()
        a.routes_query(block_points([pv, pv + 3]))
        a.routes_path(block_points([pv + 2]), 5)
    stage_calls_change_nothing(size, (d.frame(k) for k in range(10)), mapper, calls)


# ---------------------------------------------------------------------------------------------------------- 10. host layer
def test_host_layer_routes_match_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "routes_host_probe")
    size, w, cutoff, min_fnt, max_goals, min_free, min_open = (48, 40, 33), 0.1, 3.0, 3, 12, 40, 6
    frames, fpath = lidar_frames(tmp_path)
    m = mapper(size, voxel=w, cutoff_dist=cutoff)
    ref = B.GlobalRef(size)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            ref.add(m)
            m.ogm_pointcloud(pts)
            m.set_ext_boxes(np.array([[-3.6, -3.2, 0.2]], np.float32), np.array([[4.4, 3.4, 2.6]], np.float32), np.zeros(1, np.uint8))
            m.fuse(); m.batch_edt(); m.merge()
        rec, count = m.blocks_summary(dist=True, min_fnt=min_fnt)
        ref.take(m)
        robot = frames[-1][0]
        wpos, wkeys, wn, wd, wsteps = R.route_goals(ref.table, rec, robot, w, max_goals, min_free, min_open, min_fnt)
        # the mapper's own calls over the host layer's box give the reference's steps
        old_pos, _, _ = B.goals(rec, robot, w, max_goals)
        rb, _ = R.point_blocks(np.asarray(robot, np.float32).reshape(1, 3), w)
        lo, hi = R.routes_box(R.point_blocks(old_pos, w)[0], rb[0])
        m.routes_compute(lo, hi, [tuple(robot)], min_free, min_open, min_fnt)
        assert np.array_equal(np.sort(m.routes_query(old_pos)), np.sort(wsteps))
    finally:
        m.close()
    assert count > max_goals and (wsteps >= 0).any()
    res = subprocess.run([exe, fpath, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), str(min_fnt), str(max_goals), str(min_free), str(min_open)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert lines[0] == "blocks %d goals %d" % (count, max_goals), lines[0]
    got = [ln.split() for ln in lines[1:] if ln.strip()]
    assert len(got) == max_goals
    bits = wpos.view(np.uint32)
    for i, g in enumerate(got):                                  # the same order, the same positions bit for bit, the same steps
        assert [int(v, 16) for v in g[:3]] == bits[i].tolist(), (i, g)
        assert [int(v) for v in g[3:6]] == wkeys[i].tolist(), (i, g)
        assert (int(g[6]), int(g[7]), int(g[8])) == (int(wn[i]), int(wd[i]), int(wsteps[i])), (i, g)
    reached = wsteps[wsteps >= 0]
    assert (np.diff(reached) >= 0).all() and (wsteps[len(reached):] == -1).all()

"""Global block summaries on the device (include/gie.h "global block summaries", gie_blocks.inc.h) against the numpy reference of
tests/blocks_ref.py over Mapper.query_global.  Every comparison is exact: two record lists are sorted by key and must be byte-equal,
a grid must be equal cell for cell."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import blocks_ref as R
import gie
from gie import _capi
from stage_common import BoxDrive, build_host_probe, lidar_frames, mapper, scene, stage_calls_change_nothing, update

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # GIE_ERR_INVALID
FILL = 0x5a


def check(tag, got, count, want):
    assert count == len(want) == len(got), (tag, count, len(got), len(want))
    assert R.canon(got).tobytes() == want.tobytes(), tag


def check_all(tag, m, ref, boxes, min_fnts=(0, 1, 40)):
    """every flag value, box and min_fnt against the reference of one checkpoint; the grid of every finite box.  Returns the DIST
    records of the open box."""
    full = None
    for dist in (False, True):
        for lo, hi in boxes:
            for min_fnt in min_fnts:
                want = ref.summaries(dist, min_fnt, lo, hi)
                if lo is None or min_fnt != min_fnts[0]:
                    got, count = m.blocks_summary(lo, hi, dist=dist, min_fnt=min_fnt)
                else:
                    got, count, g = m.blocks_summary(lo, hi, dist=dist, min_fnt=min_fnt, grid=True)
                    assert np.array_equal(g, ref.grid(lo, hi)), (tag, dist, lo, hi)
                check((tag, dist, lo, hi, min_fnt), got, count, want)
                if dist and lo is None and min_fnt == 0:
                    full = got
    return full


def data_boxes(ref):
    """the open box, a box cutting the data, a box around all of it"""
    blo, bhi = ref.blo, ref.bhi
    cut_lo = (int(blo[0]) + 2, int(blo[1]) + 1, int(blo[2]) + 1)
    cut_hi = (max(int(bhi[0]) - 3, cut_lo[0]), max(int(bhi[1]) - 1, cut_lo[1]), int(bhi[2]))
    return [(None, None), (cut_lo, cut_hi), (tuple(int(v) - 1 for v in blo), tuple(int(v) + 1 for v in bhi))]


# ---------------------------------------------------------------------------------------------------------- 1. a drive
@pytest.mark.parametrize("size", [(48, 40, 33), (21, 19, 10)])
def test_blocks_on_a_drive(size):
    d = BoxDrive(size)
    m = mapper(size)
    ref = R.GlobalRef(size)
    try:
        behind = 0
        for k in range(20):
            pos, q, lab = d.frame(k)
            m.set_pose(pos, q)
            m.ogm_labels(lab)
            m.fuse()
            ref.add(m)
            if k == 12:                                          # between gie_fuse and gie_batch_edt, against query_global at the same point
                ref.take(m)
                check_all(("after fuse", k), m, ref, data_boxes(ref)[:2], min_fnts=(0, 1))
            m.batch_edt()
            m.merge()
            if k + 1 not in (1, 9, 20):
                continue
            ref.take(m)
            full = check_all(("merge", k), m, ref, data_boxes(ref))
            assert len(full) > 0 and (full["key"] < 0).any() and (full["n_occupied"] > 0).any()
            assert (full["min_dist_sq"] != R.EMPTY_VALUE).any() and (full["flags"] == 1).all()
            # frontier the robot has left behind: blocks with FNT voxels wholly outside the current local volume
            pv = np.array(m.pivot())
            vlo = full["key"].astype(np.int64) * 8
            outside = ((vlo + 8 <= pv) | (vlo >= pv + np.array(size))).any(1)
            behind += int((outside & (full["n_fnt"] > 0)).sum())
        assert behind > 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. deferred records
def test_blocks_read_deferred_records():
    """The drive of the display clouds' test of the same name, with its two guards: the update defers records to the pair plane
    (coc_defer == 1, tskip tiles present) and the call stores nothing of the tile state."""
    import lazy_bounds as L
    from hooks_py import HooksMapper
    size = (32, 24, 32)
    dr = L.Drive("blocks_32x24x32", size, 6, step=2, turn=20, p_occ=0.03, cutoff_dist=0.6)
    m = HooksMapper(dr.config())
    ref = R.GlobalRef(size)
    try:
        checked = changed = 0
        prev = None
        for k, pos, q, kind, lab, _ in dr.frames():
            m.set_pose(pos, q)
            m.ogm_labels(lab)
            m.fuse()
            ref.add(m)
            if k == 4:
                want = ref.take(m).summaries(True)
                got, count = m.blocks_summary(dist=True)
                check(("after fuse", k), got, count, want)
                assert count > 0
            m.batch_edt()
            m.merge()
            if k < 2:
                continue
            st = m.debug_tile_state()
            n_tskip = int((st["tskip"] != 0).sum())
            assert st["coc_defer"] == 1 and n_tskip > 0, (k, st["coc_defer"], n_tskip)      # otherwise this covers nothing
            got, count = m.blocks_summary(dist=True)
            st2 = m.debug_tile_state()
            assert (st2["tskip_count"], st2["caught_up"]) == (st["tskip_count"], st["caught_up"]), k            # the call stores nothing
            assert np.array_equal(st2["tskip"], st["tskip"]) and np.array_equal(st2["tlazy"], st["tlazy"])
            check(("deferred", k), got, count, ref.take(m).summaries(True))
            checked += 1
            # the records of the flagged tiles' voxels changed while only the pair plane held them (the clouds' guard)
            tz, ty, tx = np.nonzero(st["tskip"])
            o = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
            loc = (np.stack([tx, ty, tz], -1)[:, None, :] * 8 + o[None]).reshape(-1, 3)
            loc = loc[(loc < np.array(size)).all(1)]
            g = (loc + np.array(m.pivot())).astype(np.int32)
            cur = {tuple(c): int(v) for c, v in zip(g.tolist(), m.query_global(g)["dist_sq"])}
            if prev is not None:
                changed += sum(1 for c, v in cur.items() if c in prev and prev[c] != v)
            prev = cur
        assert checked == 4
        assert changed > 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. erasure
def test_blocks_with_erased_blocks():
    size = (48, 40, 33)
    d = BoxDrive(size, delta=8)
    max_blocks = 400                                             # (240 blocks are live at a time, 990 are handed out over the drive)
    m = mapper(size, retain_radius_blocks=1, max_blocks=max_blocks)
    ref = R.GlobalRef(size)
    try:
        handed_out, far = 0, None
        for k in range(30):
            update(m, *d.frame(k))
            ref.add(m)
            s = m.stats()
            handed_out += s["blocks_new"]
            assert s["blocks_total"] <= max_blocks
            if k == 14:                                          # the far end of the drive
                far, _ = m.blocks_summary()
            if k in (14, 29):
                ref.take(m)
                check_all(k, m, ref, data_boxes(ref)[:2], min_fnts=(0, 1))
        assert handed_out > max_blocks, handed_out               # more blocks handed out than the pool has slots: slots were reused
        # a block left behind has vanished: beyond the last volume's retained box the far end's records are gone
        edge = (m.pivot()[0] + size[0] + 8 * 3) >> 3
        last, _ = m.blocks_summary()
        assert (far["key"][:, 0] > edge).any() and not (last["key"][:, 0] > edge).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. pool edges
@pytest.mark.parametrize("max_blocks,per_workgroup", [(8000, 32), (40000, 128)])
def test_pool_ends_inside_a_workgroups_run(max_blocks, per_workgroup):
    """A workgroup takes 1 to 16 units of eight slots, chosen from the size of the pool: four units at 8000 slots, sixteen at
    40 000.  The slots handed out end inside a run (asserted), so the last workgroup with work has slots beyond the bound."""
    size = (48, 40, 33)
    m = mapper(size, max_blocks=max_blocks)
    try:
        scene(m, size)
        live = m.stats()["blocks_total"]
        assert live % per_workgroup != 0 and per_workgroup < live < max_blocks - per_workgroup, live
        ref = R.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        full = check_all(live, m, ref, data_boxes(ref), min_fnts=(0, 1))
        assert len(full) > per_workgroup
    finally:
        m.close()


def test_empty_pool_before_the_first_pose():
    m = mapper((32, 24, 16))
    try:
        for dist in (False, True):
            rec, count, g = m.blocks_summary((-2, -2, -2), (3, 2, 1), dist=dist, max_records=5, grid=True)
            assert count == 0 and len(rec) == 0 and g.shape == (4, 5, 6) and not g.any()
            rec, count = m.blocks_summary(dist=dist)
            assert count == 0 and len(rec) == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. capacity
def test_capacity_and_tail_in_both_forms():
    import torch
    size = (48, 40, 33)
    m = mapper(size)
    try:
        scene(m, size)
        full, count = m.blocks_summary(dist=True, min_fnt=1)
        assert count == len(full) > 10
        n = C.c_int32(-1)
        p = m.blocks_param(dist=True, min_fnt=1)
        assert m._f["blocks_summary"](m._h, C.byref(p), None, C.byref(n), None) == 0 and n.value == count      # NULL out only counts
        members = {r.tobytes() for r in full}
        assert len(members) == count
        for cap in (0, 1, count - 1, count, count + 3):
            nw = min(count, cap)
            p = m.blocks_param(dist=True, min_fnt=1, max_records=cap)
            buf = np.full(32 * (cap + 5), FILL, np.uint8)
            n.value = -1
            assert m._f["blocks_summary"](m._h, C.byref(p), buf.ctypes.data_as(C.c_void_p) if cap else None, C.byref(n), None) == 0
            dbuf = torch.full((32 * (cap + 5),), FILL, dtype=torch.uint8, device="cuda:0")
            dn = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            m.blocks_summary_dev(dbuf.data_ptr() if cap else 0, dn.data_ptr(), 0, dist=True, min_fnt=1, max_records=cap)
            m.sync()
            for form, raw, c2 in (("host", buf, n.value), ("dev", dbuf.cpu().numpy(), int(dn.cpu()[0]))):
                assert c2 == count, (form, cap)                  # always the full count
                rows = [r.tobytes() for r in raw[:32 * nw].view(gie.BLOCK_SUMMARY_DTYPE)]
                assert len(set(rows)) == nw and set(rows) <= members, (form, cap)      # distinct valid records
                assert raw[32 * nw:].tobytes() == bytes([FILL]) * (32 * (cap + 5 - nw)), (form, cap)      # the tail is intact
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. the _dev form
def test_dev_form_on_the_mappers_stream():
    import torch
    size = (64, 24, 20)
    m = mapper(size)
    try:
        scene(m, size)
        ref = R.GlobalRef(size)
        ref.add(m)
        ref.take(m)
        lo, hi = tuple(int(v) - 1 for v in ref.blo), tuple(int(v) + 1 for v in ref.bhi)
        cells = int(np.prod([hi[k] - lo[k] + 1 for k in range(3)]))
        want = {dist: m.blocks_summary(lo, hi, dist=dist, grid=True) for dist in (False, True)}
        cap = want[True][1] + 3
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            outs = {}
            for dist in (False, True):                           # two calls back to back, no sync in between
                dout = torch.full((cap * 32,), FILL, dtype=torch.uint8, device=dev)
                dcnt = torch.full((1,), 77, dtype=torch.int32, device=dev)
                dgrid = torch.full((cells,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
                m.blocks_summary_dev(dout.data_ptr(), dcnt.data_ptr(), dgrid.data_ptr(), lo, hi, dist=dist, max_records=cap)
                outs[dist] = (dout, dcnt, dgrid)
            dgrid_only = torch.full((cells,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
            m.blocks_summary_dev(0, 0, dgrid_only.data_ptr(), lo, hi)
            dcnt_only = torch.full((1,), 77, dtype=torch.int32, device=dev)
            m.blocks_summary_dev(0, dcnt_only.data_ptr(), 0, min_fnt=1)
            dno_count = torch.full((cap * 32,), FILL, dtype=torch.uint8, device=dev)
            m.blocks_summary_dev(dno_count.data_ptr(), 0, 0, max_records=cap)
        m.sync()
        for dist, (dout, dcnt, dgrid) in outs.items():
            rec, count, g = want[dist]
            assert count > 0 and int(dcnt.cpu()[0]) == count, dist
            raw = dout.cpu().numpy()
            check(("dev", dist), raw[:32 * count].view(gie.BLOCK_SUMMARY_DTYPE), count, R.canon(rec))
            check(("ref", dist), rec, count, ref.summaries(dist, 0, lo, hi))
            assert raw[32 * count:].tobytes() == bytes([FILL]) * (32 * (cap - count))
            assert np.array_equal(dgrid.cpu().numpy().view(np.uint32).reshape(g.shape), g) and np.array_equal(g, ref.grid(lo, hi))
        assert np.array_equal(dgrid_only.cpu().numpy().view(np.uint32).reshape(want[False][2].shape), want[False][2])
        assert int(dcnt_only.cpu()[0]) == len(ref.summaries(False, 1))
        n0 = want[False][1]
        assert R.same(dno_count.cpu().numpy()[:32 * n0].view(gie.BLOCK_SUMMARY_DTYPE), want[False][0])
        # the binding's own device route gives the host form's result
        rec, count, g = m.blocks_summary(lo, hi, dist=True, grid=True, dev=True)
        check("dev=True", rec, count, R.canon(want[True][0]))
        assert np.array_equal(g, want[True][2])
        # a misaligned d_out is refused and nothing is written
        dbuf = torch.full((cap * 32 + 16,), FILL, dtype=torch.uint8, device=dev)
        dn = torch.full((1,), -7, dtype=torch.int32, device=dev)
        p = m.blocks_param(max_records=cap)
        for off in (4, 8, 12):
            assert m._f["blocks_summary_dev"](m._h, C.byref(p), C.c_void_p(dbuf.data_ptr() + off), C.c_void_p(dn.data_ptr()), None) == INVALID, off
        m.sync()
        assert int(dn.cpu()[0]) == -7 and bool((dbuf == FILL).all())
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. refusals
def test_invalid_arguments_leave_the_buffers_alone():
    import torch
    size = (32, 24, 16)
    m, t = mapper(size), mapper(size)
    try:
        scene(m, size, room=False)
        f = m._f
        cells = 4 * 4 * 4
        buf = np.full(32 * 64, FILL, np.uint8)
        grid = np.full(cells, 0x5a5a5a5a, np.uint32)
        n = C.c_int32(-7)
        dbuf = torch.full((32 * 64,), FILL, dtype=torch.uint8, device="cuda:0")
        dgrid = torch.full((cells,), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
        dn = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        host = (buf.ctypes.data_as(C.c_void_p), C.cast(C.byref(n), C.c_void_p), grid.ctypes.data_as(C.c_void_p))
        devp = (C.c_void_p(dbuf.data_ptr()), C.c_void_p(dn.data_ptr()), C.c_void_p(dgrid.data_ptr()))

        def P(lo=(-1, -1, -1), hi=(2, 2, 2), **kw):
            p = m.blocks_param(lo, hi, max_records=64)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p
        big, top = 2 ** 31 - 1, -2 ** 31
        bad = [P(lo=(3, -1, -1)), P(lo=(-1, 3, -1)), P(lo=(-1, -1, 3)), P(flags=2), P(flags=-1), P(flags=3), P(min_fnt=-1), P(min_fnt=513),
               P(max_records=-1), P(reserved=0), P(reserved=1), P(reserved=2)]
        # with a grid only: a box that is open on a side, too long on a side, or of too many cells
        bad_grid = [P(lo=(top, -1, -1)), P(hi=(2, big, 2)), P(lo=(None, None, None), hi=(None, None, None)), P(lo=(0, 0, 0), hi=(1024, 0, 0)),
                    P(lo=(0, 0, -1024), hi=(0, 0, 0)), P(lo=(0, 0, 0), hi=(1023, 1023, 16)), P(lo=(-512, -512, -512), hi=(511, 511, 511))]
        for name, (out, cnt, g) in (("blocks_summary", host), ("blocks_summary_dev", devp)):
            for p in bad:
                assert f[name](m._h, C.byref(p), out, cnt, g) == INVALID, (name, list(p.lo), p.flags, p.min_fnt, p.max_records, list(p.reserved))
            for p in bad_grid:
                assert f[name](m._h, C.byref(p), out, cnt, g) == INVALID, (name, list(p.lo), list(p.hi))
            assert f[name](m._h, None, out, cnt, g) == INVALID                           # a NULL param
            assert f[name](m._h, C.byref(P()), None, cnt, g) == INVALID                  # a NULL out with max_records > 0
            assert f[name](m._h, C.byref(P(max_records=0)), None, None, None) == INVALID  # nothing to write
            assert f[name](None, C.byref(P()), out, cnt, g) == INVALID
        t.set_tile((8, 0, 0), (64, 24, 16))                      # a tiled mapper: both refuse
        assert f["blocks_summary"](t._h, C.byref(P()), *host) == INVALID and f["blocks_summary_dev"](t._h, C.byref(P()), *devp) == INVALID
        for off in (4, 8, 12, 16 + 2):                           # a d_out that is not 16-byte aligned
            assert f["blocks_summary_dev"](m._h, C.byref(P(max_records=8)), C.c_void_p(dbuf.data_ptr() + off), devp[1], devp[2]) == INVALID, off
        m.sync()
        assert n.value == -7 and buf.tobytes() == bytes([FILL]) * (32 * 64) and (grid == 0x5a5a5a5a).all()
        assert int(dn.cpu()[0]) == -7 and bool((dbuf == FILL).all()) and bool((dgrid == 0x5a5a5a5a).all())
        # (the same calls with good arguments work; an open box without a grid is fine)
        assert f["blocks_summary"](m._h, C.byref(P()), *host) == 0 and 0 < n.value and not (grid == 0x5a5a5a5a).any()
        assert f["blocks_summary"](m._h, C.byref(P(lo=(None,) * 3, hi=(None,) * 3)), host[0], host[1], None) == 0 and 0 < n.value
        assert f["blocks_summary_dev"](m._h, C.byref(P()), *devp) == 0
        m.sync()
        assert int(dn.cpu()[0]) > 0
    finally:
        m.close()
        t.close()


# ---------------------------------------------------------------------------------------------------------- 8. the update does not notice
def test_blocks_calls_change_nothing_of_the_map_update():
    size = (48, 40, 33)
    d = BoxDrive(size, seed=5)

    def calls(a, k, phase, pos):
        pv = np.array(a.pivot()) >> 3
        a.blocks_summary(dist=(k + len(phase)) % 2 == 0, min_fnt=k % 3)
        a.blocks_summary(tuple(pv - 1), tuple(pv + 4), dist=True, grid=True)
    stage_calls_change_nothing(size, (d.frame(k) for k in range(10)), mapper, calls)


# ---------------------------------------------------------------------------------------------------------- 9. host layer
def test_host_layer_goals_match_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "blocks_host_probe")
    size, w, cutoff, min_fnt, max_goals = (48, 40, 33), 0.1, 3.0, 3, 12
    frames, fpath = lidar_frames(tmp_path)
    m = mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.set_ext_boxes(np.array([[-3.6, -3.2, 0.2]], np.float32), np.array([[4.4, 3.4, 2.6]], np.float32), np.zeros(1, np.uint8))
            m.fuse(); m.batch_edt(); m.merge()
        rec, count = m.blocks_summary(dist=True, min_fnt=min_fnt)
    finally:
        m.close()
    assert count > max_goals and (rec["n_fnt"] >= min_fnt).all()
    wpos, wn, wd = R.goals(rec, frames[-1][0], w, max_goals)
    res = subprocess.run([exe, fpath, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), str(min_fnt), str(max_goals)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert lines[0] == "blocks %d goals %d" % (count, max_goals), lines[0]
    got = [ln.split() for ln in lines[1:] if ln.strip()]
    assert len(got) == max_goals
    bits = wpos.view(np.uint32)
    for i, g in enumerate(got):                                  # the same order, the same positions bit for bit
        assert [int(v, 16) for v in g[:3]] == bits[i].tolist(), (i, g)
        assert (int(g[6]), int(g[7])) == (int(wn[i]), int(wd[i])), (i, g)

"""Display clouds on the device (include/gie.h "display clouds", gie_cloud.inc.h) against the numpy reference of tests/cloud_ref.py
over Mapper.read_local / Mapper.query_global.  Every comparison is exact: two clouds are sorted by the bit patterns of their four
words and must be byte-equal."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cloud_ref as R
import gie
from gie import _capi, scenes
from stage_common import BoxDrive, build_host_probe, lidar_frames, mapper, scene, stage_calls_change_nothing, update

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # GIE_ERR_INVALID
FNT_T = R.param(1 << R.FNT, R.TYPE)
SIX = {"ogm": R.param(1 << R.OCCUPIED, R.TYPE), "edt": R.param(R.KNOWN, R.DIST), "fnt": FNT_T,
       "free_fnt_dist": R.param((1 << R.FREE) | (1 << R.FNT), R.DIST)}


def band(p, lo, hi):
    return dict(p, z_lo=R.NO_BAND[0] if lo is None else lo, z_hi=R.NO_BAND[1] if hi is None else hi)


def call(m, form, p, **kw):
    f = m.cloud_local if form == "local" else m.cloud_global
    return f(p["type_mask"], p["intensity"], p["z_lo"], p["z_hi"], **kw)


def check(tag, got, count, want):
    assert count == len(want) == len(got), (tag, count, len(got), len(want))
    assert R.canon(got).tobytes() == R.canon(want).tobytes(), tag


class GlobalRef:
    """the query_global records of the union box of all volumes so far, +- 8 voxels (one reference per checkpoint, shared by its clouds)"""

    def __init__(self, size):
        self.size, self.lo, self.hi = np.array(size), None, None

    def add(self, m):
        pv = np.array(m.pivot())
        self.lo = pv - 8 if self.lo is None else np.minimum(self.lo, pv - 8)
        self.hi = pv + self.size + 8 if self.hi is None else np.maximum(self.hi, pv + self.size + 8)

    def take(self, m):
        self.xyz = R.box_coords(self.lo, self.hi)
        self.rec = m.query_global(self.xyz)
        return self

    def cloud(self, w, p):
        return R.global_cloud(self.rec, self.xyz, w, p)


# ---------------------------------------------------------------------------------------------------------- 1. local
@pytest.mark.parametrize("size", [(48, 40, 33), (64, 24, 20), (65, 20, 20), (97, 61, 45), (77, 53, 1), (1, 40, 40)])
def test_local_clouds_of_one_scene(size):
    m = mapper(size)
    try:
        loc, _, _ = scene(m, size)
        pvt, w, Z = m.pivot(), m.cfg.voxel_width, size[2]
        n = size[0] * size[1] * size[2]
        bands = [(None, None), (pvt[2], pvt[2]), (pvt[2] + Z - 1, pvt[2] + Z - 1), (pvt[2] - 5, pvt[2] + 2), (pvt[2] - 40, pvt[2] - 1)]
        for name, p0 in SIX.items():
            for lo, hi in bands:
                p = band(p0, lo, hi)
                want = R.local_cloud(loc["type"], loc["edt"], pvt, w, p)
                got, count = call(m, "local", p)
                check((size, name, lo, hi), got, count, want)
                if hi is not None and hi < pvt[2]:
                    assert count == 0
                if lo is None and name in ("ogm", "edt"):
                    assert 0 < count < n, (size, name, count)     # neither empty nor the whole volume
    finally:
        m.close()


def test_several_units_per_workgroup():
    """A workgroup takes one unit of 4096 voxels (eight slots) while that leaves 256 workgroups, up to 16 beyond: 1.3 M voxels are
    two units per workgroup in the local form (type clouds; distance clouds stay at one), a pool of 40 000 slots is 16 in the
    global form (thin bands stay at one)."""
    size = (128, 128, 80)
    m = mapper(size, max_blocks=40000)
    try:
        loc, _, _ = scene(m, size)
        pvt, w = m.pivot(), m.cfg.voxel_width
        ref = GlobalRef(size)
        ref.add(m)
        ref.take(m)
        for name in ("ogm", "edt", "free_fnt_dist"):
            for lo, hi in ((None, None), (pvt[2] + 41, pvt[2] + 41)):
                p = band(SIX[name], lo, hi)
                got, count = call(m, "local", p)
                check((name, lo, "local"), got, count, R.local_cloud(loc["type"], loc["edt"], pvt, w, p))
                got, count = call(m, "global", p)
                check((name, lo, "global"), got, count, ref.cloud(w, p))
                assert count > 0
            got, count = call(m, "global", SIX[name], max_points=1000)      # a cloud that does not fit: waves beyond the capacity leave early
            assert len(got) == 1000 < count and len({r.tobytes() for r in R.canon(got)}) == 1000
    finally:
        m.close()


def test_pool_ends_inside_a_workgroups_run():
    """A pool of 1000 units of eight slots is four units (32 slots) per workgroup; the slots handed out end inside a run
    (asserted), so the last workgroup with work has units beyond the bound behind its live ones."""
    size = (48, 40, 33)
    m = mapper(size, max_blocks=8000)
    try:
        scene(m, size)
        live = m.stats()["blocks_total"]
        assert live % 32 != 0 and live < 8000 - 32, live
        ref = GlobalRef(size)
        ref.add(m)
        ref.take(m)
        w = m.cfg.voxel_width
        for name in ("ogm", "edt", "fnt"):
            got, count = call(m, "global", SIX[name])
            check((name, live), got, count, ref.cloud(w, SIX[name]))
            assert count > 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. global
def test_global_clouds_on_a_drive():
    """BoxDrive's volumes always hold an obstacle, so every known voxel of the drive has a valid distance (the batch EDT reaches
    the whole volume).  The drive is therefore preceded by one update of an obstacle-free volume next to it (disjoint in y): its
    voxels stay in the map with "see nothing" distances, which the DIST clouds of all three checkpoints have to drop."""
    size = (48, 40, 33)
    d = BoxDrive(size)
    m = mapper(size)
    ref = GlobalRef(size)
    try:
        w = m.cfg.voxel_width
        dropped = 0
        update(m, (np.float32(0.0), np.float32(6.0), np.float32(0.0)), (1.0, 0.0, 0.0, 0.0), np.ones(size[::-1], np.int8))
        ref.add(m)
        for k in range(20):
            update(m, *d.frame(k))
            ref.add(m)
            if k + 1 not in (1, 9, 20):
                continue
            ref.take(m)
            pv = np.array(m.pivot())
            slice_z = int(pv[2]) + 11
            params = dict(R.reference_params(slice_z), fnt=("global", FNT_T))
            for kb in (-2, 1):                                   # a negative and a positive block row
                for z in (8 * kb - 1, 8 * kb, 8 * kb + 7):
                    params["row%d_%d" % (kb, z)] = ("global", band(SIX["edt"], z, z))
                    params["row%d_%d_t" % (kb, z)] = ("global", band(SIX["ogm"], z, z))
            got = {}
            for name, (_, p) in params.items():
                if name.startswith("loc"):
                    continue
                want = ref.cloud(w, p)
                got[name], count = call(m, "global", p)
                check((k, name), got[name], count, want)         # equal counts: nothing lies outside the box
            loc = m.read_local(dist_sq=False, coc=False)
            for name in ("loc_ogm", "loc_edt"):
                p = params[name][1]
                g, count = call(m, "local", p)
                check((k, name), g, count, R.local_cloud(loc["type"], loc["edt"], tuple(pv), w, p))
            assert len(got["glb_edt"]) > 0 and len(got["row1_8"]) > 0 and len(got["row-2_-16"]) > 0      # one-layer bands with points
            ogm = got["glb_ogm"]
            for ax in "xyz":
                assert (ogm[ax] < 0).any() and (ogm[ax] > 0).any(), (k, ax)
            known = R.global_cloud(ref.rec, ref.xyz, w, R.param(R.KNOWN, R.TYPE))
            full, _ = call(m, "global", SIX["edt"])
            assert len(full) <= len(known), k
            dropped += len(known) - len(full)
            if k + 1 > 1:                                        # points outside the current local volume
                hi = (pv + np.array(size)).astype(np.float32) * np.float32(w)
                assert (ogm["x"] < np.float32(pv[0]) * np.float32(w)).any() or (ogm["x"] >= hi[0]).any(), k
        assert dropped > 0                                       # DIST voxels were dropped for an invalid distance
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. deferred records
def test_global_dist_cloud_reads_deferred_records():
    """The number of tskip tiles is taken from the tile plane debug_tile_state returns: its scalar `tskip_count` is a counter only
    the CPU emulation keeps (GIE_CNT_TSKIP), on the device it is always 0.  On the emulation this drive flags 4 tiles per update."""
    import lazy_bounds as L
    from hooks_py import HooksMapper
    size = (32, 24, 32)
    dr = L.Drive("cloud_32x24x32", size, 6, step=2, turn=20, p_occ=0.03, cutoff_dist=0.6)
    m = HooksMapper(dr.config())
    ref = GlobalRef(size)
    try:
        w = m.cfg.voxel_width
        p = SIX["edt"]
        checked = changed = 0
        prev = None
        for k, pos, q, kind, lab, _ in dr.frames():
            m.set_pose(pos, q)
            m.ogm_labels(lab)
            m.fuse()
            ref.add(m)
            if k == 4:                                           # between gie_fuse and gie_batch_edt, against query_global at the same point
                want = ref.take(m).cloud(w, p)
                got, count = call(m, "global", p)
                check(("after fuse", k), got, count, want)
                assert count > 0
            m.batch_edt()
            m.merge()
            if k < 2:
                continue
            st = m.debug_tile_state()
            n_tskip = int((st["tskip"] != 0).sum())
            assert st["coc_defer"] == 1 and n_tskip > 0, (k, st["coc_defer"], n_tskip)      # otherwise this covers nothing
            got, count = call(m, "global", p)
            st2 = m.debug_tile_state()
            assert (st2["tskip_count"], st2["caught_up"]) == (st["tskip_count"], st["caught_up"]), k            # the call stores nothing
            assert np.array_equal(st2["tskip"], st["tskip"]) and np.array_equal(st2["tlazy"], st["tlazy"])
            check(("deferred", k), got, count, ref.take(m).cloud(w, p))
            checked += 1
            # the voxels of the flagged tiles and their records; a voxel flagged after this update and after the one before has had
            # no record stored by either sweep: where its record changed meanwhile, the stored copy is stale
            tz, ty, tx = np.nonzero(st["tskip"])
            o = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)      # (x, y, z) offsets
            loc = (np.stack([tx, ty, tz], -1)[:, None, :] * 8 + o[None]).reshape(-1, 3)
            loc = loc[(loc < np.array(size)).all(1)]
            g = (loc + np.array(m.pivot())).astype(np.int32)
            cur = {tuple(c): int(d) for c, d in zip(g.tolist(), m.query_global(g)["dist_sq"])}
            if prev is not None:
                changed += sum(1 for c, d in cur.items() if c in prev and prev[c] != d)
            prev = cur
        assert checked == 4
        assert changed > 0                                       # records changed while only the pair plane held them
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. erasure
def test_global_clouds_with_erased_blocks():
    size = (48, 40, 33)
    d = BoxDrive(size, delta=8)
    max_blocks = 400                                             # (240 blocks are live at a time, 990 are handed out over the drive)
    m = mapper(size, retain_radius_blocks=1, max_blocks=max_blocks)
    ref = GlobalRef(size)
    try:
        w = np.float32(m.cfg.voxel_width)
        handed_out, far = 0, None
        for k in range(30):
            update(m, *d.frame(k))
            ref.add(m)
            s = m.stats()
            handed_out += s["blocks_new"]
            assert s["blocks_total"] <= max_blocks
            if k == 14:                                          # the far end of the drive
                far, _ = call(m, "global", R.param(R.KNOWN, R.TYPE))
            if k in (14, 29):
                ref.take(m)
                for name in ("ogm", "edt", "fnt"):
                    got, count = call(m, "global", SIX[name])
                    check((k, name), got, count, ref.cloud(w, SIX[name]))
        assert handed_out > max_blocks, handed_out               # more blocks handed out than the pool has slots: slots were reused
        # a block left behind has vanished: beyond the last volume's retained box the far end's points are gone
        edge = np.float32(m.pivot()[0] + size[0] + 8 * 3) * w
        last, _ = call(m, "global", R.param(R.KNOWN, R.TYPE))
        assert (far["x"] > edge).any() and not (last["x"] > edge).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. capacity
def test_capacity_and_tail_in_both_forms():
    size = (48, 40, 33)
    m = mapper(size)
    try:
        scene(m, size)
        for form in ("local", "global"):
            p = SIX["edt"]
            full, count = call(m, form, p)
            assert count == len(full) > 100
            cp = m.cloud_param(p["type_mask"], p["intensity"], None, None, 0)
            n = C.c_int32(-1)
            assert m._f["cloud_" + form](m._h, C.byref(cp), None, C.byref(n)) == 0 and n.value == count      # NULL out only counts
            members = {r.tobytes() for r in R.canon(full)}
            for cap in (count - 7, count + 9):
                buf = np.frombuffer(bytes([0x5a]) * (16 * (cap + 5)), gie.CLOUD_DTYPE).copy()
                got, c2 = call(m, form, p, max_points=cap, out=buf)
                nw = min(count, cap)
                assert c2 == count and len(got) == nw
                rows = [r.tobytes() for r in R.canon(buf[:nw])]
                assert len(set(rows)) == nw and set(rows) <= members, (form, cap)      # distinct members of the reference set
                assert buf[nw:].tobytes() == bytes([0x5a]) * (16 * (cap + 5 - nw)), (form, cap)      # the tail is intact
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. _dev forms
def test_dev_forms_on_the_mappers_stream():
    import torch
    size = (64, 24, 20)
    m = mapper(size)
    try:
        scene(m, size)
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        for form in ("local", "global"):
            fdev = m.cloud_local_dev if form == "local" else m.cloud_global_dev
            want = {name: call(m, form, SIX[name]) for name in ("ogm", "edt")}
            cap = max(c for _, c in want.values()) + 3
            with torch.cuda.stream(st):
                outs = {}
                for name in ("ogm", "edt"):                      # two calls back to back, no sync in between
                    p = SIX[name]
                    dout = torch.full((cap * 16,), 0x5a, dtype=torch.uint8, device=dev)
                    dcnt = torch.full((1,), 77, dtype=torch.int32, device=dev)
                    fdev(dout.data_ptr(), dcnt.data_ptr(), p["type_mask"], p["intensity"], max_points=cap)
                    outs[name] = (dout, dcnt)
                dcnt_only = torch.full((1,), 77, dtype=torch.int32, device=dev)
                fdev(0, dcnt_only.data_ptr(), SIX["ogm"]["type_mask"], SIX["ogm"]["intensity"], max_points=0)
                dno_count = torch.full((cap * 16,), 0x5a, dtype=torch.uint8, device=dev)
                fdev(dno_count.data_ptr(), 0, SIX["ogm"]["type_mask"], SIX["ogm"]["intensity"], max_points=cap)
            m.sync()
            for name, (dout, dcnt) in outs.items():
                pts, count = want[name]
                raw = dout.cpu().numpy()
                assert int(dcnt.cpu()[0]) == count, (form, name)
                check((form, name), raw[:16 * count].view(gie.CLOUD_DTYPE), count, pts)
                assert raw[16 * count:].tobytes() == bytes([0x5a]) * (16 * (cap - count))
            assert int(dcnt_only.cpu()[0]) == want["ogm"][1]
            assert R.same(dno_count.cpu().numpy()[:16 * want["ogm"][1]].view(gie.CLOUD_DTYPE), want["ogm"][0])
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 7. arguments
def test_invalid_arguments_leave_the_buffers_alone():
    size = (32, 24, 16)
    m, fresh, t = mapper(size), mapper(size), mapper(size)
    try:
        scene(m, size, room=False)
        f = m._f
        buf = np.frombuffer(bytes([0x5a]) * (16 * 64), gie.CLOUD_DTYPE).copy()
        n = C.c_int32(-7)
        ptr = buf.ctypes.data_as(C.c_void_p)

        def P(**kw):
            p = _capi.CloudParam(1 << R.OCCUPIED, R.TYPE, R.NO_BAND[0], R.NO_BAND[1], 64)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p
        bad = [P(type_mask=0), P(type_mask=1), P(type_mask=3), P(type_mask=1 << 4), P(type_mask=0x8000000e), P(intensity=2), P(intensity=-1),
               P(z_lo=5, z_hi=4), P(max_points=-1), P(reserved=0), P(reserved=1), P(reserved=2)]
        for name in ("cloud_local", "cloud_global", "cloud_local_dev", "cloud_global_dev"):
            for p in bad:
                assert f[name](m._h, C.byref(p), ptr, C.byref(n)) == INVALID, (name, p.type_mask, p.intensity, p.z_lo, p.max_points, list(p.reserved))
            assert f[name](m._h, None, ptr, C.byref(n)) == INVALID                       # a NULL param
            assert f[name](m._h, C.byref(P()), None, C.byref(n)) == INVALID              # a NULL out with max_points > 0
            assert f[name](m._h, C.byref(P(max_points=0)), None, None) == INVALID        # nothing to write
            assert f[name](None, C.byref(P()), ptr, C.byref(n)) == INVALID
        assert n.value == -7 and buf.tobytes() == bytes([0x5a]) * (16 * 64)
        assert f["cloud_local"](m._h, C.byref(P()), ptr, C.byref(n)) == 0 and 0 < n.value   # (the same call with good arguments works)
        buf[:] = np.frombuffer(bytes([0x5a]) * (16 * 64), gie.CLOUD_DTYPE)
        n.value = -7
        # a device buffer that is not 16-byte aligned: the _dev forms refuse and write nothing; the host forms take any address
        import torch
        dbuf = torch.full((16 * 64 + 16,), 0x5a, dtype=torch.uint8, device="cuda:0")
        dn = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
        for name in ("cloud_local_dev", "cloud_global_dev"):
            for off in (4, 8, 12):
                assert f[name](m._h, C.byref(P()), C.c_void_p(dbuf.data_ptr() + off), C.c_void_p(dn.data_ptr())) == INVALID, (name, off)
        m.sync()
        assert int(dn.cpu()[0]) == -7 and bool((dbuf == 0x5a).all())
        raw = np.frombuffer(bytes([0x5a]) * (16 * 64 + 16), np.uint8).copy()
        n2 = C.c_int32(0)
        assert f["cloud_global"](m._h, C.byref(P()), C.c_void_p(raw.ctypes.data + 4), C.byref(n2)) == 0 and 0 < n2.value
        k2 = min(n2.value, 64)
        assert raw[:4].tobytes() == b"ZZZZ" and raw[4 + 16 * k2:].tobytes() == bytes([0x5a]) * (16 * 64 + 12 - 16 * k2)
        assert set(r.tobytes() for r in R.canon(raw[4:4 + 16 * k2].copy().view(gie.CLOUD_DTYPE))) <= set(
            r.tobytes() for r in R.canon(m.cloud_global(1 << R.OCCUPIED)[0]))
        # the local form before the first pose; the global form of a fresh mapper counts nothing
        assert f["cloud_local"](fresh._h, C.byref(P()), ptr, C.byref(n)) == INVALID and f["cloud_local_dev"](fresh._h, C.byref(P()), ptr, C.byref(n)) == INVALID
        # a tiled mapper: all four refuse
        t.set_tile((8, 0, 0), (64, 24, 16))
        for name in ("cloud_local", "cloud_global", "cloud_local_dev", "cloud_global_dev"):
            assert f[name](t._h, C.byref(P()), ptr, C.byref(n)) == INVALID, name
        assert n.value == -7 and buf.tobytes() == bytes([0x5a]) * (16 * 64)
        assert f["cloud_global"](fresh._h, C.byref(P()), ptr, C.byref(n)) == 0 and n.value == 0      # an empty pool
        assert buf.tobytes() == bytes([0x5a]) * (16 * 64)
    finally:
        for x in (m, fresh, t):
            x.close()


# ---------------------------------------------------------------------------------------------------------- 8. the update does not notice
def _all_four(m, slice_z):
    for form, p in R.reference_params(slice_z).values():
        call(m, form, p)


def test_cloud_calls_change_nothing_of_the_map_update():
    size = (48, 40, 33)
    d = BoxDrive(size, seed=5)

    def calls(a, k, phase, pos):
        if phase == "fuse":
            _all_four(a, 2)                                      # between fuse and merge
        elif phase == "merge":
            _all_four(a, -3)
    stage_calls_change_nothing(size, (d.frame(k) for k in range(10)), mapper, calls)


# ---------------------------------------------------------------------------------------------------------- 9. profile
def test_profile_counts_the_calls():
    size = (32, 24, 16)
    m = mapper(size)
    try:
        scene(m, size, room=False)
        m.profile_enable(True)
        m.profile_read()
        p = SIX["ogm"]
        m.cloud_local(p["type_mask"], max_points=10)
        m.cloud_global(p["type_mask"], max_points=10)
        m.cloud_global(p["type_mask"], z_lo=10 ** 6, z_hi=10 ** 6, max_points=0)
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["cloud"][1] == 3 and prof["cloud"][0] > 0
        names = list(prof)
        assert names[-2:] == ["sdf", "sdf_query"] and names.index("cloud") == names.index("los") - 1 and names[0] == "ogm_classify"
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 10. host layer
def test_host_layer_visualize_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "cloud_host_probe")
    size, w, cutoff, vis_height = (48, 40, 33), 0.1, 3.0, -0.3
    frames, fpath = lidar_frames(tmp_path)
    m = mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.set_ext_boxes(np.array([[-3.6, -3.2, 0.2]], np.float32), np.array([[4.4, 3.4, 2.6]], np.float32), np.zeros(1, np.uint8))
            m.fuse(); m.batch_edt(); m.merge()
        want = {name: call(m, form, p)[0] for name, (form, p) in R.reference_params(scenes.pos2coord(vis_height, w)).items()}
    finally:
        m.close()
    assert all(len(v) > 0 for v in want.values()), {k: len(v) for k, v in want.items()}
    for mirror in ("0", "1"):                                    # the stream off and the clouds from the device; the mirror's loops
        out = str(tmp_path / ("clouds" + mirror))
        res = subprocess.run([exe, fpath, out, mirror, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff), repr(vis_height)],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert ("mirror_blocks 0 " in res.stdout) == (mirror == "0"), res.stdout
        for name, pts in want.items():
            got = np.fromfile(out + "." + name, gie.CLOUD_DTYPE)
            assert len(got) == len(pts) and R.same(got, pts), (mirror, name, len(got), len(pts))

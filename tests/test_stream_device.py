"""The changed-block stream (gie_stream_enable / gie_stream_changed) as its consumer sees it — the CPU mirror of the global map — on
drives with a turn, with the stream switched on and off between updates, with block erasure, with partial drains, and with a drain
that comes late, after fused updates have left records to the pair plane ("deferred records").  The invariants I1 - I5
are tests/stream_mirror.py's.  Every case runs twice from one table: on the sequential emulation of the device logic (the non-GPU
suite) and on the device, whose flag sites in k_fuse_rows, k_markc and the write-backs of waves A / B the emulation does not run."""
import numpy as np
import pytest

import gie
import parity
import stream_mirror as sm
from emu_py import EmuMapper
from oracle_py import OracleMapper
from parity import Scenario
from test_host_logic import SCENARIOS


def _hash_drive(name, frames, delta_vox=3, turn=0):
    """the hash world (scenes.hash_world_labels: full observation, a quarter of the obstacles toggling) in a volume of 64 x 48 x 40
    at 0.1 m, driven along x: the smallest in which fused updates defer records and leave tiles lazy"""
    return Scenario(name, (64, 48, 40), voxel=0.1, sensor="labels", seed=5, p_occ=0.01, toggle=0.25, delta_vox=delta_vox, yaw_deg=0.0,
                    cutoff_dist=2.0, fast_mode=False, frames=frames, turn=turn)


def _named(name, **kw):
    sc = [s for s in SCENARIOS if s.name == name][0]
    return Scenario(**dict(sc.__dict__, **kw))


def _update(m, frame, snapshot=None):
    pos, q, kind, data, kw = frame
    m.set_pose(pos, q)
    snap = snapshot(m) if snapshot else None
    parity._feed(m, kind, data, kw)
    m.fuse(); m.batch_edt(); m.merge()
    return snap


def _probes(sc, prev_pvt, pvt, rng, n):
    xyz = parity.probe_coords(pvt, sc.size, rng, n=n, margin=sc.probe_margin)
    if prev_pvt is not None:
        xyz = np.concatenate([xyz, parity.probe_left_behind(prev_pvt, pvt, sc.size, rng, n=n // 4)])
    return xyz


def _figures(name, fig):
    print("stream figures %s: %s" % (name, " ".join("%s=%s" % kv for kv in fig.items())))


# ---- A - D: a drive, both mappers in step, full drains
def run_drive(make, sc, on=None, i3=False, i4=False, control=False, need_outside=False, probes=4000):
    """on: the updates that run with the stream on (None: all of them).  Stream-on updates: I1, I2 (and I3); stream-off updates:
    I5, nothing new is flagged.  i4: the mirror after every update (only sensible with on=None), erased by the retention rule where
    the scenario retains; control: a second mirror that never erases must then go stale."""
    cfg = sc.config()
    a, o = make(cfg), OracleMapper(cfg)
    rng = np.random.default_rng(sc.seed + 79)
    mirror, never_erased = sm.Mirror(), sm.Mirror()
    drain_a, drain_o = sm.Drain(a, sc.name), sm.Drain(o, sc.name + " (oracle)")
    fig = dict(on_updates=0, flagged=0, changed=0, missed=0, extra=0, outside=0, visits_ab=0, stale=0)
    if not i3:
        fig["changed"] = fig["missed"] = fig["extra"] = "unchecked"
    prev = None
    try:
        if sc.ext_boxes:
            parity.set_ext_boxes(a, o)
        for k, frame in enumerate(sc.frames_iter()):
            is_on = on is None or k in on
            tag = "%s update %d" % (sc.name, k)
            drain_a.tag, drain_o.tag = tag, tag + " (oracle)"
            pending = [m.stream_count() for m in (a, o)]
            for m in (a, o):
                m.stream_enable(is_on)
            snap = _update(a, frame, (lambda m: sm.Snapshot(m, m.pivot(), sc.size)) if (i3 and is_on) else None)
            _update(o, frame)
            pvt = a.pivot()
            assert pvt == o.pivot()
            drain_a.updated(); drain_o.updated()
            if is_on:
                ka, ba = drain_a()
                ko, bo = drain_o()
                fig["on_updates"] += 1
                fig["flagged"] += len(ka)
                fig["outside"] += sm.outside_volume(ko, pvt, sc.size)
                st = o.stats()
                fig["visits_ab"] += st["visits_a"] + st["visits_b"]
                sm.check_oracle_equal(tag, (ka, ba), (ko, bo))
                sm.check_content(tag, a, ka, ba)
                if i3:
                    changed, extra = sm.check_complete(tag, a, snap, ka)
                    fig["changed"] += changed
                    fig["extra"] += extra
                mirror.feed(ka, ba)
                never_erased.feed(ka, ba)
            else:
                for m, p in zip((a, o), pending):
                    sm.check_not_grown(tag, m, p)
            if sc.retain:
                mirror.erase(pvt, sc.size, sc.retain)
            if i4:
                xyz = _probes(sc, prev, pvt, rng, probes)
                sm.check_mirror(tag, a, mirror, xyz)
                if control:
                    fig["stale"] += sm.mirror_mismatches(a, never_erased, xyz)[0]
            prev = pvt
    finally:
        a.close()
        o.close()
    _figures(sc.name, fig)
    assert fig["flagged"] > 0
    if need_outside:                   # the scene reaches the flag sites of waves A / B: blocks outside the volume
        assert fig["visits_ab"] > 0 and fig["outside"] > 0, fig
    if control:                        # the drive erases blocks the mirror holds
        assert fig["stale"] > 0, fig
    return fig


# ---- E: partial drains between the updates
def run_partial(make, sc, probes=8000):
    a = make(sc.config())
    rng = np.random.default_rng(sc.seed + 80)
    mirror, drain = sm.Mirror(), sm.Drain(a, sc.name)
    fig = dict(calls=0, delivered_min=None, delivered_max=0, left_min=None, left_max=0)
    prev = pvt = None
    try:
        a.stream_enable(True)
        for k, frame in enumerate(sc.frames_iter()):
            drain.tag = "%s update %d" % (sc.name, k)
            _update(a, frame)
            drain.updated()
            prev, pvt = pvt, a.pivot()
            pending = a.stream_count()
            keys, blocks = drain(max(1, pending // 3))
            sm.check_content(drain.tag, a, keys, blocks)
            left = pending - len(keys)
            fig["calls"] += 1
            fig["delivered_min"] = len(keys) if fig["delivered_min"] is None else min(fig["delivered_min"], len(keys))
            fig["left_min"] = left if fig["left_min"] is None else min(fig["left_min"], left)
            fig["delivered_max"], fig["left_max"] = max(fig["delivered_max"], len(keys)), max(fig["left_max"], left)
            # (a second call without an update in between: nothing comes twice)
            if k % 4 == 1:
                k2, b2 = drain(2)
                sm.check_content(drain.tag + " second call", a, k2, b2)
                mirror.feed(k2, b2)
            mirror.feed(keys, blocks)
            mirror.erase(pvt, sc.size, sc.retain)
        drain.tag = sc.name + " last drain"
        keys, blocks = drain()
        sm.check_content(drain.tag, a, keys, blocks)
        assert a.stream_count() == 0
        mirror.feed(keys, blocks)
        mirror.erase(pvt, sc.size, sc.retain)
        sm.check_mirror(drain.tag, a, mirror, _probes(sc, prev, pvt, rng, probes))
    finally:
        a.close()
    _figures(sc.name + " partial", fig)
    assert fig["left_max"] > 0          # the drains were partial
    return fig


# ---- F: a late drain, after fused updates
def _on_deferred_tiles(keys, pivot, ts):
    """how many of the blocks overlap a tile of the last update whose records or pairs are deferred (tskip / tlazy, [tz][ty][tx])"""
    flag = (ts["tskip"] != 0) | (ts["tlazy"] != 0)
    n = 0
    for key in keys.tolist():
        sl = []
        for i in range(3):                                  # axis i of the key is axis 2 - i of the planes
            lo = 8 * key[i] - int(pivot[i])                  # the block's first voxel, local
            t0, t1 = max(lo >> 3, 0), min((lo + 7) >> 3, flag.shape[2 - i] - 1)
            sl.append(slice(t0, t1 + 1))
        n += bool(flag[sl[2], sl[1], sl[0]].any())
    return n


def run_late(make, L, drain_first):
    """updates 0 - 2 with the stream off, update 3 with it on, (drain_first: five blocks delivered,) the stream switched off, L fused
    updates, then the drain: the flags have outlived updates that left records to the pair plane, and what is delivered must still
    be what gie_query_global returns (I2) and what the oracle delivers (I1; not after the first drain, since the two mappers need
    not pick the same five blocks)."""
    sc = _hash_drive("late_drain_L%d%s" % (L, "_after_5" if drain_first else ""), frames=4 + L)
    cfg = sc.config()
    a, o = make(cfg), OracleMapper(cfg)
    drain_a, drain_o = sm.Drain(a, sc.name), sm.Drain(o, sc.name + " (oracle)")
    fig = dict(L=L)
    try:
        for k, frame in enumerate(sc.frames_iter()):
            pending = [m.stream_count() for m in (a, o)]
            for m in (a, o):
                m.stream_enable(k == 3)
                _update(m, frame)
            drain_a.updated(); drain_o.updated()
            if k == 3:
                fig["flagged"] = a.stream_count()
                assert fig["flagged"] == o.stream_count() > 5
                if drain_first:
                    keys, blocks = drain_a(5)
                    sm.check_content("%s first drain" % sc.name, a, keys, blocks)
            else:
                for m, p in zip((a, o), pending):
                    sm.check_not_grown("%s update %d" % (sc.name, k), m, p)
        ts = a.debug_tile_state()
        keys, blocks = drain_a()
        # tskip_count: the tiles whose records the last update left to the pair plane, counted on the tskip plane (the scalar of that
        # name is a counter only the emulation keeps: the device leaves it 0)
        fig["drained"], fig["coc_defer"], fig["tskip_count"] = len(keys), ts["coc_defer"], int((ts["tskip"] != 0).sum())
        fig["lazy_tiles"] = int((ts["tlazy"] != 0).sum())
        fig["on_deferred_tiles"] = _on_deferred_tiles(keys, a.pivot(), ts)
        fig["blocks_differing"], fig["voxels_differing"], first = sm.content_mismatch(a, keys, blocks)
        _figures(sc.name, fig)
        assert fig["blocks_differing"] == 0, "%s: I2 %d of %d blocks drained late (%d voxels) differ from query_global; first %s" % (
            sc.name, fig["blocks_differing"], len(keys), fig["voxels_differing"], first)
        if not drain_first:
            sm.check_oracle_equal(sc.name, (keys, blocks), drain_o())
        if L >= 3:                     # the scene: the late drain meets deferred records
            assert fig["coc_defer"] == 1 and fig["tskip_count"] > 0 and fig["on_deferred_tiles"] > 0, fig
    finally:
        a.close()
        o.close()
    return fig


# ---- the table: (id, needs the test build on the device, runner)
def _case_a(make):
    run_drive(make, _hash_drive("drive_turn", frames=12, turn=8), i3=True, i4=True, need_outside=True)


def _case_b_uneven(make):
    run_drive(make, parity.UNEVEN_DRIVES[2], i4=True)


def _case_b_boxes(make):
    run_drive(make, _named("planner_boxes"))


def _case_c(delta_vox, on):
    def run(make):
        fig = run_drive(make, _hash_drive("toggle_d%d_on_%s" % (delta_vox, "_".join(map(str, on))), frames=12, delta_vox=delta_vox, turn=8),
                        on=set(on), i3=True)
        assert fig["on_updates"] == len(on)
    return run


def _case_d_c5(make):
    run_drive(make, _named("retain_c5_out_and_back", frames=20), i4=True, control=True, probes=8000)


def _case_d_odd(make):
    run_drive(make, _named("retain_odd_r1"), i4=True, control=True, probes=8000)


def _case_e(make):
    run_partial(make, _named("retain_odd_r1"))


def _case_f(L, drain_first):
    return lambda make: run_late(make, L, drain_first)


CASES = [("A-drive_turn", False, _case_a), ("B-uneven_mixed", False, _case_b_uneven), ("B-planner_boxes", False, _case_b_boxes)]
CASES += [("C-toggle-d%d-on%s" % (d, "_".join(map(str, on))), False, _case_c(d, on)) for d in (3, 5) for on in ((4,), (3, 7), (2, 3, 9))]
CASES += [("D-retain_c5", False, _case_d_c5), ("D-retain_odd_r1", False, _case_d_odd), ("E-partial_drains", True, _case_e)]
CASES += [("F-late-L%d-%s" % (L, "after_5" if first else "first_drain"), True, _case_f(L, first)) for L in (2, 3, 5) for first in (False, True)]
_IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_stream_emulation(oracle_lib, monkeypatch, case):
    monkeypatch.setenv("GIE_STREAM_CHUNK_BLOCKS", "3")        # (several trips through the staging buffers per call)
    case[2](EmuMapper)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_stream_device(oracle_lib, monkeypatch, case):
    if case[1]:                                                # the staging switch and gie_debug_tile_state exist in the test build only
        from hooks_py import HooksMapper
        monkeypatch.setenv("GIE_STREAM_CHUNK_BLOCKS", "3")
        case[2](HooksMapper)
    else:
        case[2](gie.Mapper)

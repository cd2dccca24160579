"""The lazy tiles' distance bounds on the device, checked at the map update that writes them (lazy_bounds.check_update), on long
drives with turns in volumes where pass Z's streaming form takes the volume (Z >= 64, more than GIE_BAND_MAXK planes with obstacles,
swept).  HooksMapper (the test build, for gie_debug_tile_state) against the oracle: after every update the local planes, the stats
and global probes in and around the volume and in the slabs just left bit for bit, then (a) stored records within their tile's
bound, (b) lazy tiles bounded above their true batch distances, (c) tbmax exact below 81 and "81 or more" in given-up slabs.

* even X, the fused form: the hash world with the bench's out-and-back drive, a pocket without obstacles on the way (wide trips,
  slabs given up), unobserved slabs, a jump off the block grid before the turn, an update in the reference's order of kernels
  (stream_enable) and two ray-cast scans between label updates;
* odd X, the unfused streaming form (the launch plan, gie_edt_plan_for, goes by X's parity): slow steps of 0-1 voxels and jumps of 6-9 in both directions;
* the bound's edge values: a constructed field whose tiles' largest batch distance^2 are exactly 64, 80, 81 and 82, with a pocket
  that makes slabs give up before their last trip (tiles of true 82 left with the give-up's "81 or more").
Each drive shows from the hook's counters and arrays that the paths it is about ran."""
import time

import numpy as np
import pytest

import lazy_bounds as L

pytestmark = pytest.mark.gpu


def _odd_path(n, turn):
    """slow steps (0-1 voxel, now and then one in y or z) and jumps of 6-9 voxels, out along +x and back after `turn` updates"""
    out = []
    for k in range(1, n):
        s = 1 if k <= turn else -1
        if k % 6 == 0:
            out.append((s * (6 + k % 4), (-1) ** k * (k % 9), (-1) ** (k // 6) * (k % 7)))
        else:
            out.append((s * (k % 2), 1 if k % 5 == 1 else 0, -1 if k % 7 == 3 else 0))
    return out


DRIVES = {
    "fused_128x96x192": L.Drive("fused_128x96x192", (128, 96, 192), 56, turn=24, jump={21: (19, -13, 6)}, pocket=((150, -30, -40), 56),
                                unobserved={3: (8, 20), 9: (30, 44), 27: (70, 90), 40: (8, 30)}, stream_on=(12,), lidar=(33, 34),
                                definition_at=(20, 55)),
    "unfused_137x120x176": L.Drive("unfused_137x120x176", (137, 120, 176), 52, path=_odd_path(52, 25), pocket=((-20, -20, -20), 56),
                                   unobserved={4: (10, 25), 31: (90, 110)}, seed=9, definition_at=(51,)),
    "edge_128x96x192": L.Drive("edge_128x96x192", (128, 96, 192), 50, path=[(0, 0, 0)] * 3 + [((1, 0, -1, 0)[k % 4], 0, 0) for k in range(46)],
                               field=L.edge_field(y0=-48), pocket=((0, -36, -32), (64, 32, 48)), definition_at=(49,)),
}


def _run(name):
    from hooks_py import HooksMapper
    from oracle_py import OracleMapper
    dr = DRIVES[name]
    t0 = time.time()
    tally = L.run_checked_drive(dr, OracleMapper, HooksMapper, definition=dr.definition_at)
    print("%s: %d updates in %.1f s" % (name, dr.updates, time.time() - t0))
    return dr, tally


def _streamed_wide_given_up(tally):
    assert tally.total("zstream") > 0 and tally.total("zwide") > 0 and tally.total("zfail") > 0, tally.updates
    assert tally.total("redo81") > 0


def test_fused_form_drive(oracle_lib):
    dr, tally = _run("fused_128x96x192")
    _streamed_wide_given_up(tally)
    # lazy tiles bounded by pass Z's record (<= 80) and by samples both occur; tiles flagged 2 and catch-ups after the jump and the turn
    assert tally.total("lazy_exact") > 0 and tally.total("lazy_sampled") > 0, tally.updates
    jump = min(dr.jump)
    for after in (jump, dr.turn):
        assert tally.total("skip2", after=after) > 0 and tally.total("caught_up", after=after) > 0, (after, tally.updates)


def test_unfused_form_drive(oracle_lib):
    dr, tally = _run("unfused_137x120x176")
    _streamed_wide_given_up(tally)
    assert tally.total("lazy_exact") > 0, tally.updates
    assert tally.total("skip2", after=25) > 0 and tally.total("caught_up", after=25) > 0, tally.updates


def test_edge_values_of_the_bound(oracle_lib):
    from gie import scenes
    dr = DRIVES["edge_128x96x192"]
    # the field is what it claims: tiles whose largest batch distance^2 is exactly 64, 80, 81 and 82
    pos = (np.float32(0), np.float32(0), np.float32(0))
    lab = dr.labels(0, scenes.local_pivot(pos, dr.voxel, dr.size))
    tm = L.tile_max(L.host_batch_edt(lab))
    assert {64, 80, 81, 82} <= set(np.unique(tm).tolist())
    dr, tally = _run("edge_128x96x192")
    _streamed_wide_given_up(tally)
    assert tally.total("lazy_exact") > 0 and tally.total("lazy_sampled") > 0, tally.updates

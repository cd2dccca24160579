"""The CPU tier of test_lazy_bounds.py: the same drive generator on the sequential emulation (tests/emu), against the oracle, with
checks (a) and (b) of lazy_bounds.check_update after every update.  The emulation bounds its tiles through the ordinary sweep
(be_markc: GIE_CNT_LAZY_EXACT = 1, no streaming pass Z), so this tier holds the bookkeeping half of the checker: the bounds
gie_markc_column records (gie_ops.h, shared with the device) and what gie_tile_oldskip builds on them across a turn, a jump off the
block grid, an update in the reference's order of kernels and a switch of sensor."""
import pytest

import lazy_bounds as L

DRIVES = {
    "40x29x40": L.Drive("cpu_40x29x40", (40, 29, 40), 48, step=3, turn=20, jump={17: (19, -13, 6)}, pocket=((30, 2, -6), 14),
                        unobserved={5: (8, 14), 23: (20, 27)}, stream_on=(12,), lidar=(30, 31), p_occ=0.02, cutoff_dist=1.0),
    "64x64x64": L.Drive("cpu_64x64x64", (64, 64, 64), 48, step=4, turn=24, jump={21: (19, -13, 6)}, pocket=((60, 10, -10), 24),
                        unobserved={7: (8, 20), 33: (40, 50)}, stream_on=(14,), lidar=(36, 37)),
}


@pytest.mark.parametrize("name", sorted(DRIVES))
def test_emulated_drive_bounds(oracle_lib, name):
    from emu_py import EmuMapper
    from oracle_py import OracleMapper
    dr = DRIVES[name]
    tally = L.run_checked_drive(dr, OracleMapper, EmuMapper, brute_pin=True, definition=(dr.updates - 1,))
    # what the drive is about happened: tiles flagged 2 (deferred records) and lazy tiles, also after the jump and after the turn
    jump = min(dr.jump)
    assert tally.total("skip2", after=jump) > 0 and tally.total("skip2", after=dr.turn) > 0
    assert tally.total("lazy_sampled", after=jump) > 0 and tally.total("lazy_sampled", after=dr.turn) > 0      # (no streaming pass Z here)

"""What a consumer of the changed-block stream (gie_stream_enable / gie_stream_changed) may rely on, as checks in plain numpy: a
mirror of the global map fed by nothing but the stream, and five invariants that raise AssertionError with counts and the first
offender.  No tests in here (tests/test_stream_device.py, parity.run_irregular).

I1 oracle equality   two mappers driven by the same calls with full drains deliver the same blocks, byte for byte
I2 content           a delivered block is what gie_query_global returns for its 512 voxels right after the call
I3 completeness      a block in which a voxel's type, distance or closest obstacle changed over an update is flagged
I4 mirror            the mirror (defaults where it holds no block) agrees with gie_query_global
I5 accounting        no key twice, the count goes down by what was delivered, nothing is flagged while the stream is off"""
import numpy as np

from gie.mapper import VOXEL_DTYPE

UNKNOWN = 0
EMPTY_VALUE = 999999            # a voxel no block holds: (UNKNOWN, EMPTY_VALUE, EMPTY_KEY = three times EMPTY_VALUE)
RECORD = ("vox_type", "dist_sq", "coc")          # what the flags follow (include/gie.h: "type, distance or closest obstacle")

_J = np.arange(512)
_IN_BLOCK = np.stack([_J >> 6, (_J >> 3) & 7, _J & 7], axis=-1).astype(np.int32)       # get_voxID_in_VB = (x&7)*64 + (y&7)*8 + (z&7)


def block_voxels(key):
    """the 512 global coordinates of block `key`, in the order of a delivered block (int32 [512, 3])"""
    return np.asarray(key, np.int32).reshape(1, 3) * 8 + _IN_BLOCK


def blocks_voxels(keys):
    """block_voxels of n keys at once: int32 [n, 512, 3]"""
    return np.asarray(keys, np.int32).reshape(-1, 1, 3) * 8 + _IN_BLOCK[None]


def key_set(keys):
    return {tuple(k) for k in np.asarray(keys).reshape(-1, 3).tolist()}


def _differs(a, b):
    """per record: does a differ from b in type, distance or closest obstacle"""
    return (a["vox_type"] != b["vox_type"]) | (a["dist_sq"] != b["dist_sq"]) | (a["coc"] != b["coc"]).any(-1)


class Mirror:
    """key -> the block as it was last delivered"""

    def __init__(self):
        self.blocks = {}

    def feed(self, keys, blocks):
        for k, b in zip(np.asarray(keys).reshape(-1, 3).tolist(), blocks):
            self.blocks[tuple(k)] = b.copy()

    def erase(self, pivot, size, R):
        """retain_radius_blocks = R (include/gie.h): the blocks more than R blocks outside the block box of the volume at `pivot`
        widened by a voxel (vb_lo / vb_hi of gie_set_pose) are gone; returns how many the mirror held"""
        lo = [((int(pivot[i]) - 1) >> 3) - R for i in range(3)]
        hi = [((int(pivot[i]) + int(size[i])) >> 3) + R for i in range(3)]
        gone = [k for k in self.blocks if any(k[i] < lo[i] or k[i] > hi[i] for i in range(3))]
        for k in gone:
            del self.blocks[k]
        return len(gone)

    def lookup(self, xyz):
        """the mirror's records of global voxels (VOXEL_DTYPE [n]); the defaults where it holds no block"""
        xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
        out = np.zeros(len(xyz), VOXEL_DTYPE)
        out["vox_type"], out["dist_sq"], out["coc"] = UNKNOWN, EMPTY_VALUE, EMPTY_VALUE
        if len(xyz) == 0:
            return out
        ukeys, inv = np.unique(xyz >> 3, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        order = np.argsort(inv, kind="stable")                      # the probes block by block
        start = np.searchsorted(inv[order], np.arange(len(ukeys) + 1))
        j = (xyz[:, 0] & 7) * 64 + (xyz[:, 1] & 7) * 8 + (xyz[:, 2] & 7)
        for u, k in enumerate(ukeys.tolist()):
            blk = self.blocks.get(tuple(k))
            if blk is not None:
                sel = order[start[u]:start[u + 1]]
                out[sel] = blk[j[sel]]
        return out


# ---- I1
def check_oracle_equal(tag, got, want):
    """got / want: (keys, blocks) of two mappers after the same calls"""
    da = {tuple(k): b for k, b in zip(got[0].tolist(), got[1])}
    db = {tuple(k): b for k, b in zip(want[0].tolist(), want[1])}
    only_a, only_b = sorted(set(da) - set(db)), sorted(set(db) - set(da))
    assert not only_a and not only_b, "%s: I1 key sets differ: %d delivered, the oracle %d; %d only here (first %s), %d only there (first %s)" % (
        tag, len(da), len(db), len(only_a), only_a[:1], len(only_b), only_b[:1])
    bad = [k for k in sorted(da) if da[k].tobytes() != db[k].tobytes()]
    if bad:
        a, b = da[bad[0]], db[bad[0]]
        j = int(np.nonzero(a.view(np.uint8).reshape(512, -1) != b.view(np.uint8).reshape(512, -1))[0][0])
        raise AssertionError("%s: I1 %d of %d blocks differ from the oracle's; first block %s voxel %d: %s, the oracle %s" % (
            tag, len(bad), len(da), bad[0], j, a[j], b[j]))


# ---- I2
def content_mismatch(m, keys, blocks):
    """(blocks differing from query_global, voxels differing, first offender or None)"""
    if len(keys) == 0:
        return 0, 0, None
    g = m.query_global(blocks_voxels(keys).reshape(-1, 3)).reshape(len(keys), 512)
    bad = _differs(blocks, g) | (blocks["occ_val"] != g["occ_val"])
    if not bad.any():
        return 0, 0, None
    b, j = [int(v[0]) for v in np.nonzero(bad)]
    first = "block %s voxel %d: delivered %s, query_global %s" % (tuple(keys[b].tolist()), j, blocks[b, j], g[b, j])
    return int(bad.any(-1).sum()), int(bad.sum()), first


def check_content(tag, m, keys, blocks):
    nb, nv, first = content_mismatch(m, keys, blocks)
    assert nb == 0, "%s: I2 %d of %d delivered blocks (%d voxels) differ from query_global; first %s" % (tag, nb, len(keys), nv, first)


# ---- I3
def volume_block_box(pivot, size, widen=0):
    """(lo, hi) block coordinates, inclusive, of the volume at `pivot`, `widen` blocks more on every side"""
    lo = np.array([int(pivot[i]) >> 3 for i in range(3)]) - widen
    hi = np.array([(int(pivot[i]) + int(size[i]) - 1) >> 3 for i in range(3)]) + widen
    return lo, hi


def outside_volume(keys, pivot, size):
    """how many of `keys` lie outside the volume's block box"""
    if len(keys) == 0:
        return 0
    lo, hi = volume_block_box(pivot, size)
    k = np.asarray(keys).reshape(-1, 3)
    return int(((k < lo) | (k > hi)).any(-1).sum())


class Snapshot:
    """every record of the volume's block box widened by 3 blocks, read through query_global"""

    def __init__(self, m, pivot, size, widen=3):
        lo, hi = volume_block_box(pivot, size, widen)
        ax = [np.arange(lo[i], hi[i] + 1) for i in range(3)]
        self.keys = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
        self.rec = m.query_global(blocks_voxels(self.keys).reshape(-1, 3)).reshape(len(self.keys), 512)


def check_complete(tag, m, before, flagged_keys):
    """`before`: Snapshot taken after set_pose and before the scan was fed; now, after the merge.  Returns (changed blocks, extras:
    flagged without a changed voxel in the box)."""
    after = Snapshot.__new__(Snapshot)
    after.keys = before.keys
    after.rec = m.query_global(blocks_voxels(before.keys).reshape(-1, 3)).reshape(len(before.keys), 512)
    ch = _differs(before.rec, after.rec)
    changed = key_set(before.keys[ch.any(-1)])
    flagged = key_set(flagged_keys)
    missed = sorted(changed - flagged)
    if missed:
        b = int(np.nonzero((before.keys == np.array(missed[0], np.int32)).all(-1))[0][0])
        j = int(np.nonzero(ch[b])[0][0])
        raise AssertionError("%s: I3 %d of %d changed blocks were not flagged (%d flagged); first %s voxel %d: %s -> %s" % (
            tag, len(missed), len(changed), len(flagged), missed[0], j, before.rec[b, j], after.rec[b, j]))
    return len(changed), len(flagged - changed)


# ---- I4
def mirror_mismatches(m, mirror, xyz):
    """(probes at which the mirror disagrees with query_global, first offender or None)"""
    if len(xyz) == 0:
        return 0, None
    g, v = m.query_global(xyz), mirror.lookup(xyz)
    bad = _differs(v, g)
    if not bad.any():
        return 0, None
    i = int(np.nonzero(bad)[0][0])
    return int(bad.sum()), "voxel %s: mirror %s (%s), query_global %s" % (
        tuple(xyz[i].tolist()), v[i], "held" if tuple((xyz[i] >> 3).tolist()) in mirror.blocks else "no block", g[i])


def check_mirror(tag, m, mirror, xyz):
    n, first = mirror_mismatches(m, mirror, xyz)
    assert n == 0, "%s: I4 the mirror disagrees with query_global at %d of %d probes; first %s" % (tag, n, len(xyz), first)


# ---- I5
class Drain:
    """gie_stream_changed of one mapper with its accounting checked at every call"""

    def __init__(self, m, tag):
        self.m, self.tag, self.since_update = m, tag, set()

    def updated(self):
        """a map update has run: a block may be flagged again"""
        self.since_update = set()

    def __call__(self, max_blocks=None):
        before = self.m.stream_count()
        keys, blocks, total = self.m.stream_changed(max_blocks)
        after = self.m.stream_count()
        want = before if max_blocks is None else min(before, int(max_blocks))
        ks = key_set(keys)
        assert total == before and len(keys) == want, "%s: I5 %d flagged, %d reported, %d delivered of %d asked for" % (
            self.tag, before, total, len(keys), want)
        assert len(ks) == len(keys), "%s: I5 %d keys delivered twice in one call" % (self.tag, len(keys) - len(ks))
        assert after == before - len(keys), "%s: I5 %d flagged before the call, %d delivered, %d flagged after" % (
            self.tag, before, len(keys), after)
        again = sorted(ks & self.since_update)
        assert not again, "%s: I5 %d keys delivered again without an update in between; first %s" % (self.tag, len(again), again[0])
        self.since_update |= ks
        return keys, blocks


def check_not_grown(tag, m, before):
    """after an update with the stream off: nothing new is flagged"""
    now = m.stream_count()
    assert now <= before, "%s: I5 %d blocks flagged before a stream-off update, %d after" % (tag, before, now)
    return now

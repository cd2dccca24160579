"""numpy reference of the global block summaries (include/gie.h "global block summaries"): from the gie_query_global records of a box
of global voxels that is aligned to blocks, the gie_block_summary records — canonically sorted by key (z, y, x) — and the grid.
Every value is an integer, so a device result and its reference are equal byte for byte once both are sorted."""
import numpy as np

BLOCK_SUMMARY_DTYPE = np.dtype([("key", "<i4", (3,)), ("n_free", "<u2"), ("n_occupied", "<u2"), ("n_fnt", "<u2"), ("fnt_voxel", "<u2"), ("free_voxel", "<u2"),
                                ("flags", "<u2"), ("min_dist_sq", "<i4"), ("reserved", "<i4")])
UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
DIST = 1                                # GIE_BLOCKS_DIST
OPEN = (-2 ** 31, 2 ** 31 - 1)
DIST_END = 900000                       # the display clouds' validity test: 0 <= dist_sq < 900000
EMPTY_VALUE = 999999                    # GIE_EMPTY_VALUE
NONE = 0xffff


def box_coords(lo, hi):
    """every global voxel of the box [lo, hi) (int32, n x 3), x fastest"""
    gz, gy, gx = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], -1).astype(np.int32)


def block_table(vox_type, dist_sq, vlo, vhi):
    """the voxels of the box [vlo, vhi) (multiples of 8; one entry per voxel in box_coords' order) by block:
    (keys [nb, 3], types [nb, 512], dist_sq [nb, 512]) with the in-block index (x & 7) * 64 + (y & 7) * 8 + (z & 7)"""
    vlo, vhi = np.asarray(vlo, np.int64), np.asarray(vhi, np.int64)
    assert (vlo % 8 == 0).all() and (vhi % 8 == 0).all() and (vhi > vlo).all()
    nb = (vhi - vlo) // 8                                        # blocks along x, y, z
    blo = vlo >> 3

    def by_block(a):
        a = np.asarray(a).reshape(nb[2], 8, nb[1], 8, nb[0], 8)  # bz, z, by, y, bx, x
        return a.transpose(0, 2, 4, 5, 3, 1).reshape(-1, 512)    # (bz, by, bx) x (x, y, z)
    kz, ky, kx = np.meshgrid(np.arange(nb[2]) + blo[2], np.arange(nb[1]) + blo[1], np.arange(nb[0]) + blo[0], indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], -1).astype(np.int32)
    return keys, by_block(vox_type).astype(np.int64), by_block(dist_sq).astype(np.int64)


def _least(mask):
    idx = np.where(mask, np.arange(512)[None, :], NONE)
    return idx.min(1).astype(np.uint16)


def _box(lo, hi):
    lo = [OPEN[0] if lo is None or lo[k] is None else int(lo[k]) for k in range(3)]
    hi = [OPEN[1] if hi is None or hi[k] is None else int(hi[k]) for k in range(3)]
    return np.array(lo, np.int64), np.array(hi, np.int64)


def summaries(table, flags=0, min_fnt=0, lo=None, hi=None, for_grid=False):
    """the records of the qualifying blocks (a known voxel, inside lo..hi) with n_fnt >= min_fnt, sorted by key (z, y, x)"""
    keys, ty, d = table
    lo, hi = _box(lo, hi)
    out = np.zeros(len(keys), BLOCK_SUMMARY_DTYPE)
    out["key"] = keys
    out["n_free"], out["n_occupied"], out["n_fnt"] = (ty == FREE).sum(1), (ty == OCCUPIED).sum(1), (ty == FNT).sum(1)
    out["fnt_voxel"] = _least(ty == FNT)
    passable = (ty == FREE) | (ty == FNT)
    out["free_voxel"] = _least(passable)
    out["flags"] = flags
    out["min_dist_sq"] = EMPTY_VALUE
    if flags & DIST:
        valid = passable & (d >= 0) & (d < DIST_END)
        out["min_dist_sq"] = np.where(valid.any(1), np.where(valid, d, DIST_END).min(1), EMPTY_VALUE)
    known = (ty == FREE) | (ty == OCCUPIED) | (ty == FNT)
    sel = known.any(1) & (keys >= lo).all(1) & (keys <= hi).all(1)
    if not for_grid:
        sel &= out["n_fnt"] >= min_fnt
    return canon(out[sel])


def grid(table, lo, hi):
    """uint32 [nz][ny][nx] over the finite block box lo..hi: 0 where no block qualifies, else 1 << 31 | n_fnt << 20 | n_occupied << 10 | n_free"""
    rec = summaries(table, 0, 0, lo, hi, for_grid=True)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    n = hi - lo + 1
    g = np.zeros((n[2], n[1], n[0]), np.uint32)
    k = rec["key"].astype(np.int64) - lo
    g[k[:, 2], k[:, 1], k[:, 0]] = (1 << 31) | (rec["n_fnt"].astype(np.uint32) << 20) | (rec["n_occupied"].astype(np.uint32) << 10) | rec["n_free"].astype(np.uint32)
    return g


def canon(rec):
    """the records sorted by key (z, y, x): two lists hold the same records iff these are byte-equal"""
    rec = np.ascontiguousarray(rec)
    return rec[np.lexsort((rec["key"][:, 0], rec["key"][:, 1], rec["key"][:, 2]))]


def same(a, b):
    return len(a) == len(b) and canon(a).tobytes() == canon(b).tobytes()


def goals(rec, robot_pos, w, max_goals):
    """VolumetricMapper::global_frontier_blocks from the records of a GIE_BLOCKS_DIST call with min_fnt >= 1: sorted by the squared
    block distance from the robot's block (pos2coord of its position, >> 3), ties by key (z, y, x); per goal the world position of
    the block's fnt_voxel ((float)voxel * w, coord2pos), n_fnt and min_dist_sq.  -> (positions float32 [n, 3], n_fnt, min_dist_sq)"""
    w = np.float32(w)
    rb = np.array([int(np.floor(np.float32(p) / w + np.float32(0.5))) for p in robot_pos], np.int64) >> 3
    rec = canon(rec)
    k = rec["key"].astype(np.int64)
    d2 = ((k - rb) ** 2).sum(1)
    rec = rec[np.argsort(d2, kind="stable")][:max_goals]
    v = rec["fnt_voxel"].astype(np.int64)
    g = rec["key"].astype(np.int64) * 8 + np.stack([v >> 6, (v >> 3) & 7, v & 7], -1)
    return g.astype(np.float32) * w, rec["n_fnt"].astype(np.int32), rec["min_dist_sq"].astype(np.int32)


class GlobalRef:
    """the query_global records of the union box of all volumes so far, +- 8 voxels, rounded out to blocks (one reference per
    checkpoint, shared by its calls)"""

    def __init__(self, size):
        self.size, self.lo, self.hi = np.array(size), None, None

    def add(self, m):
        pv = np.array(m.pivot())
        self.lo = pv - 8 if self.lo is None else np.minimum(self.lo, pv - 8)
        self.hi = pv + self.size + 8 if self.hi is None else np.maximum(self.hi, pv + self.size + 8)

    def take(self, m):
        self.vlo, self.vhi = (self.lo >> 3) << 3, ((self.hi + 7) >> 3) << 3
        rec = m.query_global(box_coords(self.vlo, self.vhi))
        self.table = block_table(rec["vox_type"], rec["dist_sq"], self.vlo, self.vhi)
        self.blo, self.bhi = self.vlo >> 3, (self.vhi >> 3) - 1      # the block box of the data, both inclusive
        return self

    def summaries(self, dist=False, min_fnt=0, lo=None, hi=None):
        return summaries(self.table, DIST if dist else 0, min_fnt, lo, hi)

    def grid(self, lo, hi):
        return grid(self.table, lo, hi)

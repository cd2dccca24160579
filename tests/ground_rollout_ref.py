"""numpy statement of ground rollouts (include/gie.h "ground rollouts") on top of ground_los_ref (the blocked rule and the cell line
L2) and ground_nf1_ref (the cells of points): a plain loop per trajectory over the cells of its polyline.

Cell planes are [Y][X]; f is ground_ref.field's dict (or Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground
field's pivot; nf the ground navigation function's field (Mapper.read_ground_nf1's), needed with the NF1 flag only.  Integers
everywhere, so that the device agrees byte for byte.  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

import ground_los_ref as L
import ground_nf1_ref as N

UNKNOWN_TRAVERSABLE, NF1 = 1, 2
MAX_POSES = 4096
ROLLOUT_DTYPE = np.dtype([("end", "<i4"), ("poses", "<i4"), ("hit", "<i4", (2,)), ("cells", "<i4"), ("min_dist_sq", "<i4"), ("cost", "<i8"),
                          ("nf1_end", "<i4"), ("nf1_min", "<i4"), ("nf1_min_at", "<i4"), ("reserved", "<i4")])
COMPLETE, BLOCKED, LEFT = 0, 1, 2


def prefix(blk, cs):
    """(m, end, hit local or None, the prefix's cells) of one trajectory: cs = its poses' cells (x, y), None for a pose without one"""
    cells = []
    for k, c in enumerate(cs):
        if c is None:
            return k, LEFT, None, cells
        leg = [c] if k == 0 else L.line(cs[k - 1], c)[1:]       # c_0, then every leg without its first cell
        for (x, y) in leg:
            if blk[y, x]:
                return k, BLOCKED, (x, y), cells
        cells += leg
    return len(cs), COMPLETE, None, cells


def rollouts(f, xy, pvt, voxel_width, clearance_sq=0, inflate_sq=0, flags=0, nf=None):
    """what gie_ground_rollouts returns (ROLLOUT_DTYPE [n]) for xy of shape (n, T, 2)"""
    xy = np.asarray(xy, np.float32)
    n, T = xy.shape[0], xy.shape[1]
    blk, d = L.blocked(f, clearance_sq, flags & UNKNOWN_TRAVERSABLE), np.asarray(f["dist_sq"])
    out = np.zeros(n, ROLLOUT_DTYPE)
    for i in range(n):
        cs = N.cells_of(xy[i], pvt, voxel_width, blk.shape)
        m, end, hit, cells = prefix(blk, cs)
        r = out[i]
        r["end"], r["poses"], r["cells"] = end, m, len(cells)
        if hit is not None:
            r["hit"] = (hit[0] + pvt[0], hit[1] + pvt[1])
        dist = [int(d[y, x]) for x, y in cells]
        r["min_dist_sq"] = min(dist) if dist else 0
        r["cost"] = sum(max(0, int(inflate_sq) - v) for v in dist if v != -1)
        if flags & NF1:
            vals = [int(nf[y, x]) for x, y in cs[:m]]
            good = [v for v in vals if v >= 0]
            r["nf1_end"] = vals[-1] if vals else -1
            r["nf1_min"] = min(good) if good else -1
            r["nf1_min_at"] = vals.index(min(good)) if good else -1
        else:
            r["nf1_end"] = r["nf1_min"] = r["nf1_min_at"] = -2
    return out

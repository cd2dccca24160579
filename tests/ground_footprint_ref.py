"""numpy statement of ground footprints (include/gie.h "ground footprints") on top of ground_los_ref (the blocked rule) and
ground_nf1_ref (the cells of points): the predicate of the header, brute force over the bounding box of every pose.

Cell planes are [Y][X]; f is ground_ref.field's dict (or Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground
field's pivot.  Integers everywhere (int64: with extents <= 1 << 16 and heading components within +-32767 every product stays below
2^52), so that the device agrees byte for byte.  Test infrastructure only: numpy, nothing of the device."""
import functools
import math

import numpy as np

import ground_los_ref as L
import ground_nf1_ref as N

UNKNOWN_TRAVERSABLE, MARGIN = 1, 2
MAX_SQ = 1 << 16
MAX_POSES = 4096
FOOTPRINT_DTYPE = np.dtype([("end", "<i4"), ("poses", "<i4"), ("hit", "<i4", (2,)), ("hit_cells", "<i4"), ("min_dist_sq", "<i4"), ("min_at", "<i4"), ("reserved", "<i4")])
COMPLETE, BLOCKED, NO_PLACEMENT = 0, 1, 2


def radius(front_sq, back_sq, side_sq):
    """R: every footprint cell has |dx|, |dy| <= R"""
    return math.isqrt(max(int(front_sq), int(back_sq)) + int(side_sq))


def offsets(h, front_sq, back_sq, side_sq):
    """the footprint of heading h around (0, 0): int64 [k][2] (dx, dy), in (y, x) order; the predicate on every cell of the box"""
    return _offsets(int(h[0]), int(h[1]), int(front_sq), int(back_sq), int(side_sq))


@functools.lru_cache(maxsize=256)
def _offsets(hx, hy, front_sq, back_sq, side_sq):
    assert (hx or hy) and abs(hx) <= 32767 and abs(hy) <= 32767 and 0 <= min(front_sq, back_sq, side_sq) and max(front_sq, back_sq, side_sq) <= MAX_SQ
    R = radius(front_sq, back_sq, side_sq)
    r = np.arange(-R, R + 1, dtype=np.int64)
    dx, dy = r[None, :], r[:, None]
    n2 = hx * hx + hy * hy
    a, b = dx * hx + dy * hy, dx * hy - dy * hx
    ok = (b * b <= int(side_sq) * n2) & (a * a <= np.where(a >= 0, int(front_sq), int(back_sq)) * n2)
    ys, xs = np.nonzero(ok)                                     # row-major: (y, x) order
    out = np.stack([r[xs], r[ys]], 1)
    out.setflags(write=False)
    return out


def placement(xy, heading, pvt, voxel_width, shape):
    """[(x, y) or None] per pose: the cell, None for a pose without a placement"""
    cs = N.cells_of(xy, pvt, voxel_width, shape)
    hd = np.asarray(heading, np.int64).reshape(-1, 2)
    return [c if c is not None and (h[0] or h[1]) and abs(int(h[0])) <= 32767 and abs(int(h[1])) <= 32767 else None for c, h in zip(cs, hd)]


def pose(blk, c, off, unknown_ok):
    """(cells [k][2] signed local (x, y) in (y, x) order, inside bool [k], blocked bool [k]) of the footprint `off` placed at cell c"""
    Y, X = blk.shape
    v = off + np.array(c, np.int64)
    inside = (v[:, 0] >= 0) & (v[:, 0] < X) & (v[:, 1] >= 0) & (v[:, 1] < Y)
    b = np.full(len(v), not unknown_ok)                         # outside: an UNKNOWN column without a dist_sq
    b[inside] = blk[v[inside, 1], v[inside, 0]]
    return v, inside, b


def footprints(f, xy, heading, pvt, voxel_width, front_sq, back_sq, side_sq, clearance_sq=0, flags=0):
    """what gie_ground_footprints returns (FOOTPRINT_DTYPE [n]) for xy and heading of shape (n, T, 2)"""
    xy, heading = np.asarray(xy, np.float32), np.asarray(heading, np.int32)
    n = xy.shape[0]
    blk, d = L.blocked(f, clearance_sq, flags & UNKNOWN_TRAVERSABLE), np.asarray(f["dist_sq"])
    out = np.zeros(n, FOOTPRINT_DTYPE)
    for i in range(n):
        cs = placement(xy[i], heading[i], pvt, voxel_width, blk.shape)
        r = out[i]
        m, best, at = 0, None, -1
        for k, c in enumerate(cs):
            if c is None:
                r["end"] = NO_PLACEMENT
                break
            v, inside, b = pose(blk, c, offsets(heading[i, k], front_sq, back_sq, side_sq), bool(flags & UNKNOWN_TRAVERSABLE))
            if b.any():
                first = v[np.flatnonzero(b)[0]]                 # the least in (y, x)
                r["end"], r["hit"], r["hit_cells"] = BLOCKED, (first[0] + pvt[0], first[1] + pvt[1]), int(b.sum())
                break
            lo = int(d[v[inside, 1], v[inside, 0]].min())
            if best is None or lo < best:
                best, at = lo, k
            m += 1
        r["poses"] = m
        if flags & MARGIN:
            r["min_dist_sq"], r["min_at"] = (best, at) if m else (0, -1)
        else:
            r["min_dist_sq"] = r["min_at"] = -2
    return out


def mask(f, xy, heading, pvt, voxel_width, front_sq, back_sq, side_sq, clearance_sq=0, flags=0):
    """what gie_ground_footprint_mask returns: (uint8 [Y][X], the T = 1 record)"""
    xy, heading = np.asarray(xy, np.float32).reshape(1, 1, 2), np.asarray(heading, np.int32).reshape(1, 1, 2)
    rec = footprints(f, xy, heading, pvt, voxel_width, front_sq, back_sq, side_sq, clearance_sq, flags)[0]
    blk = L.blocked(f, clearance_sq, flags & UNKNOWN_TRAVERSABLE)
    out = np.zeros(blk.shape, np.uint8)
    c = placement(xy[0], heading[0], pvt, voxel_width, blk.shape)[0]
    if c is not None:
        v, inside, b = pose(blk, c, offsets(heading[0, 0], front_sq, back_sq, side_sq), bool(flags & UNKNOWN_TRAVERSABLE))
        out[v[inside, 1], v[inside, 0]] = 1 + b[inside]
    return out, rec

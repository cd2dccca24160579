"""numpy statement of ground line of sight (include/gie.h "ground line of sight") on top of ground_ref.field and
ground_nf1_ref.traversable: the blocked cells, the 2-D cell line L2(a, b), the segment checks and the any-angle shortcut.

Cell planes are [Y][X]; f is ground_ref.field's dict (or Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground
field's pivot; cells are (x, y).  Integers everywhere and one float sum through np.float32 in the order the header gives it, so that
the device agrees bit for bit.  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

import ground_nf1_ref as N

UNKNOWN_TRAVERSABLE = 1
HIT_DTYPE = np.dtype([("first", "<i4"), ("len", "<i4"), ("hit", "<i4", (2,)), ("min_dist_sq", "<i4"), ("reserved", "<i4")])
WAYPOINT_DTYPE = np.dtype([("xy", "<i4", (2,)), ("index", "<i4"), ("min_dist_sq", "<i4"), ("forced", "<i4"), ("reserved", "<i4")])
INFO_DTYPE = np.dtype([("count", "<i4"), ("forced", "<i4"), ("length", "<f4"), ("reserved", "<i4")])
NO_VALUE = -2


def blocked(f, clearance_sq=0, flags=0):
    """bool [Y][X]: not traversable by the ground navigation function's rule"""
    return ~N.traversable(f, clearance_sq, flags & UNKNOWN_TRAVERSABLE)


def walk(a, b):
    """the cells (x, y) of L2(a, b), one at a time: crossing j of axis k at t = (2j - 1) / (2 n_k); the smaller pending t is taken,
    both axes step on a tie; (2 j_x - 1) * n_y against (2 j_y - 1) * n_x decides"""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    nx, ny = abs(bx - ax), abs(by - ay)
    sx, sy = (1 if bx > ax else -1), (1 if by > ay else -1)
    jx = jy = 1
    x, y = ax, ay
    yield (x, y)
    while jx <= nx or jy <= ny:
        if jy > ny:
            c = -1
        elif jx > nx:
            c = 1
        else:
            tx, ty = (2 * jx - 1) * ny, (2 * jy - 1) * nx
            c = -1 if tx < ty else (1 if tx > ty else 0)
        if c <= 0:
            x += sx
            jx += 1
        if c >= 0:
            y += sy
            jy += 1
        yield (x, y)


def line(a, b):
    """L2(a, b) as a list of (x, y)"""
    return list(walk(a, b))


def segments(f, a_xy, b_xy, pvt, voxel_width, clearance_sq=0, flags=0):
    """what gie_ground_segments returns (HIT_DTYPE [n])"""
    blk, d = blocked(f, clearance_sq, flags), np.asarray(f["dist_sq"])
    a, b = N.cells_of(a_xy, pvt, voxel_width, blk.shape), N.cells_of(b_xy, pvt, voxel_width, blk.shape)
    out = np.zeros(len(a), HIT_DTYPE)
    for i, (ca, cb) in enumerate(zip(a, b)):
        if ca is None or cb is None:
            out[i]["first"] = -2
            continue
        cells = line(ca, cb)
        first = next((k for k, (x, y) in enumerate(cells) if blk[y, x]), -1)
        upto = cells if first < 0 else cells[:first + 1]
        hx, hy = cells[first]                                   # (cells[-1] is b)
        out[i] = (first, len(cells), (hx + pvt[0], hy + pvt[1]), min(int(d[y, x]) for x, y in upto), 0)
    return out


def local(points, pvt, shape):
    """(local cells int64 [.., 2], inside [..]) of global int32 points; the difference in 64 bits"""
    Y, X = shape
    v = np.asarray(points, np.int64) - np.asarray(pvt[:2], np.int64)
    return v, np.all((v >= 0) & (v < np.array([X, Y], np.int64)), axis=-1)


def clear(blk, a, b):
    """Clear(a, b) for two cells inside the rectangle"""
    return not any(blk[y, x] for x, y in walk(a, b))


def shortcut(f, paths, lens, pvt, lookahead, max_wp, clearance_sq=0, flags=0, wp_init=None):
    """what gie_ground_shortcut returns: (wp [n, max_wp] WAYPOINT_DTYPE, info [n] INFO_DTYPE).  paths: (n, max_len, 2) int32 global
    cells; wp_init: what the caller's array held (zeros when None) — entries beyond a path's records keep it.  max J is found from
    the window's far end: the first clear index met is the largest."""
    paths = np.asarray(paths, np.int32)
    n, max_len = paths.shape[0], paths.shape[1]
    lens = np.asarray(lens, np.int32).reshape(-1)
    blk, d = blocked(f, clearance_sq, flags), np.asarray(f["dist_sq"])
    wp = np.zeros((n, max_wp), WAYPOINT_DTYPE) if wp_init is None else np.array(wp_init, WAYPOINT_DTYPE).reshape(n, max_wp)
    info = np.zeros(n, INFO_DTYPE)
    for i in range(n):
        m = int(min(max(int(lens[i]), 0), max_len))
        if m == 0:
            continue
        v, inside = local(paths[i, :m], pvt, blk.shape)
        rec = [(0, int(d[v[0, 1], v[0, 0]]) if inside[0] else NO_VALUE, 0)]
        length, forced, k = np.float32(0.0), 0, 0
        while k < m - 1:
            nk = None
            if inside[k] and not blk[v[k, 1], v[k, 0]]:
                for j in range(min(k + int(lookahead), m - 1), k, -1):
                    if inside[j] and clear(blk, v[k], v[j]):
                        nk = j
                        break
            if nk is None:
                forced += 1
                rec.append((k + 1, NO_VALUE, 1))
                k += 1
            else:
                d2 = int(((v[nk] - v[k]) ** 2).sum())
                length = np.float32(length + np.sqrt(np.float32(d2)))
                rec.append((nk, min(int(d[y, x]) for x, y in line(v[k], v[nk])), 0))
                k = nk
        info[i] = (len(rec), forced, length, 0)
        for t, (j, md, fo) in enumerate(rec[:max_wp]):
            wp[i, t] = (paths[i, j], j, md, fo, 0)
    return wp, info

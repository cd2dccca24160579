"""numpy statement of ground view gain (include/gie.h "ground view gain") on top of ground_los_ref.walk and the planes
Mapper.read_ground returns (only "type" is read): the opaque cells, the candidate tests, visibility and the mask by ONE vectorised
walk of all candidates of a view (ground_los_ref.walk's steps on arrays, a line dropped where it hits), the scores.

Cell planes are [Y][X]; cells are (x, y); normals are (n_planes, 2) integers, x then y.  Integers everywhere; the two radius products
through np.float32, so that the device agrees bit for bit.  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

import ground_los_ref as L
import ground_nf1_ref as N
import ground_ref as G

UNKNOWN_OPAQUE, UNION = 1, 2
SCORE_DTYPE = np.dtype([("unknown", "<i4"), ("frontier", "<i4"), ("occupied", "<i4"), ("candidates", "<i4")])
NORMAL_MAX = 32767


def opaque(f, flags=0):
    """bool [Y][X]: sight stops at these columns"""
    t = np.asarray(f["type"])
    op = t == G.OCCUPIED
    if flags & UNKNOWN_OPAQUE:
        op = op | (t == G.UNKNOWN)
    return op


def radii_sq(r_min, r_max, voxel_width):
    """(rmin * rmin, rmax * rmax) as the header rounds them: one float32 quotient and one float32 product each"""
    with np.errstate(over="ignore"):
        rmin, rmax = np.float32(r_min) / np.float32(voxel_width), np.float32(r_max) / np.float32(voxel_width)
        return np.float32(rmin * rmin), np.float32(rmax * rmax)


def in_sector(dx, dy, normals, flags=0):
    """the sector test of d = (dx, dy) (arrays or integers) against 0, 1 or 2 half planes"""
    nr = np.asarray(normals if normals is not None else [], np.int64).reshape(-1, 2)
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    if len(nr) == 0:
        return np.ones(dx.shape, bool)
    h = [n[0] * dx + n[1] * dy >= 0 for n in nr]
    if len(nr) == 1:
        return h[0]
    return (h[0] | h[1]) if flags & UNION else (h[0] & h[1])


def candidates(shape, p, r_min, r_max, voxel_width, normals=None, flags=0):
    """bool [Y][X]: the candidates of a view at cell p"""
    Y, X = shape
    dx, dy = np.arange(X, dtype=np.int64)[None, :] - int(p[0]), np.arange(Y, dtype=np.int64)[:, None] - int(p[1])
    d2 = dx * dx + dy * dy
    rmin2, rmax2 = radii_sq(r_min, r_max, voxel_width)
    fd = d2.astype(np.float32)
    return (d2 != 0) & (fd >= rmin2) & (fd <= rmax2) & in_sector(dx + 0 * dy, dy + 0 * dx, normals, flags)


def visible(op, p, cells):
    """bool [k]: for each candidate cell (k x 2, x then y), no cell of L2(p, v) other than v is opaque; p's own cell is not tested.
    ground_los_ref.walk's loop from p on all lines at once: the smaller pending crossing, both axes on a tie."""
    v = np.asarray(cells, np.int64).reshape(-1, 2)
    k = len(v)
    nx, ny = np.abs(v[:, 0] - int(p[0])), np.abs(v[:, 1] - int(p[1]))
    sx, sy = np.where(v[:, 0] > int(p[0]), 1, -1), np.where(v[:, 1] > int(p[1]), 1, -1)
    jx, jy = np.ones(k, np.int64), np.ones(k, np.int64)
    x, y = np.full(k, int(p[0]), np.int64), np.full(k, int(p[1]), np.int64)
    vis = np.ones(k, bool)
    live = np.arange(k)
    while live.size:
        a = live
        c = np.sign((2 * jx[a] - 1) * ny[a] - (2 * jy[a] - 1) * nx[a])
        c = np.where(jy[a] > ny[a], -1, np.where(jx[a] > nx[a], 1, c))
        mx, my = c <= 0, c >= 0
        x[a] += np.where(mx, sx[a], 0); jx[a] += mx
        y[a] += np.where(my, sy[a], 0); jy[a] += my
        at_v = (jx[a] > nx[a]) & (jy[a] > ny[a])                # the cell reached is v itself: not tested
        hit = ~at_v & op[y[a], x[a]]
        vis[a[hit]] = False
        live = a[~at_v & ~hit]
    return vis


def view(f, p, r_min, r_max, voxel_width, normals=None, flags=0):
    """(mask uint8 [Y][X], score SCORE_DTYPE record) of one view at cell p; p None (no cell) or a normal component beyond +-32767
    (what the _dev forms score -1): the mask all 0 and the score -1"""
    t = np.asarray(f["type"])
    mask = np.zeros(t.shape, np.uint8)
    score = np.zeros(1, SCORE_DTYPE)[0]
    nr = np.asarray(normals if normals is not None else [], np.int64).reshape(-1, 2)
    if p is None or (np.abs(nr) > NORMAL_MAX).any():
        score["unknown"] = score["frontier"] = score["occupied"] = score["candidates"] = -1
        return mask, score
    cand = candidates(t.shape, p, r_min, r_max, voxel_width, nr, flags)
    cells = np.argwhere(cand)[:, ::-1]
    vis = visible(opaque(f, flags), p, cells)
    mask[cand] = 1
    mask[cells[vis, 1], cells[vis, 0]] = 2
    tv = t[mask == 2]
    score["unknown"], score["frontier"], score["occupied"] = (tv == G.UNKNOWN).sum(), (tv == G.FNT).sum(), (tv == G.OCCUPIED).sum()
    score["candidates"] = cand.sum()
    return mask, score


def gain(f, xy, pvt, r_min, r_max, voxel_width, normals=None, n_planes=0, flags=0, masks=False):
    """what gie_ground_view_gain_dev returns for n views at world points xy (SCORE_DTYPE [n]); with masks also every view's mask"""
    t = np.asarray(f["type"])
    cells = N.cells_of(xy, pvt, voxel_width, t.shape)
    nr = None if n_planes == 0 else np.asarray(normals, np.int64).reshape(len(cells), n_planes, 2)
    out, ms = np.zeros(len(cells), SCORE_DTYPE), []
    for i, p in enumerate(cells):
        m, out[i] = view(f, p, r_min, r_max, voxel_width, None if nr is None else nr[i], flags)
        ms.append(m)
    return (out, ms) if masks else out


def view_by_lines(f, p, r_min, r_max, voxel_width, normals=None, flags=0):
    """the same as view() for a cell p, by a plain loop over the cells and ground_los_ref.line per candidate (small planes only)"""
    t = np.asarray(f["type"])
    Y, X = t.shape
    op = opaque(f, flags)
    rmin2, rmax2 = radii_sq(r_min, r_max, voxel_width)
    mask = np.zeros(t.shape, np.uint8)
    score = np.zeros(1, SCORE_DTYPE)[0]
    for y in range(Y):
        for x in range(X):
            dx, dy = x - int(p[0]), y - int(p[1])
            d2 = np.float32(dx * dx + dy * dy)
            if (dx == 0 and dy == 0) or not (d2 >= rmin2 and d2 <= rmax2) or not bool(in_sector(dx, dy, normals, flags)):
                continue
            score["candidates"] += 1
            vis = True
            for cx, cy in L.line(p, (x, y))[1:-1]:
                if op[cy, cx]:
                    vis = False
            mask[y, x] = 2 if vis else 1
            if vis:
                key = {G.UNKNOWN: "unknown", G.FNT: "frontier", G.OCCUPIED: "occupied"}.get(int(t[y, x]))
                if key:
                    score[key] += 1
    return mask, score

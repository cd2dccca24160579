"""numpy statement of the ground navigation function (include/gie.h "ground navigation function") on top of ground_ref.field.

Cell planes are [Y][X]; f is ground_ref.field's dict (or Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground
field's pivot; goals and starts are world points (n x 2 metres)."""
import numpy as np

import ground_ref as G
from gie import scenes

UNKNOWN_TRAVERSABLE, FROM_FRONTIERS = 1, 2
SEENDIST = G.SEENDIST


def traversable(f, clearance_sq=0, flags=0):
    t, d = np.asarray(f["type"]), np.asarray(f["dist_sq"])
    is_open = (t == G.FREE) | (t == G.FNT)
    if flags & UNKNOWN_TRAVERSABLE:
        is_open = is_open | (t == G.UNKNOWN)
    return is_open & ((d == -1) | (d >= clearance_sq))


def cells_of(xy, pvt, voxel_width, shape):
    """[(x, y) or None]: the cell of each world point, None outside the rectangle and for points that are not finite"""
    Y, X = shape
    out = []
    for p in np.asarray(xy, np.float32).reshape(-1, 2):
        c = None
        if np.isfinite(p).all():
            x, y = scenes.pos2coord(p[0], voxel_width) - pvt[0], scenes.pos2coord(p[1], voxel_width) - pvt[1]
            if 0 <= x < X and 0 <= y < Y:
                c = (int(x), int(y))
        out.append(c)
    return out


def sources(f, trav, goals_xy, pvt, voxel_width, flags=0):
    src = np.zeros(trav.shape, bool)
    for c in cells_of(goals_xy, pvt, voxel_width, trav.shape):
        if c is not None:
            src[c[1], c[0]] = True
    if flags & FROM_FRONTIERS:
        src |= np.asarray(f["type"]) == G.FNT
    return src & trav


def propagate(trav, src):
    """int32 [Y][X]: a level-synchronous dilation with the cross (4-neighbour) structure, on the index set of the frontier: level
    k + 1 is what the cross reaches from level k inside the rectangle, traversable and without a value yet"""
    Y, X = trav.shape
    nf = np.full(Y * X, -1, np.int32)
    ok = trav.ravel()
    fr = np.flatnonzero(src.ravel())
    nf[fr] = 0
    level = 0
    while fr.size:
        x = fr % X
        cand = np.concatenate([fr[x > 0] - 1, fr[x < X - 1] + 1, fr[fr >= X] - X, fr[fr < (Y - 1) * X] + X])
        cand = np.unique(cand[ok[cand] & (nf[cand] < 0)])
        level += 1
        nf[cand] = level
        fr = cand
    return nf.reshape(Y, X)


def field(f, goals_xy, pvt, voxel_width, clearance_sq=0, flags=0):
    """(nf1 int32 [Y][X], the number of sources)"""
    trav = traversable(f, clearance_sq, flags)
    src = sources(f, trav, goals_xy, pvt, voxel_width, flags)
    return propagate(trav, src), int(src.sum())


def path(nf, starts_xy, pvt, voxel_width, max_len, fill=0):
    """(path int32 [n][max_len][2] GLOBAL x y, len int32 [n]): the header's rule, one step at a time; unwritten points = fill"""
    Y, X = nf.shape
    starts = cells_of(starts_xy, pvt, voxel_width, nf.shape)
    out = np.full((len(starts), max_len, 2), fill, np.int32)
    ln = np.zeros(len(starts), np.int32)
    for i, c in enumerate(starts):
        if c is None or nf[c[1], c[0]] < 0:
            continue
        x, y = c
        ln[i] = nf[y, x] + 1
        for k in range(min(int(ln[i]), max_len)):
            out[i, k] = (x + pvt[0], y + pvt[1])
            if nf[y, x] == 0:
                break
            for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):       # -x +x -y +y
                if 0 <= nx < X and 0 <= ny < Y and nf[ny, nx] == nf[y, x] - 1:
                    x, y = nx, ny
                    break
            else:
                raise AssertionError("no neighbour one step closer: not an NF1 field")
    return out, ln


def costmap(nf, f, size, pvt, voxel_width, z_lo):
    """(payload [Y][X] SEENDIST, header fields) of gie_read_costmap_ground_nf1"""
    pay = np.zeros(nf.shape, SEENDIST)
    pay["d"] = nf.astype(np.float32)
    pay["o"] = np.asarray(f["type"]) != G.UNKNOWN
    _, hdr = G.costmap({"dist_sq": np.zeros(nf.shape, np.int32), "type": np.asarray(f["type"])}, size, pvt, voxel_width, z_lo)
    hdr["type"] = 2
    return pay, hdr

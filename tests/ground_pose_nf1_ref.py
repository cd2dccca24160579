"""numpy statement of the ground pose navigation function (include/gie.h "ground pose navigation function") on top of
ground_footprint_ref (the footprint's offsets, the blocked rule via ground_los_ref) and ground_nf1_ref (the cells of points).

States are (cell, heading k in 0..7); planes are [8][Y][X], k slowest; f is ground_ref.field's dict (or Mapper.read_ground's: only
"type" and "dist_sq" are read); pvt the ground field's pivot.  The C-space comes from shifted ORs of the blocked plane over the
footprint's offsets, the field from a plain queue BFS over predecessors, path and query one step at a time.  Test infrastructure
only: numpy, nothing of the device."""
from collections import deque

import numpy as np

import ground_footprint_ref as P
import ground_los_ref as L
import ground_nf1_ref as N
import ground_ref as G

UNKNOWN_TRAVERSABLE, FROM_FRONTIERS, REVERSE = 1, 2, 4
HEADINGS = 8
MAX_SQ = 1 << 12
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def heading_index(yaw):
    """VolumetricMapper::ground_heading_index: lround(yaw / (pi / 4)) mod 8"""
    q = yaw / (np.pi / 4)
    r = int(np.floor(abs(q) + 0.5)) * (1 if q >= 0 else -1)    # lround: halves away from zero
    return r % 8


def cspace(f, front_sq, back_sq, side_sq, clearance_sq=0, flags=0):
    """bool [8][Y][X]: state (c, k) is NOT free — some footprint cell of heading d_k at c is blocked (outside cells block without
    the UNKNOWN flag)"""
    assert 0 <= min(front_sq, back_sq, side_sq) and max(front_sq, back_sq, side_sq) <= MAX_SQ
    blk = L.blocked(f, clearance_sq, flags & UNKNOWN_TRAVERSABLE)
    Y, X = blk.shape
    R = P.radius(front_sq, back_sq, side_sq)
    pad = np.full((Y + 2 * R, X + 2 * R), not (flags & UNKNOWN_TRAVERSABLE))
    pad[R:R + Y, R:R + X] = blk
    out = np.zeros((HEADINGS, Y, X), bool)
    for k, d in enumerate(DIRS):
        for dx, dy in P.offsets(d, front_sq, back_sq, side_sq).tolist():
            out[k] |= pad[R + dy:R + dy + Y, R + dx:R + dx + X]
    return out


def cspace_bytes(cs):
    """uint8 [Y][X]: bit k set iff (c, k) is not free"""
    return (cs.astype(np.uint8) << np.arange(HEADINGS, dtype=np.uint8)[:, None, None]).sum(0).astype(np.uint8)


def sources(f, cs, goals_xy, goal_k, pvt, voxel_width, flags=0):
    """bool [8][Y][X]: the free states among the goals' and, with FROM_FRONTIERS, the FNT cells'"""
    _, Y, X = cs.shape
    src = np.zeros(cs.shape, bool)
    cells = N.cells_of(goals_xy, pvt, voxel_width, (Y, X)) if goals_xy is not None and np.size(goals_xy) else []
    ks = [-1] * len(cells) if goal_k is None else [int(k) for k in np.asarray(goal_k).reshape(-1)]
    for c, k in zip(cells, ks):
        if c is None:
            continue
        if k == -1:
            src[:, c[1], c[0]] = True
        elif 0 <= k < HEADINGS:
            src[k, c[1], c[0]] = True
    if flags & FROM_FRONTIERS:
        src |= (np.asarray(f["type"]) == G.FNT)[None]
    return src & ~cs


def moves(x, y, k, reverse):
    """the targets of F, (B,) L, R from (x, y, k), in that order; inside the rectangle or not"""
    dx, dy = DIRS[k]
    out = [(x + dx, y + dy, k)]
    if reverse:
        out.append((x - dx, y - dy, k))
    return out + [(x, y, (k + 1) & 7), (x, y, (k + 7) & 7)]


def propagate(cs, src, reverse):
    """int32 [8][Y][X]: a queue BFS from the sources over PREDECESSORS: p reaches s by one admissible move"""
    _, Y, X = cs.shape
    nf = np.full(cs.shape, -1, np.int32)
    q = deque()
    for k, y, x in zip(*np.nonzero(src)):
        nf[k, y, x] = 0
        q.append((int(x), int(y), int(k)))
    while q:
        x, y, k = q.popleft()
        dx, dy = DIRS[k]
        pred = [(x - dx, y - dy, k)]                            # its F leads here
        if reverse:
            pred.append((x + dx, y + dy, k))                    # its B leads here
        pred += [(x, y, (k + 7) & 7), (x, y, (k + 1) & 7)]      # its L, its R
        for px, py, pk in pred:
            if 0 <= px < X and 0 <= py < Y and not cs[pk, py, px] and nf[pk, py, px] < 0:
                nf[pk, py, px] = nf[k, y, x] + 1
                q.append((px, py, pk))
    return nf


def field(f, goals_xy, goal_k, pvt, voxel_width, front_sq, back_sq, side_sq, clearance_sq=0, flags=0):
    """(pnf1 int32 [8][Y][X], cspace uint8 [Y][X], counts [sources, free states])"""
    cs = cspace(f, front_sq, back_sq, side_sq, clearance_sq, flags)
    src = sources(f, cs, goals_xy, goal_k, pvt, voxel_width, flags)
    return propagate(cs, src, bool(flags & REVERSE)), cspace_bytes(cs), [int(src.sum()), int((~cs).sum())]


def _best(nf, c):
    """(k, value) of the lowest k with the least value >= 0 at cell c, (-1, -1) without one"""
    v = nf[:, c[1], c[0]]
    ok = np.flatnonzero(v >= 0)
    if not ok.size:
        return -1, -1
    k = int(ok[np.argmin(v[ok])])
    return k, int(v[k])


def query(nf, xy, k, pvt, voxel_width):
    """int32 [n]: what gie_ground_pose_nf1_query returns"""
    cells = N.cells_of(xy, pvt, voxel_width, nf.shape[1:])
    ks = [-1] * len(cells) if k is None else [int(v) for v in np.asarray(k).reshape(-1)]
    out = np.full(len(cells), -1, np.int32)
    for i, (c, kk) in enumerate(zip(cells, ks)):
        if c is None:
            continue
        if kk == -1:
            out[i] = _best(nf, c)[1]
        elif 0 <= kk < HEADINGS:
            out[i] = nf[kk, c[1], c[0]]
    return out


def path(nf, starts_xy, start_k, pvt, voxel_width, max_len, reverse, fill=0):
    """(path int32 [n][max_len][3] GLOBAL x, y and k, len int32 [n]): the header's rule; unwritten triples = fill"""
    _, Y, X = nf.shape
    cells = N.cells_of(starts_xy, pvt, voxel_width, (Y, X))
    ks = [-1] * len(cells) if start_k is None else [int(v) for v in np.asarray(start_k).reshape(-1)]
    out = np.full((len(cells), max_len, 3), fill, np.int32)
    ln = np.zeros(len(cells), np.int32)
    for i, (c, k) in enumerate(zip(cells, ks)):
        if c is None or not -1 <= k < HEADINGS:
            continue
        if k == -1:
            k = _best(nf, c)[0]
            if k < 0:
                continue
        x, y = c
        if nf[k, y, x] < 0:
            continue
        ln[i] = nf[k, y, x] + 1
        for j in range(min(int(ln[i]), max_len)):
            out[i, j] = (x + pvt[0], y + pvt[1], k)
            if nf[k, y, x] == 0:
                break
            for nx, ny, nk in moves(x, y, k, reverse):
                if 0 <= nx < X and 0 <= ny < Y and nf[nk, ny, nx] == nf[k, y, x] - 1:
                    x, y, k = nx, ny, nk
                    break
            else:
                raise AssertionError("no move one step closer: not a pose NF1 field")
    return out, ln

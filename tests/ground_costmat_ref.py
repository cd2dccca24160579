"""numpy statement of the ground cost matrix (include/gie.h "ground cost matrix") on top of ground_nf1_ref: for each valid point one
propagate from its cell, read at the other points' cells.  Cell planes are [Y][X]; f is ground_ref.field's dict (or
Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground field's pivot; points are world points (n x 2 metres)."""
import numpy as np

import ground_nf1_ref as N

MAX_POINTS = 256


def matrix_of_cells(trav, cells):
    """(cost [n, n] int32, valid [n] bool) for cells [(x, y) or None] (None: outside the rectangle, or a point that is not finite)"""
    trav = np.asarray(trav, bool)
    n = len(cells)
    valid = np.array([c is not None and bool(trav[c[1], c[0]]) for c in cells], bool).reshape(n)
    cost = np.full((n, n), -1, np.int32)
    ok = np.flatnonzero(valid)
    xs, ys = np.array([cells[i][0] for i in ok], np.int64), np.array([cells[i][1] for i in ok], np.int64)
    done = {}
    for k, j in enumerate(ok):
        if cells[j] not in done:                                # (points on one cell share their field)
            src = np.zeros(trav.shape, bool)
            src[ys[k], xs[k]] = True
            done[cells[j]] = N.propagate(trav, src)[ys, xs]
        cost[ok, j] = done[cells[j]]                            # cost[i][j]: the field of goal j at cell(i)
    return cost, valid


def matrix(f, points, pvt, voxel_width, clearance_sq=0, flags=0):
    """the whole statement on a ground field"""
    assert not flags & N.FROM_FRONTIERS and clearance_sq >= 0
    trav = N.traversable(f, clearance_sq, flags)
    return matrix_of_cells(trav, N.cells_of(points, pvt, voxel_width, trav.shape))

"""numpy statement of the goal-to-goal cost matrix (include/gie.h "cost matrix"): for each valid point one nf1_ref.bfs from its
voxel, read at the other points' voxels.  Arrays are [Z][Y][X] like read_local."""
import numpy as np

import nf1_ref

MAX_POINTS = 64


def matrix_of_voxels(trav, vox, inside):
    """(cost [n, n] int32, valid [n] bool) for local voxels vox [n, 3] (x, y, z); inside [n] bool says which lie in the volume"""
    trav = np.asarray(trav, bool)
    vox = np.asarray(vox, np.int64).reshape(-1, 3)
    n = len(vox)
    valid = np.zeros(n, bool)
    for i in range(n):
        valid[i] = bool(inside[i]) and bool(trav[vox[i, 2], vox[i, 1], vox[i, 0]])
    cost = np.full((n, n), -1, np.int32)
    ok = np.flatnonzero(valid)
    for j in ok:
        src = np.zeros(trav.shape, bool)
        src[vox[j, 2], vox[j, 1], vox[j, 0]] = True
        f = nf1_ref.bfs(trav, src)
        cost[ok, j] = f[vox[ok, 2], vox[ok, 1], vox[ok, 0]]     # cost[i][j]: the field of goal j at voxel(i)
    return cost, valid


def matrix(vtype, edt, points, clearance=0.0, flags=0, voxel_width=1.0, pvt=(0, 0, 0)):
    """the whole statement on read_local's planes: clearance in voxel units, points [n, 3] in metres"""
    assert not flags & nf1_ref.FROM_FRONTIERS
    Z, Y, X = vtype.shape
    trav = nf1_ref.traversable(vtype, edt, clearance, flags)
    vox, inside = nf1_ref.point_voxels(points, voxel_width, pvt, (X, Y, Z))
    return matrix_of_voxels(trav, vox, inside)

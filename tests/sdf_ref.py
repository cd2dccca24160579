"""numpy / scipy statement of the signed distance field and its queries (include/gie.h "signed distance").

Arrays are [Z][Y][X] like Mapper.read_local; sizes are (X, Y, Z).  The query follows the device's float32 operation order
(csrc/gie_sdf.inc.h k_sdf_query, built with -ffp-contract=off), so that it agrees with it to rounding."""
import numpy as np
from scipy import ndimage

OCCUPIED = 2
UNKNOWN = 0


def inside_dist_sq(vtype):
    """int32 [Z][Y][X]: 0 off the obstacles, the exact squared distance to the nearest non-occupied voxel of the volume on them,
    -1 everywhere when the volume holds no non-occupied voxel."""
    occ = np.asarray(vtype) == OCCUPIED
    if not occ.any():
        return np.zeros(occ.shape, np.int32)
    if occ.all():
        return np.full(occ.shape, -1, np.int32)
    _, idx = ndimage.distance_transform_edt(occ, return_indices=True)
    grid = np.indices(occ.shape)
    d = ((idx - grid).astype(np.int64) ** 2).sum(axis=0)
    return np.where(occ, d, 0).astype(np.int32)


def inside_dist_sq_brute(vtype):
    """the same by brute force (small grids)."""
    occ = np.asarray(vtype) == OCCUPIED
    free = np.argwhere(~occ)
    out = np.zeros(occ.shape, np.int32)
    for p in np.argwhere(occ):
        out[tuple(p)] = ((free - p) ** 2).sum(axis=1).min() if len(free) else -1
    return out


def max_loc_dist_sq(size):
    return int(size[0]) ** 2 + int(size[1]) ** 2 + int(size[2]) ** 2


def sdf(ids, edt, size):
    """sdf from inside_dist_sq and the positive EDT (read_local()["edt"]), float32 voxel units."""
    ids = np.asarray(ids)
    deep = np.float32(1.0) - np.sqrt(np.maximum(ids, 0).astype(np.float32))
    out = np.where(ids > 1, deep, np.asarray(edt, np.float32))
    return np.where(ids == -1, np.float32(-max_loc_dist_sq(size)), out).astype(np.float32)


def query(sdf_plane, vtype, size, pvt, voxel_width, xyz):
    """(dist [n] metres, grad [n,3] m/m, flags [n] uint8) of the trilinear interpolant of `sdf_plane` at world points xyz."""
    f32 = np.float32
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    w = f32(voxel_width)
    S = [int(s) for s in size]
    inside = np.ones(n, bool)
    i0 = np.zeros((3, n), np.int64)
    i1 = np.zeros((3, n), np.int64)
    t = np.zeros((3, n), np.float32)
    for k in range(3):
        u = (xyz[:, k] / w - f32(pvt[k])).astype(np.float32)
        if S[k] >= 2:
            ok = (u >= f32(0)) & (u <= f32(S[k] - 1))
            uu = np.where(ok, u, f32(0))
            a = np.minimum(np.floor(uu).astype(np.int64), S[k] - 2)
            i0[k] = a
            i1[k] = a + 1
            t[k] = np.where(ok, uu - a.astype(np.float32), f32(0))
        else:
            ok = (u >= f32(-0.5)) & (u < f32(0.5))
        inside &= ok
    v = []
    known = np.ones(n, bool)
    occ = np.zeros(n, bool)
    for k in range(8):
        x = np.where(k & 1, i1[0], i0[0])
        y = np.where(k & 2, i1[1], i0[1])
        z = np.where(k & 4, i1[2], i0[2])
        v.append(sdf_plane[z, y, x].astype(np.float32))
        ty = vtype[z, y, x]
        known &= ty != UNKNOWN
        occ |= ty == OCCUPIED
    tx, ty_, tz = t
    sx, sy, sz = f32(1) - tx, f32(1) - ty_, f32(1) - tz
    c00 = v[0] * sx + v[1] * tx
    c10 = v[2] * sx + v[3] * tx
    c01 = v[4] * sx + v[5] * tx
    c11 = v[6] * sx + v[7] * tx
    c0 = c00 * sy + c10 * ty_
    c1 = c01 * sy + c11 * ty_
    dist = (c0 * sz + c1 * tz) * w
    e0 = (v[1] - v[0]) * sy + (v[3] - v[2]) * ty_
    e1 = (v[5] - v[4]) * sy + (v[7] - v[6]) * ty_
    grad = np.stack([e0 * sz + e1 * tz if S[0] >= 2 else np.zeros(n, np.float32),
                     (c10 - c00) * sz + (c11 - c01) * tz if S[1] >= 2 else np.zeros(n, np.float32),
                     c1 - c0 if S[2] >= 2 else np.zeros(n, np.float32)], axis=1).astype(np.float32)
    flags = (1 | np.where(known, 2, 0) | np.where(occ, 4, 0)).astype(np.uint8)
    dist = np.where(inside, dist, np.float32(np.nan)).astype(np.float32)
    grad[~inside] = 0
    flags[~inside] = 0
    return dist, grad, flags

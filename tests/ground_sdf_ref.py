"""numpy / scipy statement of the ground signed distance field (include/gie.h "ground signed distance").

Cell planes are [Y][X] like Mapper.read_ground; `g` is that reader's dict (its "type" and "dist_sq" planes are used), `size` the
volume's (X, Y, Z), `pvt` the field's pivot, `blocks` whether the field was computed with GIE_GROUND_UNKNOWN_BLOCKS.  Every float is a
float32 and every operation one float32 operation, in the order the header states."""
import numpy as np
from scipy import ndimage

import ground_ref as R

F32 = np.float32
ROLLOUT_DTYPE = np.dtype([("points", "<i4"), ("argmin", "<i4"), ("min_dist", "<f4"), ("grad", "<f4", (2,)), ("first_below", "<i4"), ("n_below", "<i4"),
                          ("first_in", "<i4")])
MAX_POSES = 4096


def obstacles(g, blocks=False):
    return R.obstacles(np.asarray(g["type"]), R.UNKNOWN_BLOCKS if blocks else 0)


def inside_dist_sq(obs):
    """int32 [Y][X]: 0 off the obstacles; on them the exact squared distance to the nearest cell that is none, from scipy's indices;
    -1 everywhere when every cell is an obstacle"""
    obs = np.asarray(obs, bool)
    if obs.all():
        return np.full(obs.shape, -1, np.int32)
    if not obs.any():
        return np.zeros(obs.shape, np.int32)
    _, idx = ndimage.distance_transform_edt(obs, return_indices=True)
    d = ((idx - np.indices(obs.shape)).astype(np.int64) ** 2).sum(axis=0).astype(np.int32)
    d[~obs] = 0
    return d


def interior(obs):
    """bool [Y][X]: obstacle cells whose four edge neighbours are obstacle cells, outside the rectangle counting as one"""
    p = np.pad(np.asarray(obs, bool), 1, constant_values=True)
    return p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]


def gsdf(ids, dist_sq, size):
    """float32 [Y][X] from inside_dist_sq and the ground field's dist_sq (-1 everywhere on a field without an obstacle column)"""
    ids, dist_sq = np.asarray(ids), np.asarray(dist_sq)
    far = F32(size[0] ** 2 + size[1] ** 2 + size[2] ** 2)
    pos = np.where(dist_sq < 0, far, np.sqrt(np.maximum(dist_sq, 0).astype(F32))).astype(F32)
    neg = (F32(1.0) - np.sqrt(np.maximum(ids, 0).astype(F32))).astype(F32)
    return np.where(ids < 0, -far, np.where(ids <= 1, pos, neg)).astype(F32)


def field(g, size, blocks=False):
    """{"obs", "inside_dist_sq", "sdf"} of read_ground()'s planes"""
    obs = obstacles(g, blocks)
    ids = inside_dist_sq(obs)
    return {"obs": obs, "inside_dist_sq": ids, "sdf": gsdf(ids, g["dist_sq"], size)}


def query(f, g, pvt, voxel_width, xy):
    """(dist [n] float32 metres, grad [n][2] float32, flags [n] uint8) of world points xy (n x 2 metres) on field() `f` of planes `g`"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    n = len(xy)
    sdf, obs, known = f["sdf"], f["obs"], np.asarray(g["type"]) != R.UNKNOWN
    Y, X = sdf.shape
    w = F32(voxel_width)
    inside = np.ones(n, bool)
    i0, t = np.zeros((2, n), np.int64), np.zeros((2, n), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, S in enumerate((X, Y)):
            u = (xy[:, k] / w - F32(pvt[k])).astype(F32)
            if S >= 2:
                ok = (u >= F32(0)) & (u <= F32(S - 1))
                i0[k] = np.minimum(np.floor(np.where(ok, u, F32(0))).astype(np.int64), S - 2)
                t[k] = np.where(ok, u - i0[k].astype(F32), F32(0)).astype(F32)
            else:
                ok = (u >= F32(-0.5)) & (u < F32(0.5))
            inside &= ok
    i1 = [i0[0] + (1 if X >= 2 else 0), i0[1] + (1 if Y >= 2 else 0)]
    corner = [(i0[1], i0[0]), (i0[1], i1[0]), (i1[1], i0[0]), (i1[1], i1[0])]
    v0, v1, v2, v3 = (sdf[c] for c in corner)
    tx, ty = t[0], t[1]
    sx, sy = (F32(1) - tx).astype(F32), (F32(1) - ty).astype(F32)
    c0 = ((v0 * sx).astype(F32) + (v1 * tx).astype(F32)).astype(F32)
    c1 = ((v2 * sx).astype(F32) + (v3 * tx).astype(F32)).astype(F32)
    dist = ((((c0 * sy).astype(F32) + (c1 * ty).astype(F32)).astype(F32)) * w).astype(F32)
    gx = ((((v1 - v0).astype(F32) * sy).astype(F32)) + (((v3 - v2).astype(F32) * ty).astype(F32))).astype(F32)
    gy = (c1 - c0).astype(F32)
    grad = np.stack([gx if X >= 2 else np.zeros(n, F32), gy if Y >= 2 else np.zeros(n, F32)], 1).astype(F32)
    all_known = known[corner[0]] & known[corner[1]] & known[corner[2]] & known[corner[3]]
    some_obs = obs[corner[0]] | obs[corner[1]] | obs[corner[2]] | obs[corner[3]]
    flags = (1 + 2 * all_known.astype(np.uint8) + 4 * some_obs.astype(np.uint8)).astype(np.uint8)
    dist = np.where(inside, dist, F32(np.nan)).astype(F32)
    grad = np.where(inside[:, None], grad, F32(0)).astype(F32)
    flags = np.where(inside, flags, 0).astype(np.uint8)
    return dist, grad, flags


def record(dist, grad, flags, margin):
    """the record of ONE trajectory from its per-point query results: a plain loop"""
    margin = F32(margin)
    m = 0
    while m < len(dist) and flags[m] & 1:
        m += 1
    argmin, first_below, n_below, first_in = -1, -1, 0, -1
    for k in range(m):
        if argmin < 0 or dist[k] < dist[argmin]:
            argmin = k
        if dist[k] < margin:
            n_below += 1
            first_below = k if first_below < 0 else first_below
        if dist[k] <= F32(0) and first_in < 0:
            first_in = k
    r = np.zeros((), ROLLOUT_DTYPE)
    r["points"], r["argmin"], r["first_below"], r["n_below"], r["first_in"] = m, argmin, first_below, n_below, first_in
    r["min_dist"] = dist[argmin] if m else F32(np.nan)
    r["grad"] = grad[argmin] if m else (0, 0)
    return r


def rollouts(f, g, pvt, voxel_width, xy, margin=0.0):
    """(records [n], dist [n][T], grad [n][T][2]) of trajectories xy [n][T][2]"""
    xy = np.asarray(xy, F32)
    n, T = xy.shape[0], xy.shape[1]
    dist, grad, flags = query(f, g, pvt, voxel_width, xy.reshape(-1, 2))
    dist, grad, flags = dist.reshape(n, T), grad.reshape(n, T, 2), flags.reshape(n, T)
    out = np.zeros(n, ROLLOUT_DTYPE)
    for i in range(n):
        out[i] = record(dist[i], grad[i], flags[i], margin)
    return out, dist, grad

"""The exhaustive statement of gie_view_gain (include/gie.h "line of sight"): every voxel of the volume is asked whether it is a
candidate, and whether it is visible.  No candidate radius, no box around the view, no clipping: what tests/los_ref.py and the
device bound by a radius derived from r_max is not derived here at all, so a shell of candidates lost by that radius shows.

Only the scalar thresholds rmin * rmin, rmax * rmax and tan2_elev are np.float32, formed as the header states them.  |d|^2 and
d_z^2 are exact integers below 2^24 (so (float) of them is the integer itself) and are compared as integers against the
thresholds' exact values; tan2_elev * (float)(d_x^2 + d_y^2) is the one float32 product the header names; the half-space tests
are int64 dot products.  The occlusion along L(p, v) comes from los_ref.Walk, the vectorised walk that tests/test_los_reference.py
holds against the rational brute force: visible_from walks it once from p to every voxel of the volume, and since visibility
does not depend on the view's ranges, band or planes the plane can be kept (`cache`) over calls with the same scene and view.

Arrays are [Z][Y][X] like Mapper.read_local; voxels are (x, y, z).  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

import los_ref as lr
from nf1_ref import point_voxels


def thresholds(r_min, r_max, tan2_elev, voxel_width):
    """(rmin * rmin, rmax * rmax, tan2_elev) as np.float32, rmin = r_min / w and rmax = r_max / w in float32 (inf when it overflows)"""
    with np.errstate(over="ignore"):
        rmin = np.float32(r_min) / np.float32(voxel_width)
        rmax = np.float32(r_max) / np.float32(voxel_width)
        return rmin * rmin, rmax * rmax, np.float32(tan2_elev)


def offsets(size, p):
    """(dx [1, 1, X], dy [1, Y, 1], dz [Z, 1, 1]) int64: v - p over the whole volume"""
    X, Y, Z = size
    return (np.arange(X, dtype=np.int64)[None, None, :] - int(p[0]), np.arange(Y, dtype=np.int64)[None, :, None] - int(p[1]),
            np.arange(Z, dtype=np.int64)[:, None, None] - int(p[2]))


def candidate_mask(size, p, rmin2, rmax2, tan2, normals=()):
    """bool [Z][Y][X]: the candidates of a view at local voxel p, by the header's four conditions over every voxel of the volume"""
    dx, dy, dz = offsets(size, p)
    dh = dx * dx + dy * dy
    dz2 = dz * dz
    d2 = dh + dz2
    assert int(d2.max()) < 2 ** 24
    ok = (d2 != 0) & (d2 >= float(rmin2)) & (d2 <= float(rmax2))          # (a float32 threshold is exact as a Python float)
    if tan2 >= 0:
        ok &= dz2 <= (np.float32(tan2) * dh.astype(np.float32)).astype(np.float64)
    for n in np.asarray(normals, np.int64).reshape(-1, 3):
        ok &= int(n[0]) * dx + int(n[1]) * dy + int(n[2]) * dz >= 0
    return ok


def visible_from(opq, p):
    """bool [Z][Y][X]: no voxel of L(p, v) other than v itself is opaque, p's own opacity ignored; for every v of the volume (p too)"""
    Z, Y, X = opq.shape
    gz, gy, gx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.int64)
    visible = np.ones(len(v), bool)
    ids = np.arange(len(v))
    w = lr.Walk(np.broadcast_to(np.asarray(p, np.int64), v.shape), v)
    while len(ids):
        moved, last = w.step()
        blocked = moved & ~last & opq[w.v[:, 2], w.v[:, 1], w.v[:, 0]]
        visible[ids[blocked]] = False
        go = moved & ~last & ~blocked
        ids = ids[go]
        w.keep(go)
    return visible.reshape(Z, Y, X)


def view_gain(vtype, opq, views, r_min, r_max, tan2_elev, voxel_width, pvt, n_visible=None, cache=None):
    """what gie_view_gain returns (los_ref.SCORE_DTYPE [n]); arguments as los_ref.view_gain.  cache: a dict that keeps
    visible_from's planes by view voxel — the caller's promise that opq is the same plane in every call that shares it."""
    vtype = np.asarray(vtype)
    Z, Y, X = opq.shape
    views = np.asarray(views, lr.VIEW_DTYPE).reshape(-1)
    rmin2, rmax2, tan2 = thresholds(r_min, r_max, tan2_elev, voxel_width)
    pv, inside = point_voxels(views["pos"], voxel_width, pvt, (X, Y, Z))
    out = np.zeros(len(views), lr.SCORE_DTYPE)
    for i, vw in enumerate(views):
        if not inside[i]:
            out[i] = (-1, -1, -1, -1)
            if n_visible is not None:
                n_visible.append(0)
            continue
        p = tuple(int(c) for c in pv[i])
        cand = candidate_mask((X, Y, Z), p, rmin2, rmax2, tan2, vw["normal"][:vw["n_planes"]])
        vis = cache.get(p) if cache is not None else None
        if vis is None:
            vis = visible_from(opq, p)
            if cache is not None:
                cache[p] = vis
        ty = vtype[cand & vis]
        if n_visible is not None:
            n_visible.append(int(len(ty)))
        out[i] = (int((ty == lr.UNKNOWN).sum()), int((ty == lr.FNT).sum()), int((ty == lr.OCCUPIED).sum()), int(cand.sum()))
    return out


def shell_count(size, p, k):
    """the number of voxels of the volume at distance exactly k (an integer) from voxel p"""
    dx, dy, dz = offsets(size, p)
    return int((dx * dx + dy * dy + dz * dz == int(k) * int(k)).sum())


# ---- the range ties: r_max / w one float32 step either side of an integer k
TIE_KS = (1, 2, 3, 5, 9, 13, 15, 17, 25)
TIE_SIZES = ((40, 36, 20), (33, 31, 29))
TIE_WIDTHS = (0.1, 0.05)


def tie_radii(k, voxel_width):
    """the float32 r_max values around k voxels, as a list without repeats: k * w, its two float32 neighbours, and whichever
    neighbouring floats make r_max / w (float32) equal exactly k, the largest quotient below k and the smallest above k"""
    w = np.float32(voxel_width)
    r0 = np.float32(k * voxel_width)
    out = [r0, np.nextafter(r0, np.float32(0)), np.nextafter(r0, np.float32(np.inf))]
    near = [r0]
    for to in (np.float32(0), np.float32(np.inf)):
        r = r0
        for _ in range(16):
            r = np.nextafter(r, to)
            near.append(r)
    near = sorted(near)
    q = [r / w for r in near]
    below = [r for r, v in zip(near, q) if v < k]
    exact = [r for r, v in zip(near, q) if v == k]
    above = [r for r, v in zip(near, q) if v > k]
    assert below and above, (k, voxel_width)
    for r in [below[-1], above[0]] + exact[:1] + exact[-1:]:
        if not any(r == s for s in out):
            out.append(r)
    return out


def tie_need(k):
    """how many voxels at distance exactly k a view of the tie tests must have: 6 — but 3 for k = 1 and 2, where the six axis
    neighbours are all the lattice has and a corner of the volume keeps three of them"""
    return 6 if k >= 3 else 3


def tie_views(size, k, n=10):
    """n local voxels for a tie radius k, each with at least tie_need(k) voxels of the volume at distance exactly k: the first n of
    a fixed list that have them — corners, points on faces and edges, points inside.  At least one corner and two face points are
    among them (asserted), whatever k leaves of the interior (from the middle of 33 x 31 x 29 no voxel is 25 away)."""
    X, Y, Z = size
    cx, cy, cz = X // 2, Y // 2, Z // 2
    pool = [(0, 0, 0), (0, cy, cz), (cx, Y - 1, cz - 2), (cx, cy, cz), (cx - 7, cy + 5, cz - 3), (X // 4, Y // 4, 3 * Z // 4), (X - 1, Y - 1, Z - 1),
            (cx + 3, cy - 2, 0), (3 * X // 4, 1, cz), (X - 1, 0, cz), (X - 1, cy + 1, Z - 1), (2, Y - 3, 1), (0, Y - 1, 0), (X - 1, cy, cz + 1),
            (cx, 0, Z - 1), (1, 1, 1), (X - 1, 0, 0), (0, 0, Z - 1)]
    assert len(set(pool)) == len(pool)
    got = [p for p in pool if shell_count(size, p, k) >= tie_need(k)][:n]
    corner = sum(all(c in (0, s - 1) for c, s in zip(p, size)) for p in got)
    face = sum(any(c in (0, s - 1) for c, s in zip(p, size)) for p in got) - corner
    assert 8 <= len(got) <= 12 and corner >= 1 and face >= 2, (size, k, got)
    return np.array(got, np.int64)

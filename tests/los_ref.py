"""The numpy statement of the line-of-sight queries (include/gie.h "line of sight"): the opaque plane, the voxel line L(a, b), the
segment checks and the view gain.  Integers everywhere, and the few float expressions written with np.float32 in the order the
header gives them, so that the device agrees bit for bit.

Arrays are [Z][Y][X] like Mapper.read_local; voxels are (x, y, z).  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

from nf1_ref import point_voxels

UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
UNKNOWN_OPAQUE = 1
HIT_DTYPE = np.dtype([("first", "<i4"), ("len", "<i4"), ("hit", "<i4", (3,)), ("min_edt", "<f4")])
VIEW_DTYPE = np.dtype([("pos", "<f4", (3,)), ("n_planes", "<i4"), ("normal", "<i4", (4, 3))])
SCORE_DTYPE = np.dtype([("unknown", "<i4"), ("frontier", "<i4"), ("occupied", "<i4"), ("candidates", "<i4")])
_DONE = np.int64(2 ** 62)


def opaque(vtype, edt, clearance=0.0, flags=0):
    """OCCUPIED, or UNKNOWN with UNKNOWN_OPAQUE, or (clearance > 0 and edt < clearance) as a float32 comparison in voxel units"""
    vtype = np.asarray(vtype)
    op = vtype == OCCUPIED
    if flags & UNKNOWN_OPAQUE:
        op = op | (vtype == UNKNOWN)
    if np.float32(clearance) > 0:
        op = op | (np.asarray(edt, np.float32) < np.float32(clearance))
    return op


def line(a, b):
    """L(a, b) as a list of (x, y, z): crossing j of axis k at t = (2j - 1) / (2 n_k); the smallest pending t is taken, all axes
    tied at it step together; two crossings are compared by (2 j_a - 1) * n_b against (2 j_b - 1) * n_a"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    n = [abs(b[k] - a[k]) for k in range(3)]
    s = [1 if b[k] > a[k] else -1 for k in range(3)]
    j = [1, 1, 1]
    v = list(a)
    out = [tuple(v)]
    while True:
        pend = [k for k in range(3) if j[k] <= n[k]]
        if not pend:
            return out
        best = pend[0]
        for k in pend[1:]:
            if (2 * j[k] - 1) * n[best] < (2 * j[best] - 1) * n[k]:
                best = k
        cb, nb = 2 * j[best] - 1, n[best]
        for k in pend:
            if (2 * j[k] - 1) * nb == cb * n[k]:
                v[k] += s[k]
                j[k] += 1
        out.append(tuple(v))


class Walk:
    """all the lines L(a[i], b[i]) stepped together: after step(), v holds every line's next voxel, moved says which lines had one
    and last which of them have arrived at b.  The crossings of a line are ordered by the integers (2j - 1) * M_k, M_k the product
    of the other two axes' n (1 for an axis that does not move): the common denominator of line()'s comparisons."""

    def __init__(self, a, b):
        a, b = np.asarray(a, np.int64).reshape(-1, 3), np.asarray(b, np.int64).reshape(-1, 3)
        n = np.abs(b - a)
        self.s = np.sign(b - a)
        nz = np.maximum(n, 1)
        M = np.stack([nz[:, 1] * nz[:, 2], nz[:, 0] * nz[:, 2], nz[:, 0] * nz[:, 1]], axis=1)
        self.D = 2 * M
        self.T = np.where(n > 0, M, _DONE)
        self.left = n.copy()
        self.v = a.copy()

    def step(self):
        t = self.T.min(axis=1)
        moved = t != _DONE
        mv = (self.T == t[:, None]) & moved[:, None]
        self.v += self.s * mv
        self.left -= mv
        self.T = np.where(mv, np.where(self.left > 0, self.T + self.D, _DONE), self.T)
        return moved, moved & (self.left.sum(axis=1) == 0)

    def keep(self, sel):
        for k in ("s", "D", "T", "left", "v"):
            setattr(self, k, getattr(self, k)[sel])


def segments(edt, opq, a_xyz, b_xyz, voxel_width, pvt):
    """what gie_los_segments returns (HIT_DTYPE [n]) for the planes of a prepare at pivot pvt"""
    Z, Y, X = opq.shape
    edt = np.asarray(edt, np.float32)
    a, ina = point_voxels(a_xyz, voxel_width, pvt, (X, Y, Z))
    b, inb = point_voxels(b_xyz, voxel_width, pvt, (X, Y, Z))
    out = np.zeros(len(a), HIT_DTYPE)
    ok = ina & inb
    out["first"][~ok] = -2
    idx = np.flatnonzero(ok)
    a, b = a[idx], b[idx]
    w = Walk(a, b)
    first = np.full(len(idx), -1, np.int64)
    hit = b.copy()
    ln = np.ones(len(idx), np.int64)
    me = np.full(len(idx), np.inf, np.float32)
    alive = np.ones(len(idx), bool)                       # the line has a voxel at this index
    k = 0
    while alive.any():
        look = alive & (first < 0)
        v = w.v[look]
        me[look] = np.minimum(me[look], edt[v[:, 2], v[:, 1], v[:, 0]])
        now = np.flatnonzero(look)[opq[v[:, 2], v[:, 1], v[:, 0]]]
        first[now] = k
        hit[now] = w.v[now]
        alive, _ = w.step()
        ln += alive
        k += 1
    out["first"][idx] = first
    out["len"][idx] = ln
    out["hit"][idx] = hit + np.asarray(pvt, np.int64)[None, :]
    out["min_edt"][idx] = me
    return out


def candidates(p, size, rmin, rmax, tan2_elev, normals):
    """(v [m, 3] int64, d [m, 3]) of the candidates of a view at local voxel p; rmin, rmax float32 in voxels"""
    X, Y, Z = size
    rmin, rmax, tan2 = np.float32(rmin), np.float32(rmax), np.float32(tan2_elev)
    R = int(min(np.ceil(rmax), 4096)) + 1
    ax = [np.arange(max(p[k] - R, 0), min(p[k] + R, s - 1) + 1, dtype=np.int64) for k, s in enumerate((X, Y, Z))]
    gz, gy, gx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    d = v - np.asarray(p, np.int64)[None, :]
    dh = d[:, 0] ** 2 + d[:, 1] ** 2
    d2 = dh + d[:, 2] ** 2
    ok = (d2 != 0) & (d2.astype(np.float32) >= rmin * rmin) & (d2.astype(np.float32) <= rmax * rmax)
    if tan2 >= 0:
        ok &= (d[:, 2] ** 2).astype(np.float32) <= tan2 * dh.astype(np.float32)
    for nm in np.asarray(normals, np.int64).reshape(-1, 3):
        ok &= d @ nm >= 0
    return v[ok], d[ok]


def view_gain(vtype, opq, views, r_min, r_max, tan2_elev, voxel_width, pvt, n_visible=None):
    """what gie_view_gain returns (SCORE_DTYPE [n]); views: VIEW_DTYPE records; r_min, r_max in metres.  Every candidate's line is
    walked from p, all lines of a view together; a line leaves the set when it is blocked or has arrived.  n_visible: a list that
    gets the number of visible candidates of every view (of any type; 0 for a view without a voxel)."""
    Z, Y, X = opq.shape
    views = np.asarray(views, VIEW_DTYPE).reshape(-1)
    rmin = np.float32(r_min) / np.float32(voxel_width)
    rmax = np.float32(r_max) / np.float32(voxel_width)
    pv, inside = point_voxels(views["pos"], voxel_width, pvt, (X, Y, Z))
    out = np.zeros(len(views), SCORE_DTYPE)
    for i, vw in enumerate(views):
        if not inside[i]:
            out[i] = (-1, -1, -1, -1)
            if n_visible is not None:
                n_visible.append(0)
            continue
        p = pv[i]
        v, _ = candidates(p, (X, Y, Z), rmin, rmax, tan2_elev, vw["normal"][:vw["n_planes"]])
        visible = np.ones(len(v), bool)
        ids = np.arange(len(v))
        w = Walk(np.broadcast_to(p, v.shape), v)
        while len(ids):
            moved, last = w.step()
            blocked = moved & ~last & opq[w.v[:, 2], w.v[:, 1], w.v[:, 0]]
            visible[ids[blocked]] = False
            go = moved & ~last & ~blocked
            ids = ids[go]
            w.keep(go)
        ty = vtype[v[visible, 2], v[visible, 1], v[visible, 0]]
        if n_visible is not None:
            n_visible.append(int(visible.sum()))
        out[i] = (int((ty == UNKNOWN).sum()), int((ty == FNT).sum()), int((ty == OCCUPIED).sum()), len(v))
    return out

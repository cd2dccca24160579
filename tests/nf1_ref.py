"""numpy statement of the NF1 navigation function (include/gie.h "navigation function"): traversability, sources, the BFS field,
the descent rule of gie_nf1_path and a local certificate that checks a field at any size.  Arrays are [Z][Y][X] like read_local."""
import numpy as np

UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
UNKNOWN_TRAVERSABLE, FROM_FRONTIERS = 1, 2
# the 6-neighbour order of the descent: -x +x -y +y -z +z, as (axis of the [Z][Y][X] array, step)
STEPS = ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))


def traversable(vtype, edt, clearance, flags=0):
    """FREE or FNT (or UNKNOWN with UNKNOWN_TRAVERSABLE), and edt >= clearance as a float32 comparison"""
    open_ = (vtype == FREE) | (vtype == FNT)
    if flags & UNKNOWN_TRAVERSABLE:
        open_ |= vtype == UNKNOWN
    return open_ & (np.asarray(edt, np.float32) >= np.float32(clearance))


def point_voxels(xyz, voxel_width, pvt, size):
    """local voxels [n, 3] (x, y, z) of points (metres) at pivot pvt: floor(p / w + 0.5) - pvt in float32; inside [n] bool"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.floor(xyz / np.float32(voxel_width) + np.float32(0.5))
        ok = np.all((u >= -1.0e9) & (u <= 1.0e9), axis=1)
        v = np.where(ok[:, None], u, 0).astype(np.int64) - np.asarray(pvt, np.int64)[None, :]
    inside = ok & np.all((v >= 0) & (v < np.asarray(size, np.int64)[None, :]), axis=1)
    return v, inside


def sources(vtype, trav, goals=(), voxel_width=1.0, pvt=(0, 0, 0), flags=0):
    """bool mask of the sources: traversable goal voxels, and traversable FNT voxels with FROM_FRONTIERS"""
    Z, Y, X = vtype.shape
    src = np.zeros(vtype.shape, bool)
    if flags & FROM_FRONTIERS:
        src |= vtype == FNT
    v, inside = point_voxels(goals, voxel_width, pvt, (X, Y, Z))
    v = v[inside]
    src[v[:, 2], v[:, 1], v[:, 0]] = True
    return src & trav


def bfs(trav, src):
    """int32 field: BFS steps to the nearest source through traversable voxels (6-connected, inside the volume), -1 elsewhere.
    A frontier-list BFS over flat indices: the cost of a level is its frontier's, so thousands of levels are cheap."""
    trav = np.asarray(trav, bool)
    Z, Y, X = trav.shape
    t = trav.ravel()
    f = np.full(t.size, -1, np.int32)
    front = np.flatnonzero(np.asarray(src, bool).ravel() & t)
    f[front] = 0
    level = 0
    while front.size:
        level += 1
        x, y, z = front % X, (front // X) % Y, front // (X * Y)
        cand = np.concatenate([front[ok] + off for ok, off in ((x > 0, -1), (x < X - 1, 1), (y > 0, -X), (y < Y - 1, X),
                                                                (z > 0, -X * Y), (z < Z - 1, X * Y))])
        cand = np.unique(cand)
        front = cand[t[cand] & (f[cand] < 0)]
        f[front] = level
    return f.reshape(trav.shape)


def field(vtype, edt, clearance=0.0, flags=0, goals=(), voxel_width=1.0, pvt=(0, 0, 0)):
    """the whole statement: (nf1, traversable, sources)"""
    trav = traversable(vtype, edt, clearance, flags)
    src = sources(vtype, trav, goals, voxel_width, pvt, flags)
    return bfs(trav, src), trav, src


def descend(f, start):
    """the descent from local voxel start = (x, y, z): the list of local voxels v0 .. vk, [] when f(start) < 0"""
    Z, Y, X = f.shape
    x, y, z = (int(c) for c in start)
    cur = int(f[z, y, x])
    if cur < 0:
        return []
    out = [(x, y, z)]
    while cur > 0:
        for ax, d in STEPS:
            q = [z, y, x]
            q[ax] += d
            if 0 <= q[ax] < f.shape[ax] and f[q[0], q[1], q[2]] == cur - 1:
                z, y, x = q
                break
        else:
            raise AssertionError("no descent step: not a BFS field")
        cur -= 1
        out.append((x, y, z))
    return out


def paths(f, starts, voxel_width, pvt, max_len):
    """what gie_nf1_path returns: (list of (min(len, max_len), 3) int32 arrays of GLOBAL voxels, len [n] int32)"""
    Z, Y, X = f.shape
    v, inside = point_voxels(starts, voxel_width, pvt, (X, Y, Z))
    out, lens = [], np.zeros(len(v), np.int32)
    for i in range(len(v)):
        p = descend(f, v[i]) if inside[i] else []
        lens[i] = len(p)
        a = np.array(p[:max_len], np.int64).reshape(-1, 3) + np.asarray(pvt, np.int64)[None, :]
        out.append(a.astype(np.int32))
    return out, lens


_NONE = np.iinfo(np.int32).max


def _neighbour_min(f, trav):
    """per voxel: the minimum of the non-negative values of its traversable in-volume 6-neighbours (_NONE where there is none)"""
    vals = np.where(trav & (f >= 0), f, _NONE).astype(np.int32)
    m = np.full(f.shape, _NONE, np.int32)
    for ax in range(3):
        if f.shape[ax] < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        np.minimum(m[tuple(lo)], vals[tuple(hi)], out=m[tuple(lo)])
        np.minimum(m[tuple(hi)], vals[tuple(lo)], out=m[tuple(hi)])
    return m


def certificate(f, trav, src):
    """'' when f is the BFS field of (trav, src), else the reason.  Local, so it scales to 512^3:
    the sources are exactly the voxels with value 0; every other voxel with a value is traversable and equals 1 + the minimum
    over its valued traversable neighbours; no traversable voxel without a value touches a voxel with one."""
    f = np.asarray(f)
    trav = np.asarray(trav, bool)
    src = np.asarray(src, bool) & trav
    if not np.array_equal(f == 0, src):
        return "value 0 is not exactly the sources"
    if (f < -1).any():
        return "values below -1"
    valued = f >= 0
    if (valued & ~trav).any():
        return "a value at a voxel that is not traversable"
    m = _neighbour_min(f, trav)
    inner = valued & ~src
    mi = m[inner]
    if (mi == _NONE).any() or not np.array_equal(f[inner].astype(np.int64), mi.astype(np.int64) + 1):
        return "a value that is not 1 + its neighbours' minimum"
    if (trav & ~valued & (m != _NONE)).any():
        return "a traversable voxel without a value next to one with a value"
    return ""

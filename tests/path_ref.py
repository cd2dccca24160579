"""The numpy statement of path shortcutting (include/gie.h "path shortcutting"): greedy waypoints along a polyline of voxels over
the opaque plane and the edt copy of a prepare.  It builds on los_ref's voxel line; integers everywhere, the minima and the one
float sum through np.float32 in the order the header gives them, so that the device agrees bit for bit.

Arrays are [Z][Y][X] like Mapper.read_local; voxels are (x, y, z).  Test infrastructure only: numpy, nothing of the device."""
import numpy as np

import los_ref as lr

WAYPOINT_DTYPE = np.dtype([("xyz", "<i4", (3,)), ("index", "<i4"), ("min_edt", "<f4"), ("forced", "<i4")])
INFO_DTYPE = np.dtype([("count", "<i4"), ("forced", "<i4"), ("length", "<f4"), ("reserved", "<i4")])


def local(points, pvt, size):
    """(local voxels int64 [.., 3], inside [..]) of global int32 points; the difference in 64 bits"""
    v = np.asarray(points, np.int64) - np.asarray(pvt, np.int64)
    return v, np.all((v >= 0) & (v < np.asarray(size, np.int64)), axis=-1)


def clear_lines(opq, a, b):
    """which of the lines L(a[i], b[i]) between voxels INSIDE the volume have no opaque voxel (both ends included), all lines
    stepped together and a line dropped at its first opaque voxel"""
    a, b = np.asarray(a, np.int64).reshape(-1, 3), np.asarray(b, np.int64).reshape(-1, 3)
    ok = ~opq[a[:, 2], a[:, 1], a[:, 0]]
    ids = np.flatnonzero(ok)
    w = lr.Walk(a[ids], b[ids])
    while len(ids):
        moved, _ = w.step()
        hit = np.zeros(len(ids), bool)
        v = w.v[moved]
        hit[moved] = opq[v[:, 2], v[:, 1], v[:, 0]]
        ok[ids[hit]] = False
        go = moved & ~hit
        ids = ids[go]
        w.keep(go)
    return ok


def line_min_edt(edt, a, b):
    """the float32 minimum of edt over the voxels of L(a, b)"""
    v = np.array(lr.line(a, b), np.int64)
    return np.asarray(edt, np.float32)[v[:, 2], v[:, 1], v[:, 0]].min()


def windows(opq, paths, ms, pvt, lookahead):
    """the greedy walk of every path (path i: its first ms[i] points): per path a list of (k, top, clear), one per leg, clear the
    bool array over the window's indices k + 1 .. top.  A window is decided as a whole — every candidate, not up to the first
    blocked one; the legs of all paths advance together, one clear_lines per round."""
    paths = np.asarray(paths, np.int32)
    Z, Y, X = opq.shape
    ms = np.asarray(ms, np.int64)
    v, inside = local(paths, pvt, (X, Y, Z))
    out = [[] for _ in ms]
    k = np.zeros(len(ms), np.int64)
    while True:
        act = np.flatnonzero(k < ms - 1)
        if not len(act):
            return out
        top = np.minimum(k[act] + int(lookahead), ms[act] - 1)
        cnt = top - k[act]
        start = np.cumsum(cnt) - cnt
        pi, pk = np.repeat(act, cnt), np.repeat(k[act], cnt)
        pj = np.arange(cnt.sum()) - np.repeat(start, cnt) + pk + 1
        sel = inside[pi, pk] & inside[pi, pj]
        clear = np.zeros(len(pi), bool)
        clear[sel] = clear_lines(opq, v[pi[sel], pk[sel]], v[pi[sel], pj[sel]])
        for q, i in enumerate(act):
            c = clear[start[q]:start[q] + cnt[q]]
            out[i].append((int(k[i]), int(top[q]), c))
            k[i] = k[i] + 1 + int(np.flatnonzero(c)[-1]) if c.any() else k[i] + 1


def shortcut(edt, opq, paths, lens, pvt, lookahead, max_wp, wp_init=None, legs=None):
    """what gie_path_shortcut returns: (wp [n, max_wp] WAYPOINT_DTYPE, info [n] INFO_DTYPE) for the planes of a prepare at pivot pvt.
    paths: (n, max_len, 3) int32 global voxels; wp_init: what the caller's array held (zeros when None) — entries beyond a path's
    records keep it.  legs: an empty list gets every path's windows(); one that has them (the same planes, paths and lookahead: they
    do not depend on max_wp or wp_init) spares computing them again."""
    paths = np.asarray(paths, np.int32)
    n, max_len = paths.shape[0], paths.shape[1]
    lens = np.asarray(lens, np.int32).reshape(-1)
    Z, Y, X = opq.shape
    edt = np.asarray(edt, np.float32)
    wp = np.zeros((n, max_wp), WAYPOINT_DTYPE) if wp_init is None else np.array(wp_init, WAYPOINT_DTYPE).reshape(n, max_wp)
    info = np.zeros(n, INFO_DTYPE)
    ms = np.clip(lens.astype(np.int64), 0, max_len)
    if legs is None:
        legs = []
    if not legs:
        legs.extend(windows(opq, paths, ms, pvt, lookahead))
    for i in range(n):
        m, win = int(ms[i]), legs[i]
        if m == 0:
            continue
        v, inside = local(paths[i, :m], pvt, (X, Y, Z))
        rec = [(0, np.float32(edt[v[0, 2], v[0, 1], v[0, 0]]) if inside[0] else np.float32(-1.0), 0)]
        length, forced = np.float32(0.0), 0
        for k, top, clear in win:
            if clear.any():
                j = k + 1 + int(np.flatnonzero(clear)[-1])
                d2 = int(((v[j] - v[k]) ** 2).sum())
                length = np.float32(length + np.sqrt(np.float32(d2)))
                rec.append((j, line_min_edt(edt, v[k], v[j]), 0))
            else:
                forced += 1
                rec.append((k + 1, np.float32(-1.0), 1))
        assert rec[-1][0] == m - 1
        info[i] = (len(rec), forced, length, 0)
        for t, (j, me, f) in enumerate(rec[:max_wp]):
            wp[i, t] = (paths[i, j], j, me, f)
    return wp, info

"""Scenes and path sets that the CPU and the device tests of path shortcutting share (tests/path_ref.py is the statement they are
compared with).  Volumes are label planes [Z][Y][X] (1 free, 2 occupied, 0 never seen); paths are LOCAL voxels here, the tests add
the pivot.  Test infrastructure only."""
import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def pillar_scene(long):
    """(size, labels, path [m, 3] local voxels): a thin volume with occupied pillars in its middle row y = 4 (at all z) and a path
    that climbs the low-x face and then runs along the row y = 8, so that from its first point the pillars' shadows hide stretches
    of it and let the points behind them through.  long: volume (300, 9, 2), pillars at x = 20 and x = 60..140, 308 points;
    otherwise volume (130, 9, 2), pillars at x = 20 and x = 60, 138 points."""
    size = (300, 9, 2) if long else (130, 9, 2)
    lab = np.ones(size[::-1], np.int8)
    lab[:, 4, 20] = 2
    if long:
        lab[:, 4, 60:141] = 2
    else:
        lab[:, 4, 60] = 2
    path = [(0, y, 0) for y in range(9)] + [(x, 8, 0) for x in range(1, size[0])]
    return size, lab, np.array(path, np.int64)


def staircase(n, start=(1, 1, 1)):
    """n points of a 6-connected staircase that steps +x, +y, +z in turn"""
    p = [np.array(start, np.int64)]
    for i in range(n - 1):
        d = np.zeros(3, np.int64)
        d[i % 3] = 1
        p.append(p[-1] + d)
    return np.array(p)


def pack(paths, max_len, pvt, fill=0):
    """(buffer [n, max_len, 3] int32 of GLOBAL voxels, lens [n] int32) from a list of local paths, as gie_nf1_path leaves them:
    len is the path's own length also beyond max_len, the points beyond a path are `fill`"""
    buf = np.full((len(paths), max_len, 3), fill, np.int32)
    lens = np.zeros(len(paths), np.int32)
    for i, p in enumerate(paths):
        p = np.asarray(p, np.int64).reshape(-1, 3)
        lens[i] = len(p)
        g = np.clip(p[:max_len] + np.asarray(pvt, np.int64), INT_MIN, INT_MAX)
        buf[i, :len(g)] = g.astype(np.int32)
    return buf, lens


def answer_chunks(legs):
    """per leg with an answer, of all paths: (the chunk of 64 candidates, counted from the window's top, that holds the answer;
    whether a blocked index lies below the answer in the window)"""
    out = []
    for win in legs:
        for k, top, clear in win:
            if clear.any():
                j = k + 1 + int(np.flatnonzero(clear)[-1])
                out.append(((top - j) // 64, not clear[:j - k - 1].all()))
    return out


def random_boxes_labels(rng, size, nbox, smin=2, smax=7):
    X, Y, Z = size
    lab = np.ones((Z, Y, X), np.int8)
    for _ in range(nbox):
        s = rng.integers(smin, smax, 3)
        lo = rng.integers(0, np.maximum(np.array(size) - s, 1))
        lab[lo[2]:lo[2] + s[2], lo[1]:lo[1] + s[1], lo[0]:lo[0] + s[0]] = 2
    return lab


def polylines(rng, size, n, max_len):
    """n arbitrary polylines of local voxels (lists of [len, 3] int64; a len may exceed max_len: the tail is cut by pack) made of
    short hops, random voxels, jumps across the whole volume, repeats and points up to 5 voxels outside, with the lens 0, 1, 2,
    max_len - 1, max_len, max_len + 1 and 500 first"""
    S = np.array(size, np.int64)
    lens = [0, 1, 2, max_len - 1, max_len, max_len + 1, 500] + [int(v) for v in rng.integers(3, max_len + 1, max(n - 7, 0))]
    out = []
    for i, m in enumerate(lens[:n]):
        p = np.zeros((m, 3), np.int64)
        cur = rng.integers(0, S)
        for t in range(m):
            kind = rng.integers(0, 10)
            if kind < 5:
                cur = np.clip(cur + rng.integers(-3, 4, 3), 0, S - 1)              # a short hop
            elif kind < 7:
                cur = rng.integers(0, S)                                            # any voxel
            elif kind == 7:
                cur = np.where(rng.integers(0, 2, 3) == 1, S - 1 - cur, cur)        # across the whole volume
            elif kind == 8:
                pass                                                                # a repeat
            else:
                cur = rng.integers(-5, S + 5)                                       # up to 5 voxels outside
            p[t] = cur
            if kind == 9:
                cur = np.clip(cur, 0, S - 1)
        out.append(p)
    return out

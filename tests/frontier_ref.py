"""numpy / scipy statement of the frontier clusters (include/gie.h "frontier clusters"): members, components by
scipy.ndimage.label, canonical labels, sizes, sums, boxes, representative voxels, centroids, the -1 / -2 label plane, the capacity
rule and the goal array.  Shares nothing with the device code.  Arrays are [Z][Y][X] like read_local."""
import numpy as np
from scipy import ndimage

UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
CLUSTER_DTYPE = np.dtype([("label", "<i4"), ("size", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("rep", "<i4", (3,)),
                          ("centroid", "<f4", (3,)), ("sum", "<i8", (3,))])
assert CLUSTER_DTYPE.itemsize == 80 and CLUSTER_DTYPE.fields["sum"][1] == 56


def members(vtype, edt, clearance):
    """FNT and edt >= clearance as a float32 comparison"""
    return (np.asarray(vtype) == FNT) & (np.asarray(edt, np.float32) >= np.float32(clearance))


def structure(connectivity):
    if connectivity not in (6, 26):
        raise ValueError("connectivity is 6 or 26")
    return ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)


def components(mask, connectivity):
    """(ids, comp, canon, size): the members' linear indices (ascending), the component number 0 .. n-1 of each, and per component
    its label (the smallest index of a member: ndimage.minimum of the index plane at the members) and its size"""
    mask = np.asarray(mask, bool)
    lab, n = ndimage.label(mask, structure=structure(connectivity))
    ids = np.flatnonzero(mask.ravel())
    comp = lab.ravel()[ids].astype(np.int64) - 1
    if n == 0:
        return ids, comp, np.zeros(0, np.int64), np.zeros(0, np.int64), lab
    canon = np.asarray(ndimage.minimum(ids, labels=comp + 1, index=np.arange(1, n + 1)), np.int64)
    size = np.bincount(comp, minlength=n).astype(np.int64)
    return ids, comp, canon, size, lab


def clusters(mask, connectivity=26, min_size=1, max_clusters=256, pvt=(0, 0, 0), voxel_width=1.0):
    """the whole statement: dict(labels int32 [Z][Y][X], n_clusters, n_voxels, records CLUSTER_DTYPE [min(n_clusters, max_clusters)],
    goals float32 [max_clusters, 3])"""
    if min_size < 1 or max_clusters < 0:
        raise ValueError("min_size >= 1 and max_clusters >= 0")
    mask = np.asarray(mask, bool)
    Z, Y, X = mask.shape
    pvt = np.asarray(pvt, np.int64)
    w = np.float32(voxel_width)
    ids, comp, canon, size, lab = components(mask, connectivity)
    kept = size >= min_size
    labels = np.full(mask.size, -1, np.int32)
    labels[ids] = np.where(kept[comp], canon[comp], -2).astype(np.int32)
    order = np.flatnonzero(kept)
    order = order[np.argsort(canon[order], kind="stable")]               # ascending label
    n_clusters = int(order.size)
    n_voxels = int(size[order].sum())
    x, y, z = ids % X, (ids // X) % Y, ids // (X * Y)
    n = size.size
    # (bincount's weighted sums are float64: exact, the largest is below 2^53 by far)
    sums = np.stack([np.bincount(comp, weights=a, minlength=n) for a in (x, y, z)], axis=1).astype(np.int64) if n else np.zeros((0, 3), np.int64)
    boxes = ndimage.find_objects(lab)
    by_comp = np.argsort(comp, kind="stable")
    start = np.concatenate([[0], np.cumsum(size)[:-1]]) if n else np.zeros(0, np.int64)
    rec = np.zeros(min(n_clusters, max_clusters), CLUSTER_DTYPE)
    goals = np.full((max_clusters, 3), np.nan, np.float32)
    for r, k in enumerate(order[:max_clusters]):
        sz, sm = int(size[k]), sums[k]
        sl = boxes[k]
        lo = np.array([sl[2].start, sl[1].start, sl[0].start], np.int64)
        hi = np.array([sl[2].stop, sl[1].stop, sl[0].stop], np.int64) - 1
        mine = ids[by_comp[start[k]:start[k] + sz]]                        # ascending: the sort is stable
        assert mine.size == sz and mine[0] == canon[k]
        mx, my, mz = mine % X, (mine // X) % Y, mine // (X * Y)
        c = (2 * sm + sz) // (2 * sz)                                    # the centroid rounded half up to a voxel
        d2 = (mx - c[0]) ** 2 + (my - c[1]) ** 2 + (mz - c[2]) ** 2
        j = int(np.argmin(d2))                                           # (the first minimum: the smaller index)
        repl = np.array([mx[j], my[j], mz[j]], np.int64)
        q = rec[r]
        q["label"], q["size"] = canon[k], sz
        q["lo"], q["hi"], q["rep"], q["sum"] = lo + pvt, hi + pvt, repl + pvt, sm
        q["centroid"] = ((sm.astype(np.float64) / np.float64(sz)).astype(np.float32) + pvt.astype(np.float32)) * w
        g = (repl + pvt).astype(np.float32) * w
        back = np.floor(g / w + np.float32(0.5))
        assert np.array_equal(back.astype(np.int64), repl + pvt), (g, repl + pvt)    # gie_pos2coord gives rep back
        goals[r] = g
    return dict(labels=labels.reshape(mask.shape), n_clusters=n_clusters, n_voxels=n_voxels, records=rec, goals=goals)


def flood_fill(mask, connectivity):
    """plain Python: {label: sorted list of member indices}, label = the smallest index of the component"""
    mask = np.asarray(mask, bool)
    Z, Y, X = mask.shape
    if connectivity == 6:
        steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    else:
        steps = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    seen = np.zeros(mask.shape, bool)
    out = {}
    for z0, y0, x0 in np.argwhere(mask):                                 # ascending index
        if seen[z0, y0, x0]:
            continue
        seen[z0, y0, x0] = True
        stack, mem = [(int(x0), int(y0), int(z0))], []
        while stack:
            x, y, z = stack.pop()
            mem.append((z * Y + y) * X + x)
            for dx, dy, dz in steps:
                a, b, c = x + dx, y + dy, z + dz
                if 0 <= a < X and 0 <= b < Y and 0 <= c < Z and mask[c, b, a] and not seen[c, b, a]:
                    seen[c, b, a] = True
                    stack.append((a, b, c))
        mem.sort()
        out[mem[0]] = mem
    return out

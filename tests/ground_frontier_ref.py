"""numpy / scipy statement of the ground frontier clusters (include/gie.h "ground frontier clusters") on top of ground_ref's planes:
members from type and dist_sq, components by scipy.ndimage.label, canonical labels, sizes, sums, boxes, representative cells and
their dist_sq, centroids, the -1 / -2 label plane, the capacity rule, the goal array — and the gather of the ground navigation
function on top of ground_nf1_ref.  Shares nothing with the device code.

Cell planes are [Y][X]; f is ground_ref.field's dict (or Mapper.read_ground's: only "type" and "dist_sq" are read); pvt the ground
field's pivot."""
import numpy as np
from scipy import ndimage

import ground_nf1_ref as N
import ground_ref as G

CLUSTER_DTYPE = np.dtype([("label", "<i4"), ("size", "<i4"), ("lo", "<i4", (2,)), ("hi", "<i4", (2,)), ("rep", "<i4", (2,)),
                          ("centroid", "<f4", (2,)), ("sum", "<i8", (2,)), ("rep_dist_sq", "<i4"), ("reserved", "<i4")])
assert CLUSTER_DTYPE.itemsize == 64 and CLUSTER_DTYPE.fields["sum"][1] == 40


def members(f, clearance_sq=0):
    """FNT, and dist_sq == -1 or dist_sq >= clearance_sq: ground NF1's traversable rule restricted to FNT cells"""
    t, d = np.asarray(f["type"]), np.asarray(f["dist_sq"])
    return (t == G.FNT) & ((d == -1) | (d >= clearance_sq))


def structure(connectivity):
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    return ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)      # the cross, or the full 3 x 3


def components(mask, connectivity):
    """(ids, comp, canon, size, lab): the members' cell indices (ascending), the component number 0 .. n-1 of each, per component
    its label (the smallest index of a member: ndimage.minimum of the index plane at the members) and its size, scipy's plane"""
    mask = np.asarray(mask, bool)
    lab, n = ndimage.label(mask, structure=structure(connectivity))
    ids = np.flatnonzero(mask.ravel())
    comp = lab.ravel()[ids].astype(np.int64) - 1
    if n == 0:
        return ids, comp, np.zeros(0, np.int64), np.zeros(0, np.int64), lab
    canon = np.asarray(ndimage.minimum(ids, labels=comp + 1, index=np.arange(1, n + 1)), np.int64)
    size = np.bincount(comp, minlength=n).astype(np.int64)
    return ids, comp, canon, size, lab


def clusters_of_mask(mask, dist_sq, connectivity=8, min_size=1, max_clusters=256, pvt=(0, 0), voxel_width=1.0):
    """the whole statement for a member plane: dict(labels int32 [Y][X], n_clusters, n_cells, records CLUSTER_DTYPE
    [min(n_clusters, max_clusters)], goals float32 [max_clusters, 2]); dist_sq [Y][X] gives rep_dist_sq.  For the tests' own
    conditions also n_members, n_dropped (components that are not kept) and sizes (of ALL kept components, ascending label)"""
    if min_size < 1 or max_clusters < 0:
        raise ValueError("min_size >= 1 and max_clusters >= 0")
    mask = np.asarray(mask, bool)
    dist_sq = np.asarray(dist_sq)
    Y, X = mask.shape
    pvt = np.asarray(pvt[:2], np.int64)
    w = np.float32(voxel_width)
    ids, comp, canon, size, lab = components(mask, connectivity)
    kept = size >= min_size
    labels = np.full(mask.size, -1, np.int32)
    labels[ids] = np.where(kept[comp], canon[comp], -2).astype(np.int32)
    order = np.flatnonzero(kept)
    order = order[np.argsort(canon[order], kind="stable")]               # ascending label
    n_clusters = int(order.size)
    n_cells = int(size[order].sum())
    x, y = ids % X, ids // X
    n = size.size
    # (bincount's weighted sums are float64: exact, the largest is below 2^53 by far)
    sums = np.stack([np.bincount(comp, weights=a, minlength=n) for a in (x, y)], axis=1).astype(np.int64) if n else np.zeros((0, 2), np.int64)
    boxes = ndimage.find_objects(lab)
    by_comp = np.argsort(comp, kind="stable")
    start = np.concatenate([[0], np.cumsum(size)[:-1]]) if n else np.zeros(0, np.int64)
    rec = np.zeros(min(n_clusters, max_clusters), CLUSTER_DTYPE)
    goals = np.full((max_clusters, 2), np.nan, np.float32)
    for r, k in enumerate(order[:max_clusters]):
        sz, sm = int(size[k]), sums[k]
        sl = boxes[k]
        lo = np.array([sl[1].start, sl[0].start], np.int64)
        hi = np.array([sl[1].stop, sl[0].stop], np.int64) - 1
        mine = ids[by_comp[start[k]:start[k] + sz]]                        # ascending: the sort is stable
        assert mine.size == sz and mine[0] == canon[k]
        mx, my = mine % X, mine // X
        c = (2 * sm + sz) // (2 * sz)                                    # the centroid rounded half up to a cell
        d2 = (mx - c[0]) ** 2 + (my - c[1]) ** 2
        j = int(np.argmin(d2))                                           # (the first minimum: the smaller index)
        repl = np.array([mx[j], my[j]], np.int64)
        q = rec[r]
        q["label"], q["size"] = canon[k], sz
        q["lo"], q["hi"], q["rep"], q["sum"] = lo + pvt, hi + pvt, repl + pvt, sm
        q["centroid"] = ((sm.astype(np.float64) / np.float64(sz)).astype(np.float32) + pvt.astype(np.float32)) * w
        q["rep_dist_sq"] = dist_sq[repl[1], repl[0]]
        g = (repl + pvt).astype(np.float32) * w
        back = np.floor(g / w + np.float32(0.5))
        assert np.array_equal(back.astype(np.int64), repl + pvt), (g, repl + pvt)    # gie_pos2coord gives rep back
        goals[r] = g
    return dict(labels=labels.reshape(mask.shape), n_clusters=n_clusters, n_cells=n_cells, records=rec, goals=goals,
                n_members=int(ids.size), n_dropped=int(n - n_clusters), sizes=size[order])


def clusters(f, clearance_sq=0, connectivity=8, min_size=1, max_clusters=256, pvt=(0, 0), voxel_width=1.0):
    """the statement on a ground field"""
    if clearance_sq < 0:
        raise ValueError("clearance_sq >= 0")
    return clusters_of_mask(members(f, clearance_sq), f["dist_sq"], connectivity, min_size, max_clusters, pvt, voxel_width)


def gather(nf, xy, pvt, voxel_width):
    """gie_ground_nf1_query: int32 [n], the field nf [Y][X] at the cell of each world point, -1 outside and for points not finite"""
    cells = N.cells_of(xy, pvt, voxel_width, nf.shape)
    return np.array([-1 if c is None else nf[c[1], c[0]] for c in cells], np.int32).reshape(-1)


def route_steps(f, robot_xy, goals_xy, pvt, voxel_width, clearance_sq=0):
    """the chain: ground NF1 whose only goal is the robot, gathered at the goal array"""
    nf, _ = N.field(f, np.asarray(robot_xy, np.float32).reshape(1, 2), pvt, voxel_width, clearance_sq, 0)
    return gather(nf, goals_xy, pvt, voxel_width)


def flood_fill(mask, connectivity):
    """plain Python, one cell at a time: {label: sorted list of member indices}, label = the smallest index of the component"""
    mask = np.asarray(mask, bool)
    Y, X = mask.shape
    if connectivity == 4:
        steps = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    else:
        steps = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
    seen = np.zeros(mask.shape, bool)
    out = {}
    for y0, x0 in np.argwhere(mask):                                     # ascending index
        if seen[y0, x0]:
            continue
        seen[y0, x0] = True
        stack, mem = [(int(x0), int(y0))], []
        while stack:
            x, y = stack.pop()
            mem.append(y * X + x)
            for dx, dy in steps:
                a, b = x + dx, y + dy
                if 0 <= a < X and 0 <= b < Y and mask[b, a] and not seen[b, a]:
                    seen[b, a] = True
                    stack.append((a, b))
        mem.sort()
        out[mem[0]] = mem
    return out

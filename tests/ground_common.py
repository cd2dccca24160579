"""What the device tests of the ground stages (costmap, NF1, line of sight, frontier clusters, cost matrix, view gain, rollouts,
footprints, pose NF1) share on top of stage_common: the settled mapper and its ground field, local cells to world points, the label
scenes, and the field-by-field comparison of record arrays."""
import numpy as np

import ground_ref as R
from gie import scenes
from stage_common import W, box_labels, update

INVALID = 1                                                     # GIE_ERR_INVALID
POISON = 0x5a5a5a5a
P5A = bytes([0x5a])


def settle(m, lab, pos=(0.0, 0.0, 0.0)):
    """two updates of one label volume at one pose: the pivot"""
    pos = tuple(np.float32(v) for v in pos)
    for _ in range(2):
        update(m, pos, (1.0, 0.0, 0.0, 0.0), lab)
    return m.pivot()


def ground(m, size, band=None, blocks=False, min_known=1):
    """the ground field of the local layers band = (lo, hi) (default: the whole height): read_ground()'s planes"""
    z = m.pivot()[2]
    lo, hi = band if band is not None else (0, size[2] - 1)
    m.ground_compute(z + lo, z + hi, min_known, blocks)
    return m.read_ground()


def xy(pvt, cells, shift=0.0):
    """world points (float32 metres) of local cells (any shape (.., 2), fractions allowed): (cell + pvt + shift) * w, the product in float32"""
    c = np.asarray(cells, np.float64) + np.array(pvt[:2])
    return ((c.astype(np.float32) + np.float32(shift)) * np.float32(W)).astype(np.float32)


def plane(size, lab2d):
    """a [Y][X] label plane on every layer"""
    return np.repeat(np.asarray(lab2d, np.int8)[None], size[2], axis=0)


def scene(size, seed, n_boxes=14, unknown_slab=4, pos_k=2, smax=9):
    """(pose, labels) of n_boxes random boxes of sides 2 .. smax - 1 around the volume of pose pos_k"""
    rng = np.random.default_rng(seed)
    pos, q = scenes.pose(pos_k, W, delta_vox=3, yaw_deg=0.0)
    pvt = scenes.local_pivot(pos, W, size)
    boxes = []
    for _ in range(n_boxes):
        s = rng.integers(2, smax, size=3)
        c = rng.integers(np.asarray(pvt) - 2, np.asarray(pvt) + np.asarray(size))
        boxes.append((c, c + s))
    return pos, box_labels(pvt, size, 0, boxes, unknown_slab)


def framed(X, Y, fill=1):
    lab = np.full((Y, X), fill, np.int8)
    lab[0] = lab[-1] = 2
    lab[:, 0] = lab[:, -1] = 2
    return lab


def serpentine(X, Y, pitch):
    """(label plane [Y][X], the cells (x, y) in order) of ONE one-cell-wide corridor through walls: rows `pitch` apart from y = 1,
    each from x = 1 to X - 2, joined at alternating ends"""
    lab = np.full((Y, X), 2, np.int8)
    cells = []
    rows = list(range(1, Y - 1, pitch))
    for i, y in enumerate(rows):
        xs = list(range(1, X - 1)) if i % 2 == 0 else list(range(X - 2, 0, -1))
        cells += [(x, y) for x in xs]
        if i + 1 < len(rows):
            cells += [(xs[-1], yy) for yy in range(y + 1, rows[i + 1])]
    c = np.array(cells)
    lab[c[:, 1], c[:, 0]] = 1
    return lab, c


def chain_scene(X=64, Y=40, pillars=False):
    """free space in a frame; a closed room with a never-seen cell inside (a ring the robot cannot reach), never-seen lines and cells
    outside it (arcs and rings it can); with `pillars` a few of those too"""
    lab = framed(X, Y)
    lab[5:14, 40:52] = 2
    lab[6:13, 41:51] = 1
    lab[9, 45] = 0
    lab[20:30, 12] = 0
    lab[30, 30:44] = 0
    lab[8, 8] = lab[34, 55] = lab[16, 30] = 0
    if pillars:
        lab[24:28, 20:23] = 2
        lab[14:17, 56:60] = 2
    return lab


def same(got, want, what):
    """two record arrays: field by field (the failing field is named), then byte for byte"""
    for key in want.dtype.names:
        assert np.array_equal(got[key], want[key]), (what, key, got[key].tolist(), want[key].tolist())
    assert got.tobytes() == want.tobytes(), what


def open_cells(g):
    """bool [Y][X]: FREE or FNT columns (a FNT column is a free one with a never-seen voxel beside it: over the whole height of a
    volume that is nearly every free column)"""
    t = np.asarray(g["type"])
    return (t == R.FREE) | (t == R.FNT)


def arc(start, heading, step, turn, T):
    """T poses of a unicycle arc, steps of `step` cells, the heading turning by `turn` radians per step: (cells with fractions [T][2],
    headings int32 [T][2] = lround(32767 (cos, sin)) of the true heading)"""
    k = np.arange(T)
    th = heading + turn * k
    d = np.stack([np.cos(th), np.sin(th)], 1)
    pts = np.asarray(start, np.float64) + np.concatenate([np.zeros((1, 2)), np.cumsum(d[:-1] * step, 0)])
    return pts, np.rint(32767.0 * d).astype(np.int32)

"""Scenes with deep obstacle interiors at any shape of the local volume, for the planner-facing fields (signed distance, NF1, frontier
clusters), with the properties the device tests assert on what read_local returns and the shape table those tests run over.

Arrays are [Z][Y][X] like Mapper.read_local; sizes are (X, Y, Z).  Labels: 0 never seen / 1 free / 2 occupied (Mapper.ogm_labels).
Test infrastructure only: numpy, nothing of the device."""
import math

import numpy as np

OCCUPIED = 2


def sdf_cp(size):
    """the k_sdf_line<CP, .> instantiation gie_sdf_ready selects for a volume (csrc/gie_sdf.inc.h): by L = max(Y, Z)"""
    L = max(size[1], size[2])
    for cp in (1, 2, 4, 8):
        if L <= 64 * cp:
            return cp
    return 16


# (size, CP): every shape the signed distance is compared at, with the line kernel it drives
SDF_SIZES = [
    # CP 1 / 2 borders
    ((72, 64, 40), 1), ((72, 65, 40), 2), ((72, 40, 128), 2), ((72, 40, 129), 4),
    # CP 4, CP 8
    ((200, 256, 24), 4), ((96, 40, 200), 4), ((64, 257, 24), 8), ((48, 24, 512), 8),
    # CP 16
    ((16, 24, 600), 16), ((16, 1024, 12), 16), ((12, 16, 1024), 16), ((24, 513, 16), 16),
    # long x: up to 16 words per bit row
    ((1024, 16, 12), 1), ((1000, 24, 20), 1), ((320, 320, 40), 8),
    # word borders in x
    ((63, 20, 20), 1), ((64, 20, 20), 1), ((65, 20, 20), 1), ((127, 9, 7), 1), ((128, 8, 8), 1), ((129, 7, 9), 1), ((193, 24, 17), 1),
    # degenerate axes
    ((1, 40, 40), 1), ((40, 1, 40), 1), ((40, 40, 1), 1), ((1, 1, 40), 1), ((1, 300, 1), 8), ((300, 1, 1), 1), ((2, 2, 2), 1),
    ((2, 300, 2), 8), ((1, 1, 1), 1),
]
BIG_SIZES = [((256, 256, 256), 4), ((512, 512, 512), 8)]
QUERY_SIZES = [(1, 40, 40), (40, 1, 40), (2, 2, 2), (2, 300, 2), (65, 20, 20), (1024, 16, 12), (16, 1024, 12)]
RIDER_SIZES = [(1, 40, 40), (40, 1, 40), (65, 20, 20), (193, 24, 17), (1024, 16, 12), (16, 1024, 12), (12, 16, 1024), (1000, 24, 20)]


def _put(lab, lo, hi, v=OCCUPIED):
    """lab[lo, hi) = v, (x, y, z) bounds clipped to the volume"""
    Z, Y, X = lab.shape
    lo = [max(int(a), 0) for a in lo]
    hi = [min(int(b), s) for b, s in zip(hi, (X, Y, Z))]
    lab[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = v


def deep_target(size):
    """the depth (voxels) a scene's deepest interior voxel must reach: an eighth of the shortest side longer than 2, of 400 at most"""
    long_sides = [s for s in size if s > 2]
    return min(min(long_sides), 400) / 8.0 if long_sides else 0.0


def solid_labels(size, seed=0, fill=0.0):
    """int8 [Z][Y][X] labels of a scene of solid boxes whose sides scale with the volume's:
      * a core box deep enough for deep_target(size) (it spans the axes of length 1 and 2, where out of the volume is no site);
      * a beam along x over 70 % of X: occupied runs longer than 128 voxels when X >= 192, many all-occupied words at X ~ 1000;
      * a column along y and one along z over 70 % of those axes, three voxels thick: lines that are mostly occupied;
      * small cubes of side 3 (one interior voxel each: lines with a single interior voxel) and random boxes;
      * a box through each of the six faces;
      * `fill` > 0: a block over the whole cross-section at the low end of the longest axis, that share of it long (the queries
        want a large share of deep interior);
      * never-seen voxels in free space only: a slab at the high end of the longest axis, blocks of side 3 and single specks.
    A volume without a side above 2 is occupied but for its last voxel (1 x 1 x 1: occupied)."""
    X, Y, Z = (int(s) for s in size)
    S = (X, Y, Z)
    rng = np.random.default_rng([int(seed), X, Y, Z])
    if max(S) <= 2:
        lab = np.full((Z, Y, X), OCCUPIED, np.int8)
        if X * Y * Z > 1:
            lab[-1, -1, -1] = 1
        return lab
    lab = np.ones((Z, Y, X), np.int8)
    half = int(math.ceil(deep_target(size)))
    # core: centre voxel `half` voxels from the box's faces along every axis longer than 2
    side = [s if s <= 2 else min(2 * half - 1, s - 2) if s > 4 else 1 for s in S]
    lo = [(s - d) // 2 + (1 if s - d > 4 else 0) for s, d in zip(S, side)]
    _put(lab, lo, [a + d for a, d in zip(lo, side)])
    # beam along x, columns along y and z: 70 % of the axis, three voxels thick (clipped), off the centre
    for ax in range(3):
        n = S[ax]
        a0 = n // 8
        blo = [max(s // 5, 1) if s > 4 else 0 for s in S]
        bhi = [b + 3 for b in blo]
        blo[ax], bhi[ax] = a0, a0 + max((7 * n) // 10, 1)
        if ax:                                             # the y column a third of X off the beam, the z column a third of Y
            blo[ax - 1] += S[ax - 1] // 3
            bhi[ax - 1] += S[ax - 1] // 3
        _put(lab, blo, bhi)
    # random boxes, sides between a tenth and a quarter of the volume's
    for _ in range(6):
        d = [int(rng.integers(max(2, s // 10), max(3, s // 4) + 1)) for s in S]
        p = [int(rng.integers(-d[k] // 2, S[k])) for k in range(3)]
        _put(lab, p, [a + b for a, b in zip(p, d)])
    # a box through each face: at least three voxels wide and two deep, so that it has interior voxels on the face
    for ax in range(3):
        for end in (0, 1):
            d = [max(3, s // 6) for s in S]
            p = [int(rng.integers(0, max(S[k] - d[k], 0) + 1)) for k in range(3)]
            p[ax] = -1 if end == 0 else S[ax] - d[ax] + 1
            _put(lab, p, [a + b for a, b in zip(p, d)])
    if fill > 0:
        ax = int(np.argmax(S))
        hi = [X, Y, Z]
        hi[ax] = max(int(fill * S[ax]), 1)
        _put(lab, (0, 0, 0), hi)
    # a volume that is one thin line (cross-section of four voxels at most): every box spans the cross-section and together they
    # would fill the line, so two aisles across it are kept free (outside the beam and the core)
    ax = int(np.argmax(S))
    if X * Y * Z // S[ax] <= 4:
        n = S[ax]
        for a, b in ((0.02, 0.10), (0.88, 0.96))[1 if fill > 0 else 0:]:      # (the low end is the block's)
            alo, ahi = [0, 0, 0], [X, Y, Z]
            alo[ax], ahi[ax] = int(a * n), max(int(b * n), int(a * n) + 1)
            _put(lab, alo, ahi, 1)
    # cubes of side 3 standing free (one interior voxel each), then never-seen blocks of side 3 standing free (their shells are
    # frontier clusters of more than a few voxels at either connectivity); on an axis shorter than 5 they span the axis
    for count, value in ((8, OCCUPIED), (3, 0)):
        placed = 0
        for _ in range(200):
            p = [int(rng.integers(1, s - 3)) if s >= 5 else 0 for s in S]
            q = [a + 3 if s >= 5 else s for a, s in zip(p, S)]
            g0 = [a - 1 if s >= 5 else 0 for a, s in zip(p, S)]
            g1 = [b + 1 if s >= 5 else s for b, s in zip(q, S)]
            if (lab[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]] == 1).all():
                _put(lab, p, q, value)
                placed += 1
                if placed == count:
                    break
    # never-seen voxels, in free space only
    free = lab == 1
    unk = np.zeros(lab.shape, bool)
    ax = int(np.argmax(S))
    t = max(min(4, S[ax] // 8), 1)
    sl = [slice(None)] * 3
    sl[2 - ax] = slice(S[ax] - t, None)
    unk[tuple(sl)] = True
    n = X * Y * Z
    where = np.flatnonzero(free & ~unk)
    if len(where):
        unk.reshape(-1)[rng.choice(where, size=min(max(n // 400, 4), len(where)), replace=False)] = True
    lab[unk & free] = 0
    return lab


def interior(occ):
    """occupied voxels without an in-volume non-occupied face neighbour (out of the volume counts as occupied)"""
    inner = occ.copy()
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(1, None), slice(None, -1)
        inner[tuple(a)] &= occ[tuple(b)]
        inner[tuple(b)] &= occ[tuple(a)]
    return inner


def longest_x_run(occ):
    """length of the longest run of True along x"""
    Z, Y, X = occ.shape
    ar = np.arange(X, dtype=np.int32)
    best = 0
    for z in range(Z):                                     # plane by plane: no second volume of int32
        last_free = np.maximum.accumulate(np.where(occ[z], np.int32(-1), ar), axis=1)
        best = max(best, int((ar - last_free).max()))
    return best


def scene_properties(vtype, ids):
    """what the tests assert of a scene, measured on committed types [Z][Y][X] and inside_dist_sq"""
    occ = np.asarray(vtype) == OCCUPIED
    inn = interior(occ)
    Z, Y, X = occ.shape
    p = {"deepest": int(ids.max()), "x_run": longest_x_run(occ), "unknown": int((np.asarray(vtype) == 0).sum()),
         "interior": int(inn.sum())}
    for name, ax, n in (("y", 1, Y), ("z", 0, Z)):
        p[name + "_line_mostly_occupied"] = bool((occ.sum(axis=ax) > n / 2).any())
        p[name + "_line_single_interior"] = bool((inn.sum(axis=ax) == 1).any())
    p["faces_cut"] = [bool(inn.take(i, axis=ax).any()) for ax in (2, 1, 0) for i in (0, -1)]
    return p


def assert_scene(size, vtype, ids, fenced=False):
    """the requirements of a solid scene; what a shape cannot hold is not asked of it, and why is said here:
      * depth: deep_target(size)² (no side above 2: only that an interior voxel exists, or the all-occupied -1 of 1 x 1 x 1);
      * x runs above 128 voxels when X >= 192;
      * along y and along z, a line more than half occupied and a line with exactly one interior voxel.  The second comes from cubes
        of side 3 that stand free, so it is asked where they can: not along an axis of length 2 or across one (the cube spans such
        an axis and both of its voxels there are interior), and not where the axis is the volume's only line of more than one voxel
        (1 x 1 x 40: the line that is mostly occupied cannot be the line with one interior voxel);
      * interior voxels on all six faces (boxes cut by the face; out of the volume counts as occupied, so their voxels on the face
        are interior) when every side is at least 3;
      * never-seen voxels when a side is above 2."""
    X, Y, Z = size
    p = scene_properties(vtype, ids)
    if max(size) > 2:
        assert p["deepest"] >= deep_target(size) ** 2, p
        assert p["unknown"] > 0, p
    elif X * Y * Z > 1:
        assert p["deepest"] > 1, p
    else:
        assert p["deepest"] == -1 and p["interior"] == 1, p
    if X >= 192:
        assert p["x_run"] > 128, p
    for name, n, others in (("y", Y, (X, Z)), ("z", Z, (X, Y))):
        assert p[name + "_line_mostly_occupied"], (name, p)
        if not fenced and n != 2 and 2 not in others and not (n > 1 and others[0] * others[1] == 1):
            assert p[name + "_line_single_interior"], (name, p)
    if min(size) >= 3:
        assert all(p["faces_cut"]), p
    return p


# ---- a volume occupied everywhere but one voxel: the largest inside distances a shape can hold, in closed form
def hole_positions(size):
    """(x, y, z) of the free voxel: the corner at the origin, the opposite corner, the middle of the low z face"""
    X, Y, Z = size
    return [(0, 0, 0), (X - 1, Y - 1, Z - 1), (X // 2, Y // 2, 0)]


def hole_labels(size, hole):
    X, Y, Z = size
    lab = np.full((Z, Y, X), OCCUPIED, np.int8)
    lab[hole[2], hole[1], hole[0]] = 1
    return lab


def hole_inside_dist_sq(size, hole):
    """(x - x0)² + (y - y0)² + (z - z0)², int32 [Z][Y][X]"""
    X, Y, Z = size
    dx = (np.arange(X, dtype=np.int32) - hole[0]) ** 2
    dy = (np.arange(Y, dtype=np.int32) - hole[1]) ** 2
    dz = (np.arange(Z, dtype=np.int32) - hole[2]) ** 2
    return dz[:, None, None] + dy[None, :, None] + dx[None, None, :]


def complement_inside_dist_sq(vtype, edt_mt, nthreads=16):
    """inside_dist_sq by the project's CPU EDT (oracle/edt_mt.c through oracle_py.edt_mt) run on the complement of the obstacles:
    the reference of the volumes scipy is too slow for"""
    from oracle_py import EDT_MT_NONE
    occ = np.asarray(vtype) == OCCUPIED
    d, _ = edt_mt(np.where(occ, 1, 2).astype(np.int8), nthreads=nthreads, want_coc=False)
    return np.where(occ, np.where(d >= EDT_MT_NONE, -1, d), 0).astype(np.int32)


def query_points(rng, pvt, size, w, n):
    """n world points like the queries of a planner gone astray: uniform over the volume +- 3 voxels (some outside); a tenth exactly
    on a face u = 0 or u = S - 1 of an axis; every flat axis (S = 1) uniform in [-0.7, 0.7) with some exactly on u = -0.5 and
    u = 0.5, the ends of its half-open interval"""
    pvt = np.array(pvt, np.float32)
    S = np.array(size, np.float32)
    u = rng.uniform(-3, S + 2, size=(n, 3)).astype(np.float32)
    flat = S == 1
    if flat.any():
        u[:, flat] = rng.uniform(-0.7, 0.7, size=(n, int(flat.sum())))
    face = rng.random(n) < 0.1
    ax = rng.integers(0, 3, n)
    on = np.where(rng.random(n) < 0.5, 0.0, S[ax] - 1)
    on = np.where(flat[ax], np.where(rng.random(n) < 0.5, -0.5, 0.5), on)
    u[face, ax[face]] = on[face]
    tight = rng.random(n) < 0.5                            # half of the points keep the other axes inside, so that faces decide
    inside = rng.uniform(0, np.maximum(S - 1, 0), size=(n, 3)).astype(np.float32)
    for k in range(3):
        if not flat[k]:
            sel = tight & ~(face & (ax == k))
            u[sel, k] = inside[sel, k]
    return ((u + pvt) * np.float32(w)).astype(np.float32)

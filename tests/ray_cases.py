"""Hand-made clouds for the segmented ray caster (k_free_rays, csrc/gie_kernels.hip.h), shared by the CPU (oracle, emulation,
plain statement) and GPU (HIP) halves of tests/test_ray_cast_edges.py.

The kernel cuts every ray's walk into 8 time intervals of the ray's stay in the volume (one wave each), replays the walk's
state per axis (gie_dda_skip_to), finds the stop as a minimum over the segments and merges the decrements of neighbouring lanes
(gie_wave_add).  Whole scenes with the sensor in the middle of the volume do not place a ray on any of these mechanisms on
purpose; the families below do:

  axis        points exactly on +-x, +-y, +-z and in the coordinate planes (step == 0, tMax = FLT_MAX), 1 cell to 700 cells long,
              from a cell centre and from a sensor offset by binary fractions of the voxel width (w = 0.125: exact in float32)
  ties        the 2-D and 3-D diagonals from a cell-centre sensor at w = 0.125: equal tMax at every step, and (lengths of
              4, 12, 20, ... cells) border crossings that fall exactly on a segment's limit
  stops       a blocker point on the way of a long ray, in every eighth of its walk
  ends        every way a walk ends: cur == i1, far > len, far > max_length (2x, 10x, 500x), own cell, one step, points outside
              the height band (not registered, their ray is still cast)
  aggregation runs of 2 .. 200 copies of one point with NaN points and other directions in between, a fan of 512 rays within
              0.5 degrees; also as clouds of 1, 63, 64 and 65 points
  outside     the mapper is one tile of a larger volume (set_tile) and the sensor stands 10 to 20 voxels beyond a face, an edge
              or a corner of it, or 1 to 3 voxels beside it (rays parallel to a face, inside and outside the box the kernel
              clips to); also far from the origin and under a rolled and pitched pose

A case is a dict: name, family, size, voxel, tile ((off, whole) or None), pose, quat, points (float32, sensor frame), min_h,
max_h, exact (identity rotation, near the origin: the plain statement applies), subset (indices of the points the statement is
given: a Python loop; 600 rays, up to 640 where the special rays alone are more) and require(stats): a predicate on the statement's result for the subset,
stats = dict(rays=<records of raycast_ref>, count=<ray counts>, sensor=<local cell of the sensor>).  Every require must hold on
the statement alone (tests/test_ray_cast_edges.py asserts it without a GPU).

The maximum length of a walk is 0.707 * X * w with X the mapper's OWN x size, a tile's too: 45 voxels in (64, 48, 24), 11 in
(16, 200, 8).  So no ray crosses the 16 voxels of the thin tile along x, from wherever it starts; the rays that cross it
entirely do so along z (sensor 2 voxels beyond the -z face) and past its x / z edge (sensor 2 voxels beyond the -x face and 1
above the +z face), those of the large tile along z.  Every outside case, the thin ones included, asks the same of the statement's
subset: 200 rays that enter after their first step, 50 that never enter, 50 that leave before their end."""
import math

import numpy as np

IDENT = (1.0, 0.0, 0.0, 0.0)
BIG, THIN = (64, 48, 24), (16, 200, 8)
FAR = np.array([-1234.56, 789.01, -3.3])          # tests/edge_inputs.py: far from the origin, negative coordinates
UPDATES = 3
MOVE_VOX = 3                                       # the pose moves this many voxels in x per update
STATEMENT_RAYS = 600


def max_length(size, w):
    return 0.707 * size[0] * w


def poses(case):
    """The pose of every update: MOVE_VOX voxels further in x each time (float32 values)."""
    return [tuple(np.float32(case["pose"][i] + (k * MOVE_VOX * case["voxel"] if i == 0 else 0.0)) for i in range(3)) for k in range(UPDATES)]


def pivot(case, pos):
    w = np.float32(case["voxel"])
    off = case["tile"][0] if case["tile"] else (0, 0, 0)
    return [int(np.floor(np.float32(np.float32(pos[i]) / w) + np.float32(0.5))) - case["size"][i] // 2 + int(off[i]) for i in range(3)]


def _case(name, family, size, w, points, pose, band, require, tile=None, quat=IDENT, exact=True, special=None):
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    keep = np.zeros(n, bool) if special is None else np.asarray(special, bool).copy()
    rest = np.flatnonzero(~keep)
    room = max(STATEMENT_RAYS - int(keep.sum()), 50)
    if len(rest) > room:                             # every k-th of the ordinary points, all the special ones
        rest = rest[::int(math.ceil(len(rest) / room))]
    keep[rest] = True
    return dict(name=name, family=family, size=size, voxel=w, tile=tile, pose=tuple(float(v) for v in pose), quat=quat, points=points,
                min_h=float(np.float32(band[0])), max_h=float(np.float32(band[1])), require=require, exact=exact, subset=np.flatnonzero(keep))


def _count(stats, **want):
    return sum(1 for r in stats["rays"] if all(r[k] == v for k, v in want.items()))


def _signs(n):
    return [tuple(1 if (m >> i) & 1 else -1 for i in range(n)) for m in range(1 << n)]


# ------------------------------------------------------------------ axis rays
# lengths in cells; 4, 12, 20, ... put a border crossing exactly on a segment's limit ((j + 1/2) w = k / 8 of the length)
AXIS_CELLS = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 20, 23, 24, 25, 28, 31, 32, 33, 36, 44, 45, 46, 47, 60, 100, 700)


def _axis_points(w):
    pts = []
    for a in range(3):
        for s in (1, -1):
            for k in AXIS_CELLS:
                p = [0.0, 0.0, 0.0]; p[a] = s * k * w
                pts.append(p)
    for a, b in ((3, 7), (10, 4), (13, 29), (40, 11), (2, 50), (1, 1), (20, 6)):       # in the three coordinate planes
        for i, j in ((0, 1), (0, 2), (1, 2)):
            for si, sj in _signs(2):
                p = [0.0, 0.0, 0.0]; p[i] = si * a * w; p[j] = sj * b * w
                pts.append(p)
    return np.array(pts)


def _axis_require(size, w):
    long_walk = int(0.9 * max_length(size, w) / w)
    def require(st):
        r = st["rays"]
        return (_count(st, stop="end") >= 40 and _count(st, stop="max_length") >= 12 and _count(st, stop="occupied") >= 3
                and _count(st, steps=1) >= 6 and max(x["steps"] for x in r) >= long_walk
                and sum(1 for x in r if 0 <= x["last_in"] < x["steps"] - 1) >= 10)          # leaves the volume before the walk ends
    return require


def axis_cases():
    out = []
    # the band keeps the plane z = 0 unregistered (a registered point stops every longer ray of its axis); +z points of 2 to 5
    # cells are registered and stop the +z axis
    for name, size, w, pose in (("axis_centre_big", BIG, 0.1, (0.0, 0.0, 0.0)), ("axis_centre_thin", THIN, 0.1, (0.0, 0.0, 0.0)),
                                ("axis_centre_w125", BIG, 0.125, (0.0, 0.0, 0.0)),
                                ("axis_offset_big", BIG, 0.125, (0.03125, -0.046875, 0.015625)),
                                ("axis_offset_thin", THIN, 0.125, (-0.0546875, 0.0078125, 0.03125))):
        out.append(_case(name, "axis", size, w, _axis_points(w), pose, (0.15, 0.5), _axis_require(size, w)))
    return out


# ------------------------------------------------------------------ ties
def _tie_points(w):
    pts = []
    for k in (1, 2, 3, 4, 5, 8, 12, 13, 20, 21, 28, 30, 34, 36, 40, 60):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            for si, sj in _signs(2):
                p = [0.0, 0.0, 0.0]; p[i] = si * k * w; p[j] = sj * k * w
                pts.append(p)
        for s in _signs(3):
            pts.append([s[0] * k * w, s[1] * k * w, s[2] * k * w])
    return np.array(pts)


def _tie_require(st):
    return sum(r["ties"] for r in st["rays"]) >= 100 and max(r["steps"] for r in st["rays"]) >= 60


def tie_cases():
    w = 0.125                                        # the band registers z = 3 cells only: most diagonals run their whole length
    return [_case("ties", "ties", BIG, w, _tie_points(w), (0.0, 0.0, 0.0), (0.3, 0.45), _tie_require),
            _case("ties_thin", "ties", THIN, w, _tie_points(w), (0.0, 0.0, 0.0), (0.3, 0.45),
                  lambda st: sum(r["ties"] for r in st["rays"]) >= 100)]


# ------------------------------------------------------------------ stops per segment
def _stop_points(length, spread_about, n_frac, seed):
    """For each of the 8 eighths and n_frac places inside it, one direction of its own: a long point at `length` and a blocker
    point at that share of it (registered before any ray is cast, so the long ray stops there)."""
    rng = np.random.default_rng(seed)
    pts, k = [], 0
    fr = np.concatenate([[0.03, 0.97], np.linspace(0.1, 0.9, n_frac - 2)])
    n = 8 * len(fr)
    for s in range(8):
        for f in fr:
            if spread_about is None:
                az = (k + 0.37) * 2.0 * math.pi / n
            else:                                    # two bundles, about +spread and about spread + pi (a thin volume's long side)
                az = spread_about + (k % 2) * math.pi + ((k // 2) - n / 4.0) * (1.2 / n)
            el = rng.uniform(-0.08, 0.08)
            u = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
            pts.append(u * length)
            pts.append(u * length * (s + f) / 8.0)
            k += 1
    return np.array(pts)


def _stop_require(st):
    stopped = [r for r in st["rays"] if r["stop"] == "occupied"]
    return ({r["seg"] for r in stopped} == set(range(8))
            and sum(1 for r in stopped if r["seg_prev"] != r["seg"]) >= 8         # the stop is the first step of its segment
            and sum(1 for r in stopped if r["seg_next"] != r["seg"]) >= 8         # ... the last one
            and _count(st, stop="occupied", steps=1) >= 1)


def stop_cases():
    big = np.vstack([_stop_points(3.0, None, 18, 5), [[0.1, 0.0, 0.0], [0.0, -0.1, 0.0]]])     # two stops at the first step of all
    thin = np.vstack([_stop_points(1.0, math.pi / 2, 14, 6), [[0.1, 0.0, 0.0], [0.0, -0.1, 0.0]]])
    return [_case("stops_big", "stops", BIG, 0.1, big, (0.237, -0.118, 0.041), (-0.45, 0.5), _stop_require),
            _case("stops_thin", "stops", THIN, 0.1, thin, (0.237, -0.118, 0.041), (-0.25, 0.3), _stop_require)]


# ------------------------------------------------------------------ ends
def _end_points(size, w, band, seed, pose=(0.23, -0.11, 0.031)):
    rng = np.random.default_rng(seed)
    half = np.array(size) * w / 2.0
    ml = max_length(size, w)
    box = lambda n, zlo, zhi: np.stack([rng.uniform(-half[0], half[0], n), rng.uniform(-half[1], half[1], n), rng.uniform(zlo, zhi, n)], -1)
    reach = min(half[2], ml)
    inband = box(400, band[0] + 0.02, band[1] - 0.02)              # registered; far out, so that they stop few other rays
    inband = inband[np.linalg.norm(inband[:, :2], axis=1) > 0.6 * min(half[0], ml)][:40]
    above = box(150, band[1] + 0.03, reach)                       # not registered, their ray is still cast
    below = box(80, -reach, band[0] - 0.03)
    v = rng.standard_normal((24, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    far = np.concatenate([v[:8] * 2 * ml, v[8:16] * 10 * ml, v[16:] * 500 * ml])
    own = [[0.01, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0e6, 0.0, 0.0], [0.3, -1.5e6, band[0] + 0.05]]     # own cell; beyond +-1e6 m: ignored
    nb = [[w, 0, 0], [-w, 0, 0], [0, w, 0], [0, -w, 0], [0, 0, w], [0, 0, -w]]       # one-step rays; below the band: not registered
    edge = box(80, -reach, band[0] - 0.03)                         # on cell borders in x and y: the walk and pos2coord may part (far > len)
    edge[:, :2] = (np.floor(edge[:, :2] / w) + 0.5) * w - np.array(pose[:2])
    return np.concatenate([inband, above, below, edge, far, own, nb])


def _end_require(st):
    return (_count(st, stop="end") >= 30 and _count(st, stop="len") >= 1 and _count(st, stop="max_length") >= 20
            and _count(st, stop="occupied") >= 10 and _count(st, stop="own_cell") >= 2 and _count(st, stop="unusable") >= 2 and _count(st, steps=1) >= 6)


def end_cases():
    return [_case("ends_big", "ends", BIG, 0.1, _end_points(BIG, 0.1, (0.15, 0.5), 7), (0.23, -0.11, 0.031), (0.15, 0.5), _end_require),
            _case("ends_thin", "ends", THIN, 0.1, _end_points(THIN, 0.1, (0.15, 0.3), 8), (0.23, -0.11, 0.031), (0.15, 0.3), _end_require)]


# ------------------------------------------------------------------ aggregation
def _aggregation_cloud():
    nan = [np.nan, np.nan, np.nan]
    p = [1.52, 0.41, 0.13]
    rng = np.random.default_rng(9)
    other = lambda: list(rng.uniform(-1.5, 1.5, 3) * [1.0, 1.0, 0.2])
    pts, special = [], []
    def add(rows, sp):
        pts.extend(rows); special.extend([sp] * len(rows))
    add([p] * 64, True); add([other()], True); add([p] * 65, True); add([nan], True); add([p] * 200, True)
    for k in range(2, 64):                           # runs of 2 .. 63 copies, each in a direction of its own
        az = 0.4 + 0.09 * k
        q = [2.1 * math.cos(az), 2.1 * math.sin(az), 0.07 * math.sin(3.0 * k)]
        add([nan] if k % 2 == 0 else [other()], k <= 14)
        add([q] * k, k <= 14)
    az = math.radians(200.0) + math.radians(0.5) * np.arange(512) / 512.0
    fan = np.stack([3.0 * np.cos(az), 3.0 * np.sin(az), np.full(512, -0.21)], -1)
    add([list(v) for v in fan], False)
    while len(pts) % 64 != 1:                        # 64 k + 1 points: the last workgroup holds one ray
        add([other()], False)
    return np.array(pts, np.float32), np.array(special, bool)


def _aggregation_require(st):
    c = st["count"].copy()
    z, y, x = st["sensor"][2], st["sensor"][1], st["sensor"][0]
    c[z, y, x] = 0                                   # (every ray clears the sensor's own cell: that one proves nothing)
    return c.min() <= -200 and c.max() >= 64


def aggregation_cases():
    pts, special = _aggregation_cloud()
    assert len(pts) % 64 == 1
    pose, band = (0.237, -0.118, 0.041), (-0.45, 0.5)
    out = [_case("aggregation", "aggregation", BIG, 0.1, pts, pose, band, _aggregation_require, special=special)]
    tail = pts[129:]                                 # a cloud of n points: the end of the second run, the NaN point, the 200 copies
    for n in (1, 63, 64, 65):
        out.append(_case("aggregation_%d" % n, "aggregation", BIG, 0.1, tail[:n], pose, band,
                         lambda st, n=n: st["count"].max() == n - (n > 1)))       # every finite point is a copy of one point
    return out


# ------------------------------------------------------------------ outside sensor (tiled)
def _tile_off(size, beyond):
    """Offsets that put the sensor's cell `beyond[i]` voxels beyond the tile's low face (> 0) or high face (< 0) on axis i;
    0: the tile stays centred on the sensor on that axis."""
    off = []
    for s, b in zip(size, beyond):
        off.append(0 if b == 0 else (s // 2 + b if b > 0 else b - (s - s // 2) + 1))
    return tuple(off)


def _fib_sphere(n):
    i = np.arange(n) + 0.5
    ph, th = np.arccos(1.0 - 2.0 * i / n), math.pi * (1.0 + 5.0 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], -1)


def _outside_cloud(size, w, off, pose, n_sphere, seed):
    """Points in the MAP frame relative to the sensor (the caller turns them into the sensor frame), and which are special."""
    rng = np.random.default_rng(seed)
    ml = max_length(size, w)
    c = np.floor(np.array(pose) / w + 0.5)
    lo = (c - np.array(size) // 2 + np.array(off) - 0.5) * w - np.array(pose)      # the tile's faces, relative to the sensor
    hi = lo + np.array(size) * w
    mid = (lo + hi) / 2.0
    parts, special = [], []
    def add(p, every):                               # every k-th ray of the group goes to the statement
        p = np.asarray(p, np.float64).reshape(-1, 3); parts.append(p)
        m = np.zeros(len(p), bool); m[::every] = True; special.append(m)
    add(_fib_sphere(n_sphere) * np.resize([0.25, 0.55, 0.9, 1.3], n_sphere)[:, None] * ml, 16)
    towards = mid / np.linalg.norm(mid)                                            # a cone of rays towards the tile, of every length
    v = towards + 0.45 * rng.standard_normal((n_sphere // 2, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    add(v * rng.uniform(0.1, 1.4, (len(v), 1)) * ml, 16)
    grid = np.linspace(-0.1, 1.1, 5)
    faces = []
    for a in range(3):                                                             # along the faces: targets on, and within a cell of, each face plane
        i, j = [k for k in range(3) if k != a]
        for plane in (lo[a], hi[a]):
            for dlt in (-1.0, -0.5, 0.0, 0.5, 1.0):
                for u in grid:
                    for t in grid:
                        q = np.zeros(3); q[a] = plane + dlt * w
                        q[i] = lo[i] + u * (hi[i] - lo[i]); q[j] = lo[j] + t * (hi[j] - lo[j])
                        faces.append(q)
    add(faces, 8)
    corners = np.array([[(lo, hi)[(m >> k) & 1][k] for k in range(3)] for m in range(8)])
    edges = []
    for m in range(8):
        for k in range(3):
            if not (m >> k) & 1:
                for f in (0.25, 0.5, 0.75):
                    edges.append(corners[m] + f * (corners[m | (1 << k)] - corners[m]))
    through = np.vstack([corners, edges])
    add(through, 1); add(through * 1.5, 1)                                   # to the edges and corners, and through them
    near = np.linalg.norm(np.clip(0.0, lo, hi))                                    # distance to the tile
    add(v[:120] * near * rng.uniform(0.2, 0.95, (120, 1)), 3)                  # end before reaching the tile
    rlo, rhi = np.maximum(lo, -ml), np.minimum(hi, ml)                             # the part of the tile within reach
    if (rlo < rhi).all():
        add(rlo + rng.uniform(0.0, 1.0, (300, 3)) * (rhi - rlo), 4)                # end inside the tile
    tgt = []                                                                       # through the tile and out of it: aimed at a place
    blo, bhi = np.maximum(lo, -0.9 * ml), np.minimum(hi, 0.9 * ml)                 # where the ray leaves the tile within 0.9 of the maximum length
    for _ in range(40000 if (blo < bhi).all() else 0):
        a, side = int(rng.integers(3)), int(rng.integers(2))
        t = blo + rng.uniform(0.0, 1.0, 3) * (bhi - blo)
        t[a] = (lo, hi)[side][a]
        if (t[a] > 0.0) == bool(side) and np.linalg.norm(t) <= 0.9 * ml:
            tgt.append(t / np.linalg.norm(t) * 1.4 * ml)
            if len(tgt) == 450:
                break
    if tgt:
        add(tgt, 3)        # through the tile and out of it (or up to the maximum length)
    ax = []
    for a in range(3):                                                             # parallel to the faces: step == 0 on two axes
        for s in (1, -1):
            for r in (0.3, 0.8, 1.2, 5.0):
                p = np.zeros(3); p[a] = s * r * ml
                ax.append(p)
    add(ax, 1)
    return np.vstack(parts), np.concatenate(special)


def _outside_require(st):
    r = st["rays"]
    return (sum(1 for x in r if x["first_in"] > 0) >= 200 and sum(1 for x in r if x["steps"] > 0 and x["first_in"] < 0) >= 50
            and sum(1 for x in r if 0 <= x["last_in"] < x["steps"] - 1) >= 50)


def rot_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _outside(name, size, beyond, n_sphere=1000, pose=(0.237, -0.118, 0.041), shift=None, quat=IDENT, require=_outside_require, seed=21,
             family="outside", twin=None):
    w = 0.1
    off = _tile_off(size, beyond)
    whole = tuple(2 * (abs(o) + s) for o, s in zip(off, size))
    pts, special = _outside_cloud(size, w, off, pose, n_sphere, seed)
    band = (-0.45, 0.5) if size == BIG else (-0.25, 0.3)
    band = (band[0] + off[2] * w, band[1] + off[2] * w)                            # around the tile's middle height
    if quat != IDENT:
        pts = pts @ rot_from_quat(quat)                                            # R^T p: the sensor frame
    if shift is not None:
        pose = tuple(np.array(pose) + shift)
        band = (band[0] + shift[2], band[1] + shift[2])
    case = _case(name, family, size, w, pts, pose, band, require, tile=(off, whole), quat=quat, exact=(shift is None and quat == IDENT), special=special)
    if twin is not None:
        case["twin"] = twin
    return case


def outside_cases():
    out = [_outside("outside_-x", BIG, (15, 0, 0)), _outside("outside_+x", BIG, (-12, 3, 0)), _outside("outside_-y", BIG, (0, 10, -2)),
           _outside("outside_+y", BIG, (4, -17, 0)), _outside("outside_-z", BIG, (0, 0, 13)), _outside("outside_+z", BIG, (-5, 0, -20)),
           _outside("outside_edge", BIG, (14, 11, 0)), _outside("outside_corner", BIG, (10, -10, 10)),
           _outside("outside_thin_-z", THIN, (0, 0, 2)), _outside("outside_thin_-x", THIN, (10, 0, 0)), _outside("outside_thin_edge", THIN, (2, 0, -1))]
    # 1 to 3 voxels beside the -y face and 12 beyond the -x face: the rays along x lie inside the grown box (1), outside it by
    # less than a cell (2) and by more (3)
    out += [_outside("beside_%d" % d, BIG, (12, d, 0), n_sphere=500, seed=30 + d) for d in (1, 2, 3)]
    return out


def far_cases():
    """Far from the origin (the pose shifted as tests/edge_inputs.py does) and tilted: against the oracle only.  Each names its
    `twin`: the exact case with the same cloud in the map frame (same tile, same seed), whose precondition stands for both."""
    w = 0.125
    c = tie_cases()[0]
    # a cell centre again: the shift rounded to whole voxels
    shift = np.round(FAR / w) * w
    ties_far = dict(c, name="ties_far", family="far", pose=tuple(shift), min_h=float(np.float32(c["min_h"] + shift[2])),
                    max_h=float(np.float32(c["max_h"] + shift[2])), exact=False, twin="ties")
    roll, pitch = 0.5, 0.35
    q = _qmul((math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0), (math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0))
    q = tuple(float(np.float32(v)) for v in q)
    return [ties_far,
            _outside("outside_far", BIG, (15, 0, 0), shift=FAR, family="far", twin="outside_-x"),
            _outside("outside_corner_far", BIG, (10, -10, 10), shift=FAR, family="far", twin="outside_corner"),
            _outside("outside_tilted", BIG, (15, 0, 0), quat=q, family="tilted", twin="outside_-x")]


def _qmul(a, b):
    """Hamilton product, (w, x, y, z)."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def all_cases():
    return axis_cases() + tie_cases() + stop_cases() + end_cases() + aggregation_cases() + outside_cases() + far_cases()


CASES = all_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

"""Tilted poses and odd sensor geometry for the three projective classifiers (depth camera, multi-ring lidar, 2-D scan), shared by
the CPU (emulation) and GPU (HIP) suites: a sensor whose z axis is NOT the map's z axis (roll and pitch up to upside down and on
its side), lidars with a negative ring increment, a one-sided field of view, bins that wrap through the modulo, one ring, rings
up to +-88 degrees; cameras with fx != fy, a principal point off centre and outside the image, one pixel; scans of 77 and 1081
bins; volumes that cross every edge of the z-column kernel (partial 64-lane row, partial group of 4 in y, partial column of 8 in z,
exactly one workgroup, Z = 1, X = 3).

run() drives one case through a reference mapper (the oracle) and a mapper under test and asserts, update by update: equal scan
labels and ray counts, everything edge_inputs._compare checks after fuse / batch EDT / merge, and the test mapper's labels against
the float64 statement of that sensor (tests/ogm_f64.py), which shares no arithmetic with either.

op_classify_multiscan (gie_functors.h) is why the tilts matter: tile_skip drops a z-column of 8 voxels on its two end voxels by a
convexity argument that an upright sensor never puts to work (hor is constant along the column, lz monotone), and the guard
tan_hi >= 0 && tan_lo <= 0 decides only for a one-sided field of view on a sensor rolled by about 90 degrees."""
import math

import numpy as np

import edge_inputs
import gie
from gie import scenes
from ogm_f64 import _compare as compare_f64
from ogm_f64 import _depth_f64, _g2l, _multiscan_f64, _scan2d_f64, _voxel_positions

# (roll, pitch) in rad; the quaternion is yaw * roll * pitch, the yaw turning 31 degrees per update
TILTS = ((0.0, 0.0), (0.3, 0.0), (0.0, -0.4), (0.5, 0.35), (-1.2, 0.9), (3.0, 0.2), (1.5, 0.0), (-1.6, 0.1))
STRONG = ((-1.6, 0.1), (-1.2, 0.9), (3.0, 0.2))      # on its side, tumbling, upside down: the subset the small volumes get
YAW_DEG = 31.0
DELTA_VOX = 4
# where the drive starts: off the origin, every coordinate negative, no multiple of a voxel width (an upright sensor on a voxel
# centre puts whole planes of voxels exactly on a pixel edge or on the 2-D scan's slab face: ties, which pin nothing)
BASE = np.array([-2.73, -1.88, -0.63])

MAIN_VOLUME = (70, 45, 19)                           # partial 64-lane row in x, partial group of 4 in y, partial column of 8 in z
SMALL_VOLUMES = ((64, 4, 8), (65, 5, 9), (40, 40, 1), (3, 50, 33))

# rings, bins, phi_min (deg), phi_inc (deg), theta_min
MULTISCAN = {
    "a": (16, 440, -15.0, 2.0, -math.pi),
    "b": (16, 440, 15.0, -2.0, -math.pi),            # negative increment
    "c": (8, 360, 20.0, 3.0, -math.pi + 0.3),        # upward only: tan_lo > 0
    "d": (8, 360, -41.0, 3.0, -math.pi),             # downward only: tan_hi < 0
    "e": (8, 100, -30.0, 3.0, 0.7),                  # bins wrap through the modulo
    "f": (1, 77, 0.0, 1.0, -math.pi),
    "g": (64, 512, -60.0, 2.0, -math.pi),
    "h": (32, 900, -88.0, 5.6, -math.pi),            # fov_test == 0: no early-out at all
    "i": (4, 33, -3.0, 2.0, 2.0),
}
# rows, cols, cx, cy, fx, fy
DEPTH = {
    "60x80": (60, 80, 39.5, 29.5, 70.0, 70.0),
    "37x53": (37, 53, 20.0, 30.0, 45.0, 80.0),
    "1x1": (1, 1, 0.0, 0.0, 5.0, 5.0),
    "48x64_outside": (48, 64, -10.0, 60.0, 60.0, 60.0),      # the principal point lies outside the image
}
# bins, theta_min
SCAN2D = {
    "360": (360, -math.pi + math.pi / 360),
    "77": (77, 0.4),
    "1081": (1081, -2.356),
}
# FREE / OCCUPIED labels of the float64 statement, summed over the eight tilts in the main volume, that every set must reach: what
# the restatement tests of tests/test_independent_checks.py ask of their three frames
FLOORS = {"multiscan": (1000, 50), "depth": (1000, 50), "scan2d": (1000, 30)}
# ... and over the three tilts in a small volume: the same share of the voxel-updates for FREE (1000 of 8 x 59 850 voxel-updates;
# 31 of the 3 x 4 950 of the largest small volume, 10 of the 3 x 1 600 of the smallest); for OCCUPIED that share is below two
# voxels everywhere, so the floor is 3: more than a stray voxel or two
def small_floors(size):
    n = size[0] * size[1] * size[2]
    return int(math.ceil(FLOORS["multiscan"][0] * 3.0 * n / (8.0 * MAIN_VOLUME[0] * MAIN_VOLUME[1] * MAIN_VOLUME[2]))), 3


# the one (set, volume) pair left out: a single ring 1 degree wide meets the single layer of voxels of a Z = 1 volume in a line, and
# a voxel centre 2 cm off that line lies outside the ring nearer than 2.3 m: further than this volume reaches.  Nothing but chance
# would put an OCCUPIED voxel there
LEFT_OUT = {("multiscan", "f", (40, 40, 1))}
# what makes a small volume see something: the sensor's view axis (the ray through the middle of its image or of its rings) is
# turned to this heading (degrees; along the volume's long side) whatever the tilt, and a pillar stands in that direction, through
# the volume's whole height, in front of its far face
AIM = {(64, 4, 8): 0.0, (65, 5, 9): 0.0, (40, 40, 1): 0.0, (3, 50, 33): 90.0}
PILLARS = {0.0: ((18, -4, -40), (24, 4, 40)), 90.0: ((-4, 18, -40), (12, 24, 40))}       # (lo, hi) in voxels from where the drive starts
AIM_STEP_DEG = 4.0                                   # the heading moves on by this much per update
SETS = {"multiscan": MULTISCAN, "depth": DEPTH, "scan2d": SCAN2D}


def f32(v):
    return float(np.float32(v))


def qmul(a, b):
    """Hamilton product, (w, x, y, z)."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def view_axis(sensor, p):
    """The middle of what a sensor sees, in its own frame: the ray through the centre of the image / at the middle ring, bin 0."""
    if sensor == "depth":
        rows, cols, cx, cy, fx, fy = p
        return np.array([1.0, (cx - (cols - 1) / 2.0) / fx, (cy - (rows - 1) / 2.0) / fy])
    if sensor == "multiscan":
        mid = math.radians(p[2] + p[3] * (p[0] - 1) / 2.0)
        return np.array([math.cos(mid), 0.0, math.sin(mid)])
    return np.array([1.0, 0.0, 0.0])


def tilted_pose(k, w, roll, pitch, aim=None, axis=(1.0, 0.0, 0.0)):
    """Update k of a drive: DELTA_VOX voxels in x and YAW_DEG of yaw per update from BASE, rolled and pitched; float32 values.
    aim (degrees): the yaw is chosen instead so that `axis` of the sensor, rolled and pitched, heads aim + AIM_STEP_DEG * k.
    Returns (pos, q, origin): origin is the same place in the frame of the box world, which stands around BASE."""
    yaw = math.radians(YAW_DEG * k)
    if aim is not None:
        fwd = scenes.rot_from_quat(qmul((math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0), (math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0))) @ np.asarray(axis)
        yaw = math.radians(aim + AIM_STEP_DEG * k) - math.atan2(fwd[1], fwd[0])
    q = qmul(qmul((math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)), (math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0)),
             (math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0))
    q = tuple(f32(v) for v in q)
    pos = tuple(np.float32(v) for v in BASE + np.array([k * DELTA_VOX * w, 0.0, 0.0]))
    origin = np.array([float(v) for v in pos]) - BASE
    return pos, q, origin


def ring_image(world, frame, origin, q, rings, bins, phi_min, phi_inc, theta_min):
    """One ray through the centre of every (ring, bin) of a lidar: the horizontal range, +inf where nothing is hit within 30 m.
    Bin b is centred on theta_min + b * theta_inc (the classifiers take floor((theta - theta_min) / theta_inc + 0.5))."""
    ph, th = np.meshgrid(phi_min + phi_inc * np.arange(rings), theta_min + (2.0 * math.pi / bins) * np.arange(bins), indexing="ij")
    d_s = np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], axis=-1).reshape(-1, 3)
    t = world.cast(origin, d_s @ scenes.rot_from_quat(q).T, frame).reshape(rings, bins)
    return np.where(t <= 30.0, t * np.cos(ph), np.inf).astype(np.float32)


def _world(sensor, pillar=None):
    if sensor == "depth":
        world = scenes.BoxWorld(4, extent=(2.0, 2.0, 1.0), n_boxes=25, toggle_frac=0.25)
    else:
        world = scenes.BoxWorld(3, extent=(4.0, 4.0, 1.2), n_boxes=30, toggle_frac=0.25)
    if pillar is not None:                               # one more box, always present
        world.lo, world.hi = np.vstack([world.lo, [pillar[0]]]), np.vstack([world.hi, [pillar[1]]])
        world.toggles, world.phase = np.append(world.toggles, False), np.append(world.phase, 0)
    return world


def cases(sensor, name):
    """The cases of one parameter set: every tilt in the main volume, the three strongest in each small one."""
    w = 0.05 if sensor == "depth" else 0.1
    out = [dict(sensor=sensor, name=name, param=SETS[sensor][name], size=MAIN_VOLUME, voxel=w, tilts=TILTS,
                floors=FLOORS[sensor])]
    out += [dict(sensor=sensor, name=name, param=SETS[sensor][name], size=s, voxel=w, tilts=STRONG, floors=small_floors(s), aim=AIM[s])
            for s in SMALL_VOLUMES if (sensor, name, s) not in LEFT_OUT]
    return out


def planner_case():
    """Set a with for_motion_planner: the robot's sphere is FREE whatever the field of view says, so neither early-out may drop it."""
    return dict(sensor="multiscan", name="a", param=MULTISCAN["a"], size=MAIN_VOLUME, voxel=0.1, tilts=TILTS, floors=FLOORS["multiscan"],
                planner=True)


def height_gate(case):
    """(ogm_min_h, ogm_max_h): a band of the main volume's height around the drive, so that the gate decides inside the volume."""
    h = case["voxel"] * MAIN_VOLUME[2]
    return f32(BASE[2] - 0.32 * h), f32(BASE[2] + 0.37 * h)


def config(case):
    lo, hi = height_gate(case)
    return gie.make_config(case["voxel"], case["size"], cutoff_dist=1.0, ogm_min_h=lo, ogm_max_h=hi, for_motion_planner=bool(case.get("planner")))


def frames(case):
    """(pos, q, data, kw, restate) of every update of a case; restate() returns (labels, sure) of the float64 statement."""
    sensor, size, w, p = case["sensor"], case["size"], case["voxel"], case["param"]
    aim = case.get("aim")
    world = _world(case.get("world", sensor), None if aim is None else w * np.array(PILLARS[aim], np.float64))
    lo, hi = height_gate(case)
    for k, (roll, pitch) in enumerate(case["tilts"], case.get("k0", 0)):      # (k0: the drive goes on where another case's ended)
        pos, q, origin = tilted_pose(k, w, roll, pitch, aim, view_axis(sensor, p))
        if sensor == "multiscan":
            rings, bins, phi_min, phi_inc, theta_min = p[0], p[1], math.radians(p[2]), math.radians(p[3]), p[4]
            img = ring_image(world, k, origin, q, rings, bins, phi_min, phi_inc, theta_min)
            if case.get("planner"):
                img[min(3, rings - 1), bins // 9:bins // 5] = np.nan          # a NaN stretch
                img[:, bins // 2:bins // 2 + bins // 20] = 0.25               # and a stretch of ranges <= 0.3, over every ring
                img[rings // 2, 0:bins // 40] = 0.3
            kw = dict(theta_inc=2.0 * math.pi / bins, theta_min=theta_min, phi_inc=phi_inc, phi_min=phi_min)
            restate = lambda pos=pos, q=q, img=img, kw=kw: _multiscan_f64(                                   # noqa: E731
                pos, q, size, w, img, f32(kw["theta_inc"]), f32(kw["theta_min"]), f32(kw["phi_inc"]), f32(kw["phi_min"]), lo, hi)
            yield pos, q, img, kw, restate
        elif sensor == "depth":
            rows, cols, cx, cy, fx, fy = p
            dep = scenes.depth_frame(world, k, origin, q, rows=rows, cols=cols, fx=fx, fy=fy, cx=cx, cy=cy, max_depth=6.0)
            valid_nan = bool(k & 1)                                            # alternates; with the patch, all four combinations
            if k & 2:
                dep = dep.copy(); dep[rows // 4:rows // 2 + 1, cols // 3:2 * cols // 3 + 1] = np.nan
            kw = dict(cx=cx, cy=cy, fx=fx, fy=fy, valid_nan=valid_nan)
            restate = lambda pos=pos, q=q, dep=dep, valid_nan=valid_nan: _depth_f64(                         # noqa: E731
                pos, q, size, w, dep, f32(cx), f32(cy), f32(fx), f32(fy), valid_nan, lo, hi)
            yield pos, q, dep, kw, restate
        elif sensor == "scan2d":
            bins, theta_min = p
            r = ring_image(world, k, origin, q, 1, bins, 0.0, 0.0, theta_min)[0]
            r[bins // 9:bins // 9 + bins // 24 + 1] = np.nan                   # a NaN stretch
            r[5 * bins // 9:5 * bins // 9 + bins // 36 + 1] = 0.25             # a too-short stretch
            kw = dict(theta_inc=2.0 * math.pi / bins, theta_min=theta_min)
            restate = lambda pos=pos, q=q, r=r, kw=kw: _scan2d_f64(pos, q, size, w, r, f32(kw["theta_inc"]), f32(kw["theta_min"]), lo, hi)  # noqa: E731
            yield pos, q, r, kw, restate
        else:
            raise ValueError(sensor)


def feed(m, sensor, data, kw):
    {"multiscan": m.ogm_multiscan, "depth": m.ogm_depth, "scan2d": m.ogm_scan2d}[sensor](data, **kw)


def robot_sphere(cfg, size):
    """The voxels for_motion_planner declares FREE: |crd - size / 2|^2 <= robot_r2_grids (vlp16_fast.cu:30-40), [Z][Y][X]."""
    z, y, x = np.meshgrid(np.arange(size[2]) - size[2] // 2, np.arange(size[1]) - size[1] // 2, np.arange(size[0]) - size[0] // 2, indexing="ij")
    return x * x + y * y + z * z <= int(cfg.robot_r2_grids)


def outside_rings(pos, q, size, w, kw, rings):
    """Voxels whose elevation bin, in float64, is no ring of the lidar and not within 0.05 bin of one: the early-outs drop them."""
    rt, t = _g2l(pos, q)
    l = _voxel_positions(pos, size, w) @ rt.T + t
    pp = (np.arctan2(l[..., 2], np.hypot(l[..., 0], l[..., 1])) - f32(kw["phi_min"])) / f32(kw["phi_inc"]) + 0.5
    return (pp < -0.05) | (pp > rings + 0.05)


def run(make_ref, make_test, sensor, case):
    """One case through a pair of mappers, its tilts as successive updates.  Returns the (FREE, OCCUPIED) counts seen."""
    assert sensor == case["sensor"]
    cfg = config(case)
    size, w = case["size"], case["voxel"]
    a, b = make_ref(cfg), make_test(cfg)
    seen = [0, 0]
    skipped_in_sphere = 0
    try:
        for k, (pos, q, data, kw, restate) in enumerate(frames(case)):
            tag = "%s %s %s%s tilt %s" % (sensor, case["name"], "x".join(str(s) for s in size), " planner" if case.get("planner") else "",
                                          case["tilts"][k])
            for m in (a, b):
                m.set_pose(pos, q)
                feed(m, sensor, data, kw)
            assert a.pivot() == b.pivot(), tag
            lab = b.read_ogm()["inst_type"]
            want, sure = restate()
            if case.get("planner"):
                ball = robot_sphere(cfg, size)
                assert (lab[ball] == 1).all(), "%s: %d voxels of the robot's sphere are not FREE" % (tag, int((lab[ball] != 1).sum()))
                skipped_in_sphere += int((ball & outside_rings(pos, q, size, w, kw, case["param"][0])).sum())
                want[ball] = 1
                sure = sure | ball
            nf, no = compare_f64(lab, want, sure, tag)
            seen[0] += nf; seen[1] += no
            edge_inputs._compare(a, b, tag)              # labels and ray counts bit for bit, then fuse / batch EDT / merge and their results
        assert seen[0] > case["floors"][0] and seen[1] > case["floors"][1], (sensor, case["name"], size, seen)
        if case.get("planner"):
            assert skipped_in_sphere > 100               # the sphere reached outside the field of view: the early-outs had to let it be
    finally:
        a.close(); b.close()
    return tuple(seen)

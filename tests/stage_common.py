"""What the device tests of the query stages (SDF, NF1, frontier clusters, line of sight, display clouds, ground costmap, cost matrix)
and of the planner loop share: the mapper at the tests' settings, the label scenes and drives, local voxels to world points, the probes
of the global map, the invariant that a stage's calls write nothing of the map, and the build and input of the host-layer probes."""
import os
import subprocess

import numpy as np

import gie
import planner_scenes as ps
from gie import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1


def mapper(size, voxel=W, **kw):
    kw.setdefault("cutoff_dist", 3.0)
    return gie.Mapper(gie.make_config(voxel, size, fast_mode=False, **kw))


def update(m, pos, q, labels):
    m.set_pose(pos, q)
    m.ogm_labels(labels)
    m.step()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def closed_room(lab, x0, y0, z0, inner, unknown):
    """a closed room (local voxels): occupied walls one voxel thick around `inner` free voxels with `unknown` never-seen voxels in
    its middle; a flat volume has no floor and ceiling.  Returns (a free voxel next to the room's low corner, the never-seen box)."""
    Z, Y, X = lab.shape
    ix, iy, iz = inner
    lab[z0:min(z0 + iz + 2, Z), y0:y0 + iy + 2, x0:x0 + ix + 2] = 2
    zi0, zi1 = (z0 + 1, z0 + 1 + iz) if Z > 1 else (0, 1)
    lab[zi0:zi1, y0 + 1:y0 + 1 + iy, x0 + 1:x0 + 1 + ix] = 1
    ux, uy, uz = unknown
    uz = min(uz, zi1 - zi0)
    cx, cy, cz = x0 + 1 + (ix - ux) // 2, y0 + 1 + (iy - uy) // 2, zi0 + (zi1 - zi0 - uz) // 2
    lab[cz:cz + uz, cy:cy + uy, cx:cx + ux] = 0
    return (x0 + 1, y0 + 1, zi0), (slice(cz, cz + uz), slice(cy, cy + uy), slice(cx, cx + ux))


def scene(m, size, seed=3, room=True):
    """two updates of the solid scene of planner_scenes (with a closed room where it fits): (loc, corner voxel, never-seen box)"""
    pos, q = scenes.pose(0, m.cfg.voxel_width, delta_vox=4, yaw_deg=0.0)
    lab = ps.solid_labels(size, seed)
    corner = pocket = None
    if room and size[0] >= 40 and size[1] >= 40:
        corner, pocket = closed_room(lab, 12, 10, max(size[2] // 2 - 5, 0), (9, 9, 9), (3, 3, 3))
    for _ in range(2):
        update(m, pos, q, lab)
    return m.read_local(dist_sq=False, coc=False), corner, pocket


def world(m, v, jitter=None, pvt=None):
    """world points [n, 3] (float32 metres) of local voxels (x, y, z) at the mapper's pivot: the sum in float64, rounded once to
    float32 (for integers and for float32 voxels that is the float32 sum); `jitter` is added in float32, in voxels"""
    v = (np.asarray(v, np.float64).reshape(-1, 3) + np.array(m.pivot() if pvt is None else pvt)).astype(np.float32)
    if jitter is not None:
        v = v + jitter.astype(np.float32)
    return (v * np.float32(m.cfg.voxel_width)).astype(np.float32)


def cv(m, clearance):
    return np.float32(clearance) / np.float32(m.cfg.voxel_width)


def random_boxes(rng, n, extent, smin, smax):
    out = []
    for _ in range(n):
        s = rng.integers(smin, smax, size=3)
        lo = rng.integers(-extent, extent, size=3)
        out.append((lo, lo + s))
    return out


def box_labels(pvt, size, frame, boxes, unknown_slab=0):
    """label plane [Z][Y][X]: 2 inside the active boxes (global voxel coords, lo inclusive / hi exclusive), 1 elsewhere;
    box k is active unless (frame + k) % 4 == 3 (a quarter of the world toggles every update); optional unknown x-slab"""
    X, Y, Z = size
    gx = np.arange(X)[None, None, :] + pvt[0]
    gy = np.arange(Y)[None, :, None] + pvt[1]
    gz = np.arange(Z)[:, None, None] + pvt[2]
    lab = np.ones((Z, Y, X), np.int8)
    for k, (lo, hi) in enumerate(boxes):
        if (frame + k) % 4 == 3:
            continue
        lab[(gx >= lo[0]) & (gx < hi[0]) & (gy >= lo[1]) & (gy < hi[1]) & (gz >= lo[2]) & (gz < hi[2])] = 2
    if unknown_slab:
        lab[:, :, :unknown_slab] = 0
    return lab


class BoxDrive:
    """boxes fixed in the world that toggle from frame to frame, seen from a pose that moves out and back; a never-seen x-slab"""

    def __init__(self, size, seed=3, w=W, delta=3, unknown_slab=4):
        self.size, self.w, self.delta, self.unknown_slab = size, w, delta, unknown_slab
        self.boxes = random_boxes(np.random.default_rng(seed), 24, 60, 6, 26)

    def frame(self, k):
        pos, q = scenes.pose(k if k < 15 else 30 - k, self.w, delta_vox=self.delta, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, self.w, self.size)
        return pos, q, box_labels(pvt, self.size, k, self.boxes, self.unknown_slab)


def serpentine_cells(size, pitch, margin):
    """the voxels of ONE one-voxel-wide line snaking along x, rows `pitch` apart in y, layers `pitch` apart in z, `margin` voxels
    inside the volume's faces, in order"""
    X, Y, Z = size
    ys, zs = list(range(margin, Y - margin, pitch)), list(range(margin, Z - margin, pitch))
    cells, d = [], 0
    for li, z in enumerate(zs):
        yo = ys if li % 2 == 0 else ys[::-1]
        for yi, y in enumerate(yo):
            xs = list(range(margin, X - margin)) if d % 2 == 0 else list(range(X - margin - 1, margin - 1, -1))
            d += 1
            cells += [(x, y, z) for x in xs]
            if yi + 1 < len(yo):
                st = 1 if yo[yi + 1] > y else -1
                cells += [(xs[-1], yy, z) for yy in range(y + st, yo[yi + 1], st)]
        if li + 1 < len(zs):
            cells += [(xs[-1], yo[-1], zz) for zz in range(z + 1, zs[li + 1])]
    return np.array(cells)


def serpentine_labels(size, pitch=2):
    """labels of a walled volume with ONE corridor of free voxels (serpentine_cells at margin 1); the corridor's voxels in order"""
    c = serpentine_cells(size, pitch, 1)
    lab = np.full(size[::-1], 2, np.int8)
    lab[c[:, 2], c[:, 1], c[:, 0]] = 1
    return lab, c


def probe(m, size, rng, n=500):
    pvt = np.array(m.pivot())
    xyz = (pvt + rng.integers(-4, np.array(size) + 4, size=(n, 3))).astype(np.int32)
    return m.query_global(xyz)


def stage_calls_change_nothing(size, frames, make, calls, n_probe=500, after=None):
    """the invariant that lets a query stage run next to the map update: it writes nothing of the map.  Two mappers make(size) take
    the frames (pos, q, labels) through set_pose, ogm_labels, fuse, batch_edt, merge; on the first only, calls(a, k, phase, pos) runs
    after ogm_labels ("labels"), fuse ("fuse"), batch_edt ("edt") and merge ("merge") of frame k.  After every frame the two agree
    on every plane of read_local, on stats() and on a probe of the global map; then after(k, a, read_local's planes of a) runs."""
    a, b = make(size), make(size)
    try:
        for k, (pos, q, lab) in enumerate(frames):
            for m in (a, b):
                m.set_pose(pos, q)
                m.ogm_labels(lab)
                for phase, step in (("labels", m.fuse), ("fuse", m.batch_edt), ("edt", m.merge), ("merge", None)):
                    if m is a:
                        calls(a, k, phase, pos)
                    if step is not None:
                        step()
            la, lb = a.read_local(), b.read_local()
            for key in la:
                assert np.array_equal(la[key], lb[key]), (k, key)
            assert a.stats() == b.stats()
            assert np.array_equal(probe(a, size, np.random.default_rng(k), n_probe), probe(b, size, np.random.default_rng(k), n_probe))
            if after is not None:
                after(k, a, la)
    finally:
        a.close()
        b.close()


def lidar_frames(tmp_path):
    """the four lidar frames of the host-layer tests, [(pos, q, points)], and the path of the frames.f32 written from them: float32
    words, the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates"""
    box_world = scenes.BoxWorld(4, extent=(2.5, 2.5, 1.0), n_boxes=30)
    frames, words = [], [np.float32(4)]
    for k in range(4):
        pos, q = scenes.pose(k, W, delta_vox=3, yaw_deg=5.0)
        pts, _ = scenes.lidar_frame(box_world, k, pos, q, az=360, max_range=6.0)
        frames.append((pos, q, pts))
        words += [np.array(list(pos) + list(q) + [len(pts)], np.float32), pts.ravel()]
    fpath = str(tmp_path / "frames.f32")
    np.concatenate([np.atleast_1d(x) for x in words]).astype(np.float32).tofile(fpath)
    return frames, fpath


def build_host_probe(tmp_path, name, extra=()):
    """tests/gpu_helpers/<name>.cpp built against the project's library (with `extra` compile and link flags): the program's path"""
    import __graft_entry__ as ge
    ge.build_hip()
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "gpu_helpers", name + ".cpp"), "-o", exe,
                           "-L" + ge.CSRC, "-lgie_hip", "-Wl,-rpath," + ge.CSRC] + list(extra))
    return exe

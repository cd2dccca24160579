"""What the device tests of the line-of-sight queries and of the planner loop share: the mapper at the tests' settings, the solid
scene with a closed room, local voxels to world points, the drive past toggling boxes and the probes of the global map."""
import numpy as np

import gie
import planner_scenes as ps
from gie import scenes

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


def world(m, v, pvt=None):
    """world points (float32 metres) of local voxel coordinates (possibly fractional)"""
    pvt = np.asarray(m.pivot() if pvt is None else pvt, np.float32)
    return ((np.asarray(v, np.float32) + pvt) * np.float32(m.cfg.voxel_width)).astype(np.float32)


def cv(m, clearance):
    return np.float32(clearance) / np.float32(m.cfg.voxel_width)


def random_boxes(rng, n, extent, smin, smax):
    out = []
    for _ in range(n):
        s = rng.integers(smin, smax, size=3)
        lo = rng.integers(-extent, extent, size=3)
        out.append((lo, lo + s))
    return out


class BoxDrive:
    """boxes fixed in the world that toggle from frame to frame, seen from a pose that moves out and back; a never-seen x-slab"""

    def __init__(self, size, seed=3, w=W, delta=3):
        self.size, self.w, self.delta = size, w, delta
        self.boxes = random_boxes(np.random.default_rng(seed), 24, 60, 6, 26)

    def frame(self, k):
        pos, q = scenes.pose(k if k < 15 else 30 - k, self.w, delta_vox=self.delta, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, self.w, self.size)
        X, Y, Z = self.size
        gx = np.arange(X)[None, None, :] + pvt[0]
        gy = np.arange(Y)[None, :, None] + pvt[1]
        gz = np.arange(Z)[:, None, None] + pvt[2]
        lab = np.ones((Z, Y, X), np.int8)
        for i, (lo, hi) in enumerate(self.boxes):
            if (k + i) % 4 != 3:
                lab[(gx >= lo[0]) & (gx < hi[0]) & (gy >= lo[1]) & (gy < hi[1]) & (gz >= lo[2]) & (gz < hi[2])] = 2
        lab[:, :, :4] = 0
        return pos, q, lab


def probe(m, size, rng):
    pvt = np.array(m.pivot())
    xyz = (pvt + rng.integers(-4, np.array(size) + 4, size=(500, 3))).astype(np.int32)
    return m.query_global(xyz)

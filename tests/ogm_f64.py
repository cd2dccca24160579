"""Float64 numpy statements of the reference's projective OGM kernels, written from the reference sources (vlp16_fast.cu:8-87 +
vlp16_helper.h:35-65, realsense_fast.cu:9-94 + camera_helper.h:11-23, hokuyo_fast.cu:9-81 + hokuyo_helper.h:17-33) and sharing
nothing with include/gie_math.h or the oracle: voxel centres, the sensor-frame transform, the three classifiers and the comparison
that holds a mapper's scan labels against them.  Shared by tests/test_independent_checks.py (oracle) and tests/sensor_edges.py
(oracle, emulation and HIP library under tilted poses)."""
import math

import numpy as np


def _rot64(q):
    """Rotation matrix of a unit quaternion (w, x, y, z) in float64, the textbook form."""
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _voxel_positions(pos, size, w):
    pvt = [int(math.floor(float(np.float32(np.float32(p) / np.float32(w)) + np.float32(0.5)))) - s // 2 for p, s in zip(pos, size)]
    z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    g = np.stack([x + pvt[0], y + pvt[1], z + pvt[2]], -1).astype(np.float64) * float(np.float32(w))     # coord2pos: crd * voxel_width
    return g


def _g2l(pos, q):
    r = _rot64(np.asarray(q, np.float64) / np.linalg.norm(q))
    return r.T, -r.T @ np.asarray(pos, np.float64)


def _multiscan_f64(pos, q, size, w, img, theta_inc, theta_min, phi_inc, phi_min, min_h, max_h, eps_m=1e-4):
    """VLP_FAST::setLocalOccupancy + VLP_HELPER::G2L in float64.  Returns (labels, sure) — sure = no decision quantity of
    the voxel is within rounding distance of its threshold."""
    g = _voxel_positions(pos, size, w)
    rt, t = _g2l(pos, q)
    l = g @ rt.T + t
    ring, scan = img.shape
    theta = np.arctan2(l[..., 1], l[..., 0])
    tt = (theta - theta_min) / theta_inc + 0.5
    ti = np.floor(tt).astype(np.int64) % scan
    hor = np.sqrt(l[..., 0] ** 2 + l[..., 1] ** 2)
    phi = np.arctan2(l[..., 2], hor)
    pp = (phi - phi_min) / phi_inc + 0.5
    pi_ = np.floor(pp).astype(np.int64)
    lab = np.zeros(g.shape[:-1], np.int8)
    inr = (pi_ >= 0) & (pi_ < ring)
    real = img.astype(np.float64)[np.clip(pi_, 0, ring - 1), ti]
    ok = inr & ~np.isnan(real) & (real > 0.3)
    ideal = hor
    free = ok & (ideal < real - 0.3)
    gap = ok & (ideal >= real - 0.3) & (ideal < real - 0.1)
    beyond = ok & (ideal > real + 0.1)
    band = ok & ~free & ~gap & ~beyond                     # the height gate decides
    occ = band & (g[..., 2] >= min_h) & (g[..., 2] <= max_h)
    lab[free] = 1
    lab[occ] = 2
    # a voxel is "sure" when none of the quantities its label hangs on is within rounding distance of its threshold
    # (bins: in units of a bin; ranges and heights: metres; fp32 evaluation of the reference is off by ~1e-6 of those)
    with np.errstate(invalid="ignore"):
        m_bin = np.minimum(np.minimum(tt % 1.0, 1 - tt % 1.0), np.minimum(pp % 1.0, 1 - pp % 1.0))
        m_rng = np.minimum(np.minimum(np.abs(ideal - (real - 0.3)), np.abs(ideal - (real - 0.1))), np.abs(ideal - (real + 0.1)))
        m_h = np.minimum(np.abs(g[..., 2] - min_h), np.abs(g[..., 2] - max_h))
    sure = (m_bin > 2e-3) & (hor > 1e-3) & (~ok | (m_rng > eps_m)) & (~band | (m_h > 1e-5)) & (np.isnan(real) | (np.abs(real - 0.3) > 1e-5))
    return lab, sure


def _depth_f64(pos, q, size, w, dep, cx, cy, fx, fy, valid_nan, min_h, max_h, eps_m=1e-4):
    """REALSENSE_FAST::setLocalOccupancy + CAM_HELPER::G2L in float64."""
    g = _voxel_positions(pos, size, w)
    rt, t = _g2l(pos, q)
    l = g @ rt.T + t
    rows, cols = dep.shape
    ideal = l[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        px = -l[..., 1] * fx / ideal + cx + 0.5
        py = -l[..., 2] * fy / ideal + cy + 0.5
    pxi, pyi = np.nan_to_num(np.floor(px), nan=-1.0, posinf=-1.0, neginf=-1.0), np.nan_to_num(np.floor(py), nan=-1.0, posinf=-1.0, neginf=-1.0)
    front = (ideal > 0.3) & (ideal <= 6.0)
    inimg = front & (pxi >= 0) & (pxi < cols) & (pyi >= 0) & (pyi < rows)
    real = dep.astype(np.float64)[np.clip(pyi, 0, rows - 1).astype(np.int64), np.clip(pxi, 0, cols - 1).astype(np.int64)]
    ok = inimg & ~(real <= 0.21)
    if valid_nan:
        real = np.where(np.isnan(real), 1000.0, real)
    else:
        ok &= ~np.isnan(real)
    wv = float(np.float32(w))
    free = ok & (ideal < real - wv)
    beyond = ok & (ideal > real + wv)
    occ = ok & ~free & ~beyond & (g[..., 2] >= min_h) & (g[..., 2] <= max_h)
    lab = np.zeros(g.shape[:-1], np.int8)
    lab[free] = 1
    lab[occ] = 2
    band = ok & ~free & ~beyond
    with np.errstate(invalid="ignore"):
        m_pix = np.minimum(np.minimum(px % 1.0, 1 - px % 1.0), np.minimum(py % 1.0, 1 - py % 1.0))
        m_front = np.minimum(np.abs(ideal - 0.3), np.abs(ideal - 6.0))
        m_rng = np.minimum(np.abs(ideal - (real - wv)), np.abs(ideal - (real + wv)))
        m_h = np.minimum(np.abs(g[..., 2] - min_h), np.abs(g[..., 2] - max_h))
        m_real = np.abs(real - 0.21)
    sure = (m_front > eps_m) & (~front | (m_pix > 2e-3)) & (~inimg | np.isnan(real) | (m_real > 1e-5)) & (~ok | (m_rng > eps_m)) & (~band | (m_h > 1e-5))
    return lab, sure


def _compare(lab_ref, lab_f64, sure, what):
    assert sure.mean() > 0.8, "%s: only %.3f of the voxels are clear of every threshold" % (what, sure.mean())
    bad = sure & (lab_ref != lab_f64)
    assert not bad.any(), "%s: %d voxels differ from the float64 statement of the reference (first at %s)" % (
        what, int(bad.sum()), np.argwhere(bad)[0])
    assert (lab_ref != lab_f64).mean() < 0.01             # and the rest are a handful of ties
    return int((lab_f64 == 1).sum()), int((lab_f64 == 2).sum())


def _scan2d_f64(pos, q, size, w, rng, theta_inc, theta_min, min_h, max_h, eps_m=1e-4):
    """HOKUYO_FAST::setLocalOccupancy (hokuyo_fast.cu:9-81) + SCAN_HELPER::G2L (hokuyo_helper.h:17-33) in float64: the voxel centre
    in the sensor frame; theta = atan2(y, x) -> bin floor((theta - theta_min) / theta_inc + 0.5) modulo scan_num; the voxel is looked
    at only when |z| < voxel width (depth = horizontal range, else -1); range NaN or <= 0.3 -> nothing; ideal < real - 0.3 -> FREE;
    ideal > real + 0.3 -> nothing; else OCCUPIED inside the height gate."""
    g = _voxel_positions(pos, size, w)
    rt, t = _g2l(pos, q)
    l = g @ rt.T + t
    n = rng.shape[0]
    theta = np.arctan2(l[..., 1], l[..., 0])
    tt = (theta - theta_min) / theta_inc + 0.5
    ti = np.floor(tt).astype(np.int64) % n
    wv = float(np.float32(w))
    inplane = np.abs(l[..., 2]) < wv
    ideal = np.sqrt(l[..., 0] ** 2 + l[..., 1] ** 2)
    real = rng.astype(np.float64)[ti]
    ok = inplane & ~np.isnan(real) & (real > 0.3)
    free = ok & (ideal < real - 0.3)
    beyond = ok & (ideal > real + 0.3)
    band = ok & ~free & ~beyond
    occ = band & (g[..., 2] >= min_h) & (g[..., 2] <= max_h)
    lab = np.zeros(g.shape[:-1], np.int8)
    lab[free] = 1
    lab[occ] = 2
    with np.errstate(invalid="ignore"):
        m_bin = np.minimum(tt % 1.0, 1 - tt % 1.0)
        m_z = np.abs(np.abs(l[..., 2]) - wv)
        m_rng = np.minimum(np.abs(ideal - (real - 0.3)), np.abs(ideal - (real + 0.3)))
        m_h = np.minimum(np.abs(g[..., 2] - min_h), np.abs(g[..., 2] - max_h))
    sure = (m_z > 1e-5) & (~inplane | ((m_bin > 2e-3) & (ideal > 1e-3))) & (~ok | (m_rng > eps_m)) & (~band | (m_h > 1e-5)) \
        & (~inplane | np.isnan(real) | (np.abs(real - 0.3) > 1e-5))
    return lab, sure

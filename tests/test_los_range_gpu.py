"""gie_view_gain on the device against the exhaustive statement of tests/los_exact.py, which asks every voxel of the volume and
knows no candidate radius and no box: at r_max / w one float32 step either side of an integer k whose square is reached by
lattice vectors, at r_min == r_max, r_max == 0 and beyond the clamp of the radius at 1024, with an elevation band that has exact
ties, and with the candidate box clipped by faces, edges and corners of thin, flat and long volumes.  All counts are integers:
every comparison is of bytes."""
import hashlib

import numpy as np
import pytest

import gie
import los_exact as lx
import los_ref as lr
from gie import scenes
from stage_common import W, mapper, scene, update, world

pytestmark = pytest.mark.gpu

TIE_CASES = [(s, w) for s in lx.TIE_SIZES for w in lx.TIE_WIDTHS]
_case_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


_VISIBLE = {}


def _visible_planes(opq):
    """the exhaustive statement's visibility planes by view voxel, kept over the tests of this file by the opaque plane they
    belong to (the tie tests meet the same plane at both voxel widths: a plane is walked once)"""
    return _VISIBLE.setdefault((opq.shape, hashlib.sha1(np.ascontiguousarray(opq).tobytes()).hexdigest()), {})


def _prepared(m, size):
    """the solid scene updated twice, a prepare at clearance 0: (types, opaque plane, pivot, the plane's visibility planes)"""
    loc, _, _ = scene(m, size)
    m.los_prepare(0.0, 0)
    opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
    return loc["type"], opq, np.array(m.pivot()), _visible_planes(opq)


def _gain(m, ty, opq, pvt, views, r_min, r_max, tan2=-1.0, cache=None, vis=None):
    got = m.view_gain(views, r_min, r_max, tan2)
    ref = lx.view_gain(ty, opq, views, r_min, r_max, tan2, m.cfg.voxel_width, pvt, vis, cache)
    assert got.dtype == lr.SCORE_DTYPE and got.tobytes() == ref.tobytes(), (float(r_min), float(r_max), tan2, got, ref)
    return ref


@pytest.mark.parametrize("size,w", TIE_CASES, ids=_case_id)
def test_range_ties(size, w):
    """r_max = k * w, its float32 neighbours, and the floats whose quotient by w is k, just below and just above: the shell |d| = k
    (populated: tests/test_los_reference.py) is counted or not by one float32 step, and a candidate radius one too small loses it"""
    m = mapper(size, voxel=w)
    try:
        ty, opq, pvt, cache = _prepared(m, size)
        vis, ncand = [], 0
        for k in lx.TIE_KS:
            vox = lx.tie_views(size, k)
            views = gie.make_views(world(m, vox))
            counts = []
            for r in lx.tie_radii(k, w):
                ref = _gain(m, ty, opq, pvt, views, 0.0, r, cache=cache, vis=vis)
                counts.append((float(r / np.float32(w)), ref["candidates"].astype(np.int64)))
                ncand += int(ref["candidates"].sum())
            shell = np.array([lx.shell_count(size, p, k) for p in vox])
            below = [c for q, c in counts if q < k]
            at = [c for q, c in counts if q >= k]
            assert below and at and all(np.array_equal(a - b, shell) for a in at for b in below)
        assert sum(vis) >= ncand // 10 and ncand - sum(vis) >= ncand // 10      # neither branch of the walk is idle
    finally:
        m.close()


@pytest.mark.parametrize("size,w", TIE_CASES, ids=_case_id)
def test_shell_zero_range_and_the_clamp(size, w):
    m = mapper(size, voxel=w)
    try:
        ty, opq, pvt, cache = _prepared(m, size)
        # r_min == r_max: the candidates are exactly the shell when (r / w)^2 is k^2 as rounded, and none when it is no integer
        # (no float32 r makes r / w exactly 13 at these widths: there the shell stays empty at every neighbour)
        full = 0
        for k in (5, 13):
            vox = lx.tie_views(size, k)
            views = gie.make_views(world(m, vox))
            shell = [lx.shell_count(size, p, k) for p in vox]
            for r in lx.tie_radii(k, w):
                r2 = float(lx.thresholds(r, r, -1.0, w)[0])
                assert r2 == k * k or r2 != int(r2)
                ref = _gain(m, ty, opq, pvt, views, r, r, cache=cache)
                assert ref["candidates"].tolist() == (shell if r2 == k * k else [0] * len(vox)) and min(shell) >= 6
                full += r2 == k * k
        assert full >= 1
        # r_max == 0: no candidate — 0 in every field for a view inside, -1 outside
        vox = np.concatenate([lx.tie_views(size, 3), [(-1, 3, 0), (size[0], 0, 0)]])
        views = gie.make_views(world(m, vox))
        ref = _gain(m, ty, opq, pvt, views, 0.0, 0.0, cache=cache)
        assert (ref[:-2].view(np.int32) == 0).all() and (ref[-2:].view(np.int32) == -1).all()
        # the clamp of the candidate radius at 1024 (a launch of 2049 slices per view): the candidates are the whole volume but p
        vox = lx.tie_views(size, 3)[[0, 3, 6, 7]]
        views = gie.make_views(world(m, vox))
        for r in (np.float32(1023.9 * w), np.float32(1024 * w), np.float32(5000 * w), np.float32(3e38)):
            ref = _gain(m, ty, opq, pvt, views, 0.0, r, cache=cache)
            assert (ref["candidates"] == m.n - 1).all()
    finally:
        m.close()


@pytest.mark.parametrize("size", lx.TIE_SIZES, ids=_case_id)
def test_elevation_band_ties(size):
    """tan2_elev 0, 1 and 0.25: d_z^2 == tan2 * (d_x^2 + d_y^2) holds exactly on many voxels (counted in tests/test_los_reference.py)"""
    m = mapper(size)
    try:
        ty, opq, pvt, cache = _prepared(m, size)
        vox = lx.tie_views(size, 9)
        views = gie.make_views(world(m, vox))
        seen = []
        for tan2 in (0.0, 1.0, 0.25):
            for r in (64 * W, 1.7):                              # the whole volume, and a sphere that cuts the band
                seen.append(_gain(m, ty, opq, pvt, views, 0.0, r, tan2, cache=cache)["candidates"].astype(np.int64))
        assert (seen[0] < seen[4]).all() and (seen[4] < seen[2]).all() and (seen[0] > 0).all()
    finally:
        m.close()


# ---- the candidate box clipped by the volume
CLIP_SIZES = [(200, 5, 9), (130, 3, 40), (1, 40, 40), (70, 70, 1), (129, 2, 2), (65, 9, 130)]
CLIP_W = 0.125                                                 # a power of two: a radius of k voxels is k * w exactly
CLIP_RADII = (3, 64, 65, 200)


def clip_labels(size):
    """free space; along every axis of 9 voxels or more an occupied slab a third of the way, one voxel thick, over half of the
    cross-section (all of it on the sides shorter than 4); a never-seen block of side 5 (clipped) two thirds of the way"""
    X, Y, Z = size
    S = (X, Y, Z)
    lab = np.ones((Z, Y, X), np.int8)
    for ax in range(3):
        if S[ax] < 9:
            continue
        lo, hi = [0, 0, 0], [s // 2 + 1 if s >= 4 else s for s in S]
        if ax == 1:
            lo, hi = [s - h for s, h in zip(S, hi)], list(S)   # (the y slab covers the other half)
        lo[ax], hi[ax] = S[ax] // 3, S[ax] // 3 + 1
        lab[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = 2
    c = [(2 * s) // 3 for s in S]
    free = lab[max(c[2] - 2, 0):c[2] + 3, max(c[1] - 2, 0):c[1] + 3, max(c[0] - 2, 0):c[0] + 3]
    free[free == 1] = 0
    return lab


def clip_views(size):
    """local voxels: the eight corners, the six face centres, one voxel off each face on the inside, the centre; and, where X > 128,
    x = 0, 1, 63, 64, 65 (the first x of the clipped box, against the 64-lane step) — without repeats.  The largest volume keeps
    seven of them: the time of the file is the reference's, and it grows with voxels times line length."""
    S = np.array(size)
    c = S // 2
    v = [[x, y, z] for x in (0, S[0] - 1) for y in (0, S[1] - 1) for z in (0, S[2] - 1)] + [list(c)]
    for ax in range(3):
        for e in (0, S[ax] - 1, min(1, S[ax] - 1), max(S[ax] - 2, 0)):
            p = list(c)
            p[ax] = e
            v.append(p)
    if size[0] > 128:
        v += [[x, c[1], c[2]] for x in (0, 1, 63, 64, 65)] + [[x, 0, S[2] - 1] for x in (63, 64, 65)]
    if size[0] * size[1] * size[2] > 50000:                    # (65, 9, 130): the reference walks 76 050 lines of up to 130 voxels per
        x, y, z = S - 1                                        # view; four corners that clip every side between them, the centre,
        v = [[0, 0, 0], [x, y, 0], [x, 0, z], [0, y, z], list(c), [1, y - 1, z - 1], [c[0], c[1], 0]]      # off three faces, a face
    return np.unique(np.array(v, np.int64), axis=0)


@pytest.mark.parametrize("size", CLIP_SIZES, ids=_case_id)
def test_clipped_candidate_box(size):
    """views on corners, faces and one voxel inside them, radii of 3, 64, 65 and 200 voxels (the last wider than the volume on
    every side): rows longer than a wave from an x0 that is no multiple of 64, 1, 2, 3 and 5 rows for the four waves, X = 1, Z = 1"""
    m = mapper(size, voxel=CLIP_W)
    try:
        lab = clip_labels(size)
        pos, q = scenes.pose(0, CLIP_W, delta_vox=4, yaw_deg=0.0)
        for _ in range(2):
            update(m, pos, q, lab)
        loc = m.read_local(dist_sq=False, coc=False)
        pvt = np.array(m.pivot())
        m.los_prepare(0.0, 0)
        opq = lr.opaque(loc["type"], loc["edt"], 0.0, 0)
        assert np.array_equal(opq, lab == 2)
        vox = clip_views(size)
        views = gie.make_views(world(m, vox))
        cache, vis, ncand = _visible_planes(opq), [], 0
        for k in CLIP_RADII:
            assert np.float32(k * CLIP_W) / np.float32(CLIP_W) == k
            ref = _gain(m, loc["type"], opq, pvt, views, 0.0, k * CLIP_W, cache=cache, vis=vis)
            ncand += int(ref["candidates"].sum())
            if k == 200:
                assert (ref["candidates"] == m.n - 1).all()
        assert sum(vis) >= ncand // 10 and ncand - sum(vis) >= ncand // 10      # neither branch of the walk is idle
    finally:
        m.close()

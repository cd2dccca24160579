"""The ground costmap on the device (include/gie.h "ground costmap", gie_ground.inc.h) against the numpy statement of
tests/ground_ref.py on the types Mapper.read_local returns at the same point of the mapper's stream.  Every comparison is exact;
the closest column is checked as a witness (in range, an obstacle column, at exactly dist_sq)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gie
import ground_costmat_ref as CM
import ground_footprint_ref as FP
import ground_frontier_ref as FR
import ground_los_ref as L
import ground_nf1_ref as N
import ground_pose_nf1_ref as PQ
import ground_ref as R
import ground_rollout_ref as RO
import ground_view_ref as V
from gie import _capi, scenes
from ground_common import INVALID, ground as _ground, settle
from stage_common import W, box_labels as _box_labels, build_host_probe, lidar_frames, mapper as _mapper, stage_calls_change_nothing

pytestmark = pytest.mark.gpu
HDR_FIELDS = ("x_size", "y_size", "z_size", "x_origin", "y_origin", "z_origin", "width", "type")


def _boxes_between(rng, n, lo, hi, smin, smax):
    """n boxes (global voxel coords) of sides smin .. smax - 1 with their low corners in [lo, hi)"""
    out = []
    for _ in range(n):
        s = rng.integers(smin, smax, size=3)
        c = rng.integers(np.asarray(lo), np.asarray(hi))
        out.append((c, c + s))
    return out


def _boxes_in(rng, n, pvt, size, smin, smax):
    return _boxes_between(rng, n, np.asarray(pvt) - smin, np.asarray(pvt) + np.asarray(size), smin, smax)


def _settle(m, lab, pos=(0.0, 0.0, 0.0)):
    """two updates of one label plane at one pose: (types as read_local returns them, pivot)"""
    pvt = settle(m, lab, pos)
    return m.read_local(edt=False, dist_sq=False, coc=False)["type"], pvt


def _labels(size, fill=1):
    return np.full((size[2], size[1], size[0]), fill, np.int8)


def _check(m, vtype, size, z_lo, z_hi, min_known=1, blocks=False, pvt=None):
    """compute + read + CostMap against the reference on `vtype`; returns (the planes read, the reference)"""
    pvt = m.pivot() if pvt is None else pvt
    f = R.field(vtype, pvt, z_lo, z_hi, min_known, R.UNKNOWN_BLOCKS if blocks else 0)
    counts = m.ground_compute(z_lo, z_hi, min_known, blocks)
    g = m.read_ground()
    tag = (size, z_lo, z_hi, min_known, blocks)
    assert counts.tolist() == f["counts"].tolist(), tag
    assert np.array_equal(g["type"], f["type"]), tag
    assert np.array_equal(g["top"], f["top"]), tag
    assert np.array_equal(g["dist_sq"], f["dist_sq"]), (tag, int((g["dist_sq"] != f["dist_sq"]).sum()))
    R.check_witness(g["coc"], f, pvt)
    pay, hdr = m.read_costmap_ground()
    want, whdr = R.costmap(f, size, pvt, m.cfg.voxel_width, z_lo)
    assert pay.tobytes() == want.tobytes(), tag
    assert [getattr(hdr, k) for k in HDR_FIELDS] == [whdr[k] for k in HDR_FIELDS] and list(hdr.pad) == [0, 0, 0], tag
    return g, f


def _whole(m, size):
    z = m.pivot()[2]
    return z, z + size[2] - 1


# ---------------------------------------------------------------------------------------------------------- 1. bit rows
@pytest.mark.parametrize("X", [1, 63, 64, 65, 130])
def test_padding_and_word_counts_of_the_bit_rows(X):
    """obstacles in the first and last column of a row and just either side of a word boundary; both flag values (with
    UNKNOWN_BLOCKS every unknown column is a set bit, the padding never is)"""
    size = (X, 70, 6)
    lab = _labels(size)
    for i, x in enumerate(sorted({0, X - 1, min(62, X - 1), min(63, X - 1), min(64, X - 1), min(65, X - 1), min(127, X - 1), min(128, X - 1)})):
        lab[i % 6, (7 * i + 3) % 70, x] = 2
    lab[:, 40:44, X // 2:] = 0
    m = _mapper(size)
    try:
        vtype, _ = _settle(m, lab)
        lo, hi = _whole(m, size)
        g, f = _check(m, vtype, size, lo, hi)
        assert f["counts"][R.OCCUPIED] >= (1 if X == 1 else 2) and f["dist_sq"].max() > 0
        g, f = _check(m, vtype, size, lo, hi, blocks=True)
        assert f["counts"][R.UNKNOWN] > 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 2. projection forms
@pytest.mark.parametrize("size", [(96, 40, 9), (97, 40, 9)])
def test_both_projection_forms(size):
    rng = np.random.default_rng(size[0])
    m = _mapper(size)
    try:
        pos, q = scenes.pose(1, W, delta_vox=4, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, W, size)
        lab = _box_labels(pvt, size, 0, _boxes_in(rng, 14, pvt, size, 2, 9), unknown_slab=5)
        lab[rng.random(lab.shape) < 0.05] = 0
        vtype, pv = _settle(m, lab, pos)
        assert tuple(pv) == tuple(pvt)
        lo, hi = _whole(m, size)
        for band in ((lo, hi), (lo + 2, lo + 6), (lo + 8, lo + 8)):
            for min_known in (1, 3):
                g, f = _check(m, vtype, size, band[0], band[1], min_known, False)
                _check(m, vtype, size, band[0], band[1], min_known, True)
                if band == (lo, hi) and min_known == 1:
                    assert {R.UNKNOWN, R.OCCUPIED, R.FNT} <= set(np.unique(g["type"])) and (g["top"] != R.NO_TOP).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 3. pass Y dispatch
@pytest.mark.parametrize("Y", [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_every_line_length_of_pass_y(Y):
    """one obstacle column near y = 0 and one near y = Y - 1: the far half of each line is decided by the envelope"""
    size = (24, Y, 4)
    lab = _labels(size)
    lab[1, min(2, Y - 1), 5] = 2
    lab[2, max(Y - 3, 0), 17] = 2
    m = _mapper(size)
    try:
        vtype, _ = _settle(m, lab)
        lo, hi = _whole(m, size)
        g, f = _check(m, vtype, size, lo, hi)
        assert f["counts"][R.OCCUPIED] == 2
        if Y > 1:
            cy = g["coc"][..., 1] - m.pivot()[1]
            assert (cy == min(2, Y - 1)).any() and (cy == Y - 3).any()      # both sites win somewhere
            assert f["dist_sq"].max() >= (Y // 2 - 3) ** 2
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 4. the band
def test_bands():
    size = (40, 33, 12)
    rng = np.random.default_rng(12)
    m = _mapper(size)
    try:
        pos = (-5.03, -3.3, -2.0)                               # a pose on the negative side of the origin: a negative pivot
        pvt = scenes.local_pivot(pos, W, size)
        assert all(p < 0 for p in pvt) and pvt[2] + size[2] - 1 < 0
        lab = _box_labels(pvt, size, 0, _boxes_in(rng, 10, pvt, size, 2, 8), unknown_slab=3)
        lab[:, 20:, 30:] = np.where(rng.random((12, 13, 10)) < 0.5, 0, lab[:, 20:, 30:])
        vtype, pv = _settle(m, lab, pos)
        assert tuple(pv) == tuple(pvt)
        z = pvt[2]
        for lo, hi in ((z + 4, z + 4), (z, z + 11), (z - 7, z + 3), (z + 9, z + 30), (-2 ** 31, 2 ** 31 - 1)):
            for mk in (1, 2):
                g, f = _check(m, vtype, size, lo, hi, mk)
        assert f["counts"][R.OCCUPIED] > 0
        for lo, hi in ((z - 9, z - 1), (z + 12, z + 12)):       # entirely outside: every column UNKNOWN
            g, f = _check(m, vtype, size, lo, hi)
            assert (g["type"] == R.UNKNOWN).all() and (g["dist_sq"] == -1).all() and (g["coc"] == R.EMPTY).all() and (g["top"] == R.NO_TOP).all()
            g, f = _check(m, vtype, size, lo, hi, blocks=True)
            assert (g["dist_sq"] == 0).all()
        g, f = _check(m, vtype, size, z + 2, z + 4, min_known=4)      # min_known larger than the band: OCCUPIED or UNKNOWN
        assert set(np.unique(g["type"])) == {R.UNKNOWN, R.OCCUPIED}
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 5. column rules
def test_column_rules_and_the_difference_to_a_slice_of_the_3d_edt():
    size = (48, 40, 10)
    lab = _labels(size)
    lab[0] = 2                                                  # the floor
    lab[9] = 2                                                  # a ceiling
    lab[1:9, 18:22, 30:33] = 2                                  # a pillar
    lab[:, :, :4] = 0                                           # never seen: FNT columns at the edge of known space
    lab[5, 10, 4] = 2                                           # one OCCUPIED voxel in a column of FNT voxels
    m = _mapper(size)
    try:
        vtype, pvt = _settle(m, lab)
        z = pvt[2]
        col = vtype[1:9, 10, 4]
        assert (col == R.FNT).sum() >= 2 and (col == R.OCCUPIED).sum() == 1
        g, f = _check(m, vtype, size, z + 1, z + 8)             # the body's band: floor and ceiling lie just outside it
        assert g["type"][10, 4] == R.OCCUPIED and g["top"][10, 4] == z + 5
        assert (g["type"] == R.FNT).any() and (g["type"] == R.UNKNOWN).any() and (g["type"] == R.FREE).any()
        assert f["counts"][R.OCCUPIED] == 12 + 1                # the pillar and that voxel: neither floor nor ceiling blocks
        edt = m.read_local(vtype=False, dist_sq=False, coc=False)["edt"]
        free = g["type"] == R.FREE
        d2 = np.sqrt(g["dist_sq"].astype(np.float32))
        assert (edt[1][free] == 1.0).all() and (d2[free] >= 1.0).all() and (d2[free] > 1.0).sum() > 100      # the slice sees the floor one voxel away everywhere
        g, f = _check(m, vtype, size, z, z + 8)                 # with the floor inside the band every known column is blocked
        assert not (g["type"] == R.FREE).any() and not (g["type"] == R.FNT).any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 6. degenerate fields
def test_no_obstacle_only_obstacles_and_one_voxel():
    size = (37, 21, 1)
    m, full, one = _mapper(size), _mapper(size), _mapper((1, 1, 1))
    try:
        vtype, pvt = _settle(m, _labels(size))
        g, f = _check(m, vtype, size, pvt[2], pvt[2])
        assert (g["dist_sq"] == -1).all() and (g["coc"] == R.EMPTY).all() and f["counts"][R.OCCUPIED] == 0
        q = m.ground_query(np.zeros((3, 2), np.float32))
        assert (q["dist_sq"] == -1).all() and (q["coc"] == R.EMPTY).all() and (q["inside"] == 1).all()
        vtype, pvt = _settle(full, _labels(size, 2))
        g, f = _check(full, vtype, size, pvt[2], pvt[2])
        assert (g["dist_sq"] == 0).all() and f["counts"].tolist() == [0, 0, 37 * 21, 0]
        for fill in (2, 1):
            vtype, pvt = _settle(one, _labels((1, 1, 1), fill))
            g, f = _check(one, vtype, (1, 1, 1), pvt[2], pvt[2])
            assert g["dist_sq"].item() == (0 if fill == 2 else -1)
    finally:
        for x in (m, full, one):
            x.close()


# ---------------------------------------------------------------------------------------------------------- 7. a drive
def test_a_drive_keeps_each_field_at_its_own_pivot():
    size = (64, 48, 16)
    boxes = _boxes_between(np.random.default_rng(7), 40, (-40, -28, -10), (60, 24, 8), 3, 10)
    m = _mapper(size)
    try:
        prev = None
        pivots = set()
        for k in range(5):
            pos, q = scenes.pose(k, W, delta_vox=5, yaw_deg=0.0)
            pvt = scenes.local_pivot(pos, W, size)
            m.set_pose(pos, q)
            m.ogm_labels(_box_labels(pvt, size, k, boxes, unknown_slab=2))
            m.step()
            if prev is not None:                                 # the field computed before this update is unchanged by it
                g = m.read_ground()
                for key in g:
                    assert np.array_equal(g[key], prev[0][key]), (k, key)
                assert m.read_costmap_ground()[0].tobytes() == prev[1].tobytes()
            vtype = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
            g, f = _check(m, vtype, size, pvt[2] + 3, pvt[2] + 9, min_known=2)
            if prev is not None:
                assert not np.array_equal(g["dist_sq"], prev[0]["dist_sq"])      # the next compute follows the map
            prev = (g, m.read_costmap_ground()[0])
            pivots.add(tuple(m.pivot()))
            assert f["counts"][R.OCCUPIED] > 0
        assert len(pivots) == 5
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8. query and _dev forms
def _scene_64(m, size):
    rng = np.random.default_rng(64)
    pos, q = scenes.pose(2, W, delta_vox=3, yaw_deg=0.0)
    pvt = scenes.local_pivot(pos, W, size)
    lab = _box_labels(pvt, size, 0, _boxes_in(rng, 12, pvt, size, 2, 9), unknown_slab=4)
    return _settle(m, lab, pos)


def test_query_and_dev_forms():
    import torch
    size = (64, 40, 8)
    m = _mapper(size)
    try:
        vtype, pvt = _scene_64(m, size)
        z = pvt[2]
        g, f = _check(m, vtype, size, z + 1, z + 5, min_known=2)
        rng = np.random.default_rng(1)
        w = np.float32(W)
        cells = np.stack([rng.integers(-3, size[0] + 3, 400), rng.integers(-3, size[1] + 3, 400)], 1) + np.array(pvt[:2])
        centres = cells.astype(np.float32) * w
        borders = (cells.astype(np.float32) + np.float32(0.5)) * w          # the ties of pos2coord
        inner = (cells.astype(np.float32) + rng.uniform(-0.49, 0.49, cells.shape).astype(np.float32)) * w
        odd = np.array([[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [1e30, 0.0], [0.0, -3e9], [(pvt[0] - 1) * W, pvt[1] * W],
                        [(pvt[0] + size[0]) * W, pvt[1] * W]], np.float32)
        xy = np.concatenate([centres, borders, inner, odd]).astype(np.float32)
        got = m.ground_query(xy)
        want = R.query(f, g["coc"], pvt, W, xy)
        assert got.tobytes() == want.tobytes()
        assert 0 < got["inside"].sum() < len(xy) and (got["inside"][-7:] == 0).all()
        assert len(m.ground_query(np.zeros((0, 2), np.float32))) == 0            # n = 0 is accepted
        assert m._f["ground_query"](m._h, None, 0, None) == 0 and m._f["ground_query_dev"](m._h, None, 0, None) == 0
        # the _dev forms on the mapper's stream, back to back with no sync in between, give the host forms' bytes
        host_counts = m.ground_compute(z + 1, z + 5, 2, True)
        host = m.read_ground()
        host_pay, host_hdr = m.read_costmap_ground()
        host_q = m.ground_query(xy)
        n = size[0] * size[1]
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        with torch.cuda.stream(st):
            d_counts = torch.full((4,), 77, dtype=torch.int32, device=dev)
            d_type = torch.full((n,), 0x5a, dtype=torch.int8, device=dev)
            d_dist, d_top = (torch.full((n,), 77, dtype=torch.int32, device=dev) for _ in range(2))
            d_coc = torch.full((2 * n,), 77, dtype=torch.int32, device=dev)
            d_pay = torch.full((8 * n,), 0x5a, dtype=torch.uint8, device=dev)
            d_xy = torch.from_numpy(xy).to(dev)
            d_q = torch.full((16 * len(xy),), 0x5a, dtype=torch.uint8, device=dev)
            m.ground_compute_dev(z + 1, z + 5, 2, True, d_counts.data_ptr())
            m.read_ground_dev(d_type.data_ptr(), d_dist.data_ptr(), d_coc.data_ptr(), d_top.data_ptr())
            hdr = m.read_costmap_ground_dev(d_pay.data_ptr())
            m.ground_query_dev(d_xy.data_ptr(), len(xy), d_q.data_ptr())
            d_top_only = torch.full((n,), 77, dtype=torch.int32, device=dev)
            m.read_ground_dev(0, 0, 0, d_top_only.data_ptr())
            m.ground_compute_dev(z + 1, z + 5, 2, True, 0)       # no counts wanted
        m.sync()
        assert d_counts.cpu().numpy().tolist() == host_counts.tolist()
        assert d_type.cpu().numpy().tobytes() == host["type"].tobytes() and d_dist.cpu().numpy().tobytes() == host["dist_sq"].tobytes()
        assert d_top.cpu().numpy().tobytes() == host["top"].tobytes() == d_top_only.cpu().numpy().tobytes()
        assert d_coc.cpu().numpy().tobytes() == host["coc"].tobytes()      # the same kernels on the same planes: the same witness
        assert d_pay.cpu().numpy().tobytes() == host_pay.tobytes()
        assert bytes(hdr) == bytes(host_hdr)
        assert d_q.cpu().numpy().tobytes() == host_q.tobytes()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 8b. one mapping of a point to its cell
def _cell_table(pvt, size):
    """(points float32 [n][2], {category: indices}) around the field of `size` at `pvt`: "centres" the centres of cells at x = 0, 63, 64
    and of one cell outside each side; "ties" the pos2coord ties half a cell outside the first and the last cell of both axes, each
    with its two float32 neighbours (whichever way a tie rounds, one side of it is inside and one outside); "odd" NaN, +-inf, +-1e30
    and +-3e9 in one coordinate beside a good other one"""
    X, Y = size[0], size[1]
    w, px, py = np.float32(W), pvt[0], pvt[1]
    xm, ym = np.float32(px + 32) * w, np.float32(py + 4) * w   # a good x, a good y
    centres = [(np.float32(px + x) * w, ym) for x in (0, 63, 64, -1, X)] + [(xm, np.float32(py + y) * w) for y in (-1, Y)]
    ties = []
    for edge in (px - 0.5, px + X - 0.5):
        t = np.float32(edge) * w
        ties += [(v, ym) for v in (np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf)))]
    for edge in (py - 0.5, py + Y - 0.5):
        t = np.float32(edge) * w
        ties += [(xm, v) for v in (np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf)))]
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9]
    odd = [(v, ym) for v in bad] + [(xm, v) for v in bad]
    cat, at = {}, 0
    for name, pts in (("centres", centres), ("ties", ties), ("odd", odd)):
        cat[name] = np.arange(at, at + len(pts))
        at += len(pts)
    return np.array(centres + ties + odd, np.float32), cat


def test_every_point_taking_entry_maps_one_table_of_points_alike():
    """include/gie.h: every ground entry maps a point to its cell the way gie_ground_query does.  One table of points — cell centres
    either side of the word boundary, the rounding ties on the field's four edges, one cell outside each side, NaN, inf and values no
    int32 holds — goes through every entry that takes points, host and _dev form; each answer is its own reference's, exactly, and
    where an answer shows whether the point had a cell that is ground_nf1_ref.cells_of's verdict."""
    import torch
    size = (65, 9, 2)                                           # two bit words per row, 63 padding bits
    X, Y = size[0], size[1]
    pos = (3.0, -2.0, 0.5)
    pvt = scenes.local_pivot(pos, W, size)
    assert pvt[0] != 0 and pvt[1] != 0
    T, cat = _cell_table(pvt, size)
    cells = N.cells_of(T, pvt, W, (Y, X))
    has = np.array([c is not None for c in cells])
    # the table itself, before the device is touched: both verdicts in the categories that admit both; an odd point fails by its odd
    # coordinate alone
    for name in ("centres", "ties"):
        assert has[cat[name]].any() and not has[cat[name]].all(), name
    assert [cells[i] for i in cat["centres"][:3]] == [(0, 4), (63, 4), (64, 4)]
    for k in range(0, len(cat["ties"]), 3):                    # around each tie one neighbour is inside and one outside
        assert has[cat["ties"][k]] != has[cat["ties"][k + 2]], k
    assert not has[cat["odd"]].any()
    for i, j in enumerate(cat["odd"]):
        k = int(i >= len(cat["odd"]) // 2)                      # the first half is odd in x, the second in y
        fixed = T[j].copy()
        fixed[k] = T[1, k]                                      # (T[1]: the centre of cell (63, 4))
        assert np.isfinite(fixed).all() and N.cells_of(fixed[None], pvt, W, (Y, X))[0] is not None, j
    lab = _labels(size)
    lab[:, 0, :] = lab[:, -1, :] = lab[:, :, 0] = lab[:, :, -1] = 2      # a one-cell frame of walls
    lab[:, 5, 30] = 0                                           # one never-seen cell
    n = len(T)
    inside_pt = np.float32([(pvt[0] + 32) * W, (pvt[1] + 2) * W])
    seg_a, seg_b = np.concatenate([T, np.tile(inside_pt, (n, 1))]), np.concatenate([np.tile(inside_pt, (n, 1)), T])
    traj = T.reshape(n, 1, 2)
    head = np.tile(np.int32([[[1, 0]]]), (n, 1, 1))
    m = _mapper(size)
    try:
        assert tuple(settle(m, lab, pos)) == tuple(pvt)
        g = _ground(m, size)
        assert (g["type"] == R.UNKNOWN).sum() == 1 and (g["type"] == R.OCCUPIED).sum() == 2 * X + 2 * Y - 4
        trav = N.traversable(g)
        on_free = np.array([c is not None and bool(trav[c[1], c[0]]) for c in cells])
        decided = ~has | on_free                                # where a value of a field tells whether the point had a cell
        assert on_free.any() and (has & ~on_free).any()
        # ---- the references
        want = {"query": R.query(g, g["coc"], pvt, W, T)}
        want["nf"], want["ns"] = N.field(g, T, pvt, W)
        nf1, _ = N.field(g, inside_pt[None], pvt, W)
        want["steps"] = FR.gather(nf1, T, pvt, W)
        want["path"], want["len"] = N.path(nf1, T, pvt, W, 8)
        want["hits"] = L.segments(g, seg_a, seg_b, pvt, W)
        want["cost"], want["valid"] = CM.matrix(g, T, pvt, W)
        want["gain"] = V.gain(g, T, pvt, 0.0, 0.45, W)
        want["roll"] = RO.rollouts(g, traj, pvt, W)
        want["foot"] = FP.footprints(g, traj, head, pvt, W, 0, 0, 0)
        want["pnf"], want["cs"], want["pcounts"] = PQ.field(g, T, None, pvt, W, 0, 0, 0)
        want["psteps"] = PQ.query(want["pnf"], T, None, pvt, W)
        # ---- the host forms
        got = {"query": m.ground_query(T)}
        got["ns"] = m.ground_nf1_compute(T)
        got["nf"] = m.read_ground_nf1()
        assert m.ground_nf1_compute(inside_pt[None]) == 1
        got["steps"] = m.ground_nf1_query(T)
        got["path"], got["len"] = m.ground_nf1_path(T, 8)
        got["hits"] = m.ground_segments(seg_a, seg_b)
        got["cost"], got["valid"] = m.ground_costmat(T)
        got["gain"] = m.ground_view_gain(T, 0.0, 0.45)
        got["roll"] = m.ground_rollouts(traj)
        got["foot"] = m.ground_footprints(traj, head, 0, 0, 0)
        got["pcounts"] = m.ground_pose_nf1_compute(T, None, 0, 0, 0)
        got["pnf"], got["cs"] = m.read_ground_pose_nf1()
        got["psteps"] = m.ground_pose_nf1_query(T)
        for key in want:
            a, b = np.asarray(got[key]), np.asarray(want[key])
            assert a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes(), key
        # ---- each entry's verdict on "this point has a cell"
        verdict = {"query": got["query"]["inside"] == 1, "segments a": got["hits"]["first"][:n] != -2, "segments b": got["hits"]["first"][n:] != -2,
                   "view": got["gain"]["candidates"] >= 0, "rollouts": got["roll"]["end"] != RO.LEFT, "footprints": got["foot"]["end"] != FP.NO_PLACEMENT}
        for key, v in verdict.items():
            assert np.array_equal(v, has), key
        fields = {"nf1 goals": np.array([c is not None and got["nf"][c[1], c[0]] == 0 for c in cells]), "nf1 query": got["steps"] >= 0,
                  "nf1 path": got["len"] > 0, "costmat": got["valid"], "pose query": got["psteps"] >= 0,
                  "pose goals": np.array([c is not None and bool((got["pnf"][:, c[1], c[0]] == 0).all()) for c in cells])}
        for key, v in fields.items():
            assert np.array_equal(v[decided], has[decided]) and not v[~has].any(), key
        # ---- the _dev forms on the mapper's stream, back to back: the host forms' bytes
        dev = torch.device("cuda", 0)
        st = torch.cuda.ExternalStream(m.stream_handle(), device=dev)
        out = {}

        def buf(key, nbytes):
            out[key] = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=dev)
            return out[key].data_ptr()
        with torch.cuda.stream(st):
            d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
                 (("T", T), ("p", inside_pt[None]), ("a", seg_a), ("b", seg_b), ("head", head))}
            m.ground_query_dev(d["T"].data_ptr(), n, buf("query", 16 * n))
            m.ground_nf1_compute_dev(d["T"].data_ptr(), n, d_n_sources=buf("ns", 4))
            m.read_ground_nf1_dev(buf("nf", 4 * X * Y))
            m.ground_nf1_compute_dev(d["p"].data_ptr(), 1)
            m.ground_nf1_query_dev(d["T"].data_ptr(), n, buf("steps", 4 * n))
            d_path = torch.zeros((n * 8 * 2,), dtype=torch.int32, device=dev)
            m.ground_nf1_path_dev(d["T"].data_ptr(), n, 8, d_path.data_ptr(), buf("len", 4 * n))
            m.ground_segments_dev(d["a"].data_ptr(), d["b"].data_ptr(), 2 * n, buf("hits", 24 * 2 * n))
            m.ground_costmat_dev(d["T"].data_ptr(), n, buf("cost", 4 * n * n), buf("valid", n))
            m.ground_view_gain_dev(d["T"].data_ptr(), 0, n, buf("gain", 16 * n), 0.0, 0.45)
            m.ground_rollouts_dev(d["T"].data_ptr(), n, 1, buf("roll", 48 * n))
            m.ground_footprints_dev(d["T"].data_ptr(), d["head"].data_ptr(), n, 1, buf("foot", 32 * n), 0, 0, 0)
            m.ground_pose_nf1_compute_dev(d["T"].data_ptr(), 0, n, buf("pcounts", 8), 0, 0, 0)
            m.read_ground_pose_nf1_dev(buf("pnf", 4 * 8 * X * Y), buf("cs", X * Y))
            m.ground_pose_nf1_query_dev(d["T"].data_ptr(), 0, n, buf("psteps", 4 * n))
        m.sync()
        out["path"] = d_path
        for key, t in out.items():
            host = np.asarray(got[key], np.int32) if key in ("ns", "pcounts") else np.asarray(got[key])
            assert t.cpu().numpy().tobytes() == (host.astype(np.uint8) if key == "valid" else host).tobytes(), key
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 9. the update does not notice
def test_ground_calls_change_nothing_of_the_map_update():
    size = (48, 40, 16)
    boxes = _boxes_between(np.random.default_rng(5), 40, (-30, -24, -10), (50, 20, 8), 3, 10)

    def frame(k):
        pos, q = scenes.pose(k, W, delta_vox=3, yaw_deg=0.0)
        return pos, q, _box_labels(scenes.local_pivot(pos, W, size), size, k, boxes, unknown_slab=3)

    def calls(a, k, phase, pos):
        z = scenes.local_pivot(pos, W, size)[2]
        if phase == "fuse":                                  # between fuse and merge
            a.ground_compute(z + 2, z + 9, 2, k % 2 == 1)
            a.read_ground()
        elif phase == "merge":
            a.ground_compute(z, z + 15)
            a.read_costmap_ground()
            a.ground_query(np.random.default_rng(k).uniform(-4, 4, (300, 2)).astype(np.float32))
    stage_calls_change_nothing(size, (frame(k) for k in range(8)), _mapper, calls, n_probe=2000)


# ---------------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_write_nothing():
    import torch
    size = (32, 24, 8)
    m, fresh, posed, t = _mapper(size), _mapper(size), _mapper(size), _mapper(size)
    try:
        vtype, pvt = _settle(m, _labels(size))
        f = m._f
        n = size[0] * size[1]
        POISON = bytes([0x5a])
        counts = np.frombuffer(POISON * 16, np.int32).copy()
        planes = [np.frombuffer(POISON * (n * k), np.uint8).copy() for k in (1, 4, 8, 4)]
        pay = np.frombuffer(POISON * (8 * n), np.uint8).copy()
        hdr = _capi.CostMapHdr.from_buffer_copy(POISON * C.sizeof(_capi.CostMapHdr))
        cells = np.frombuffer(POISON * (16 * 5), np.uint8).copy()
        xy = np.zeros((5, 2), np.float32)
        dbuf = torch.full((16 * n,), 0x5a, dtype=torch.uint8, device="cuda:0")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        dp = C.c_void_p(dbuf.data_ptr())

        def P(**kw):
            p = _capi.GroundParam(pvt[2], pvt[2] + 3, 1, 0)
            for k, v in kw.items():
                if k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        def unwritten():
            m.sync()
            assert counts.tobytes() == POISON * 16 and all(a.tobytes() == POISON * a.size for a in planes + [pay, cells])
            assert bytes(hdr) == POISON * C.sizeof(_capi.CostMapHdr) and bool((dbuf == 0x5a).all())

        def readers(h, who):
            """every reader and query of handle h, host and _dev, refuses"""
            assert f["read_ground"](h, *[ptr(a) for a in planes]) == INVALID, who
            assert f["read_ground_dev"](h, dp, dp, dp, dp) == INVALID, who
            assert f["read_costmap_ground"](h, ptr(pay), C.byref(hdr)) == INVALID, who
            assert f["read_costmap_ground_dev"](h, dp, C.byref(hdr)) == INVALID, who
            assert f["ground_query"](h, ptr(xy), 5, ptr(cells)) == INVALID, who
            assert f["ground_query_dev"](h, dp, 5, dp) == INVALID, who

        bad = [P(z_lo=5, z_hi=4), P(min_known=0), P(min_known=-3), P(flags=2), P(flags=3), P(flags=-2 ** 31),
               P(reserved=0), P(reserved=1), P(reserved=2), P(reserved=3)]
        for name, out in (("ground_compute", ptr(counts)), ("ground_compute_dev", dp)):
            for p in bad:
                assert f[name](m._h, C.byref(p), out) == INVALID, (name, p.z_lo, p.z_hi, p.min_known, p.flags, list(p.reserved))
            assert f[name](m._h, None, out) == INVALID                               # a NULL param
            assert f[name](None, C.byref(P()), out) == INVALID                       # a NULL handle
            assert f[name](fresh._h, C.byref(P()), out) == INVALID                   # before the first gie_set_pose
        readers(None, "null handle")
        readers(m._h, "before the first compute")                                   # (every compute so far was refused)
        readers(fresh._h, "fresh")
        unwritten()
        # a tiled mapper: all eight refuse
        t.set_tile((8, 0, 0), (64, 24, 8))
        assert f["ground_compute"](t._h, C.byref(P()), ptr(counts)) == INVALID and f["ground_compute_dev"](t._h, C.byref(P()), dp) == INVALID
        readers(t._h, "tiled")
        unwritten()
        # after a compute: all four outputs NULL, n < 0, NULL points or records, a NULL device payload
        posed.set_pose((0.0, 0.0, 0.0))
        assert f["ground_compute"](posed._h, C.byref(P()), None) == 0                # counts may be NULL; a pose is enough
        assert f["ground_compute"](m._h, C.byref(P()), None) == 0
        assert f["read_ground"](m._h, None, None, None, None) == INVALID and f["read_ground_dev"](m._h, None, None, None, None) == INVALID
        for name in ("ground_query", "ground_query_dev"):
            out, pts = (ptr(cells), ptr(xy)) if name == "ground_query" else (dp, dp)
            assert f[name](m._h, pts, -1, out) == INVALID and f[name](m._h, None, 5, out) == INVALID and f[name](m._h, pts, 5, None) == INVALID
        assert f["read_costmap_ground_dev"](m._h, None, C.byref(hdr)) == INVALID
        unwritten()
        assert f["ground_query"](m._h, ptr(xy), 5, ptr(cells)) == 0                  # (the same call with good arguments works)
        assert cells.view(gie.GROUND_CELL_DTYPE)["inside"].tolist() == [1] * 5
    finally:
        for x in (m, fresh, posed, t):
            x.close()


# ---------------------------------------------------------------------------------------------------------- 11. profile
def test_profile_entries():
    size = (32, 24, 8)
    m = _mapper(size)
    try:
        _settle(m, _labels(size, 2))
        z = m.pivot()[2]
        m.profile_enable(True)
        m.profile_read()
        m.ground_compute(z, z + 7)
        m.read_ground()
        m.read_costmap_ground()
        m.ground_query(np.zeros((4, 2), np.float32))
        prof = m.profile_read()
        m.profile_enable(False)
        assert prof["ground"][1] == 3 and prof["ground"][0] > 0 and prof["ground_query"][1] == 1 and prof["ground_query"][0] > 0
        names = list(prof)
        assert names.index("ground") == names.index("ground_query") - 1 == names.index("cloud") - 2 and names[0] == "ogm_classify"
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 12. at size
def test_at_size_512x512x24():
    size = (512, 512, 24)
    rng = np.random.default_rng(512)
    boxes = [(lo, lo + s) for lo, s in zip(np.stack([rng.integers(-250, 250, 300), rng.integers(-250, 250, 300), rng.integers(-14, 10, 300)], 1),
                                           rng.integers(2, 12, (300, 3)))]
    m = _mapper(size, cutoff_dist=1.0)
    try:
        pos, q = scenes.pose(0, W, delta_vox=4, yaw_deg=0.0)
        pvt = scenes.local_pivot(pos, W, size)
        lab = _box_labels(pvt, size, 0, boxes, unknown_slab=6)
        vtype, _ = _settle(m, lab, pos)
        g, f = _check(m, vtype, size, pvt[2] + 4, pvt[2] + 15, min_known=3)
        assert f["counts"][R.OCCUPIED] > 2000 and f["dist_sq"].max() > 400
        _check(m, vtype, size, pvt[2], pvt[2] + 23, blocks=True)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- 13. host layer
def test_host_layer_ground_costmap_matches_the_mapper(tmp_path):
    exe = build_host_probe(tmp_path, "ground_host_probe")
    size, w, cutoff, gmin, gmax, min_known = (48, 40, 33), 0.1, 3.0, -0.72, 0.43, 2
    frames, fpath = lidar_frames(tmp_path)
    m = _mapper(size, voxel=w, cutoff_dist=cutoff)
    try:
        for pos, q, pts in frames:
            m.set_pose(pos, q)
            m.ogm_pointcloud(pts)
            m.set_ext_boxes(np.array([[-3.6, -3.2, 0.2]], np.float32), np.array([[4.4, 3.4, 2.6]], np.float32), np.zeros(1, np.uint8))
            m.fuse(); m.batch_edt(); m.merge()
        z_lo, z_hi = scenes.pos2coord(gmin, w), scenes.pos2coord(gmax, w)
        counts = m.ground_compute(z_lo, z_hi, min_known)
        pay, hdr = m.read_costmap_ground()
        vtype = m.read_local(edt=False, dist_sq=False, coc=False)["type"]
        _check(m, vtype, size, z_lo, z_hi, min_known)
    finally:
        m.close()
    assert counts[R.OCCUPIED] > 0 and counts[R.FREE] + counts[R.FNT] > 0 and counts[R.UNKNOWN] > 0
    args = [fpath, None, repr(w), str(size[0]), str(size[1]), str(size[2]), repr(cutoff)]
    out = str(tmp_path / "on")
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + [repr(gmin), repr(gmax), str(min_known)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 4 cells %d" % (size[0] * size[1]) in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".payload", np.uint8).tobytes() == pay.tobytes()
    assert np.fromfile(out + ".hdr", np.uint8).tobytes() == bytes(hdr)
    assert np.fromfile(out + ".counts", np.int32).tolist() == counts.tolist()
    out = str(tmp_path / "off")                                 # the default, max < min: the section is off
    res = subprocess.run([exe] + args[:1] + [out] + args[2:] + ["0", "-1", "1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "made 0 cells 0" in res.stdout, (res.stdout, res.stderr)
    assert np.fromfile(out + ".hdr", np.uint8).tobytes() == bytes([0x5a]) * C.sizeof(_capi.CostMapHdr)

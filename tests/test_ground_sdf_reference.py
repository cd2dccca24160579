"""tests/ground_sdf_ref.py (the numpy statement of include/gie.h "ground signed distance") against statements that share nothing with it:
an O(cells²) brute force for the inside distances, float64 bilinear interpolation for the query, a literal loop for the record — and
the section's declarations in the header, the binding, the host layer and the built library.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

import gie
import ground_ref as R
import ground_sdf_ref as S
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
PVT = (-7, 40, 3)
NAMES = ["read_ground_sdf", "read_ground_sdf_dev", "ground_query_sdf", "ground_query_sdf_dev", "ground_sdf_rollouts", "ground_sdf_rollouts_dev"]


def _brute(obs):
    """inside_dist_sq by definition: every obstacle cell against every cell that is none"""
    Y, X = obs.shape
    free = np.argwhere(~obs)
    out = np.zeros((Y, X), np.int32)
    for y in range(Y):
        for x in range(X):
            if obs[y, x]:
                out[y, x] = -1 if not len(free) else int(((free[:, 0] - y) ** 2 + (free[:, 1] - x) ** 2).min())
    return out


def _grids(shape, rng):
    Y, X = shape
    yield "no obstacle", np.zeros(shape, bool)
    yield "obstacles only", np.ones(shape, bool)
    for cy, cx in ((0, 0), (0, X - 1), (Y - 1, 0), (Y - 1, X - 1)):
        o = np.ones(shape, bool)
        o[cy, cx] = False
        yield "one free cell in a corner", o
    o = np.zeros(shape, bool)
    o[:, X // 2:] = True                                        # a block reaching the right edge
    yield "block to the right edge", o
    for k in range(6):
        yield "random %d" % k, rng.random(shape) < (0.3, 0.6, 0.9)[k % 3]


def test_inside_distances_equal_the_brute_force():
    rng = np.random.default_rng(30)
    deep = 0
    for shape in ((5, 7), (9, 70), (9, 1)):                     # [Y][X]: 7 x 5, 70 x 9 and 1 x 9
        for what, obs in _grids(shape, rng):
            got, want = S.inside_dist_sq(obs), _brute(obs)
            assert got.dtype == np.int32 and np.array_equal(got, want), (shape, what)
            deep += int((want > 1).sum())
            # the gate's rule: a cell is deeper than 1 (or the rectangle has no free cell) only if it is interior
            assert np.array_equal(S.interior(obs), obs & (want != 1)), (shape, what)
    assert deep > 300
    o = np.ones((9, 70), bool)
    o[8, 0] = False
    assert S.inside_dist_sq(o)[0, 69] == 69 * 69 + 8 * 8         # the closed form of one free cell in a corner


def test_gsdf_is_the_costmap_outside_and_on_the_surface():
    size = (7, 5, 4)
    far = np.float32(7 * 7 + 5 * 5 + 4 * 4)
    t = np.full((5, 7), R.FREE, np.int8)
    t[1:4, 2:7] = R.OCCUPIED
    t[0, 0] = R.UNKNOWN
    for blocks in (False, True):
        obs = R.obstacles(t, R.UNKNOWN_BLOCKS if blocks else 0)
        g = {"type": t, "dist_sq": R.dist_sq(obs)}
        f = S.field(g, size, blocks)
        pay, _ = R.costmap({"dist_sq": g["dist_sq"], "type": t}, size, PVT, W, 0)
        same = f["inside_dist_sq"] <= 1
        assert np.array_equal(f["sdf"][same].view(np.uint32), pay["d"][same].view(np.uint32)) and (f["sdf"][f["obs"] & same] == 0).all()
        assert f["inside_dist_sq"][2, 5] == 4 and f["sdf"][2, 5] == np.float32(-1.0) and (~same).sum() == 4      # (3 .. 6, 2): the block reaches the right edge
        assert bool(f["obs"][0, 0]) == blocks
    none = {"type": np.full((5, 7), R.FREE, np.int8), "dist_sq": np.full((5, 7), -1, np.int32)}
    assert (S.field(none, size)["sdf"] == far).all()
    full = {"type": np.full((5, 7), R.OCCUPIED, np.int8), "dist_sq": np.zeros((5, 7), np.int32)}
    f = S.field(full, size)
    assert (f["inside_dist_sq"] == -1).all() and (f["sdf"] == -far).all()


def _scene(shape, rng):
    Y, X = shape
    t = np.full(shape, R.FREE, np.int8)
    t[rng.random(shape) < 0.1] = R.UNKNOWN
    t[Y // 4:Y // 4 + 6, X // 3:X // 3 + 9] = R.OCCUPIED
    t[rng.random(shape) < 0.05] = R.OCCUPIED
    obs = R.obstacles(t)
    return {"type": t, "dist_sq": R.dist_sq(obs)}


def test_query_against_float64_bilinear_interpolation():
    """The bound, from the float32 rounding of the header's operations, eps = 2^-24 the unit roundoff, V the largest |corner| and D the
    largest difference of two corners of the cell:
      u = p / w - pvt is two roundings: |du| <= eps (|p / w| + |u|) <= 2 eps (|pvt| + size) per axis; t = u - i0 is exact (u and i0
      lie within a factor of two, or i0 = 0); the interpolant is continuous over the rectangle with slope at most D per axis, so the
      coordinates' error moves it by at most D (|du_x| + |du_y|), whichever cell either side picks;
      sx, sy: one rounding each; c0, c1: three each, on values <= V; the second level three more and the product with w one: fewer
      than 16 eps V in all.
    dist (metres): w (16 eps V + D (|du_x| + |du_y|)).  The gradient is continuous only INSIDE a cell: it is compared where both sides
    pick the same cell (no coordinate within 1e-3 of an integer), with 12 eps D for its own operations and 2 D |du| for the
    weights."""
    rng = np.random.default_rng(31)
    eps = 2.0 ** -24
    shape = (20, 65)
    Y, X = shape
    g = _scene(shape, rng)
    f = S.field(g, (X, Y, 8))
    assert (f["inside_dist_sq"] > 1).sum() >= 20
    cells = rng.uniform(-1.0, [X, Y], (2000, 2))
    xy = ((cells + np.array(PVT[:2])) * W).astype(np.float32)
    dist, grad, flags = S.query(f, g, PVT, W, xy)
    w32 = np.float32(W)
    u = xy.astype(np.float64) / np.float64(w32) - np.array(PVT[:2], np.float64)
    inside64 = (u[:, 0] >= 0) & (u[:, 0] <= X - 1) & (u[:, 1] >= 0) & (u[:, 1] <= Y - 1)
    edge = (np.abs(u[:, 0] - np.clip(u[:, 0], 0, X - 1)) < 1e-3) & (np.abs(u[:, 1] - np.clip(u[:, 1], 0, Y - 1)) < 1e-3) & \
        ((np.abs(u[:, 0]) < 1e-3) | (np.abs(u[:, 0] - (X - 1)) < 1e-3) | (np.abs(u[:, 1]) < 1e-3) | (np.abs(u[:, 1] - (Y - 1)) < 1e-3))
    assert not edge.any()                                       # no sample within rounding of the rectangle's faces: both sides agree on `inside`
    assert np.array_equal(flags & 1, inside64.astype(np.uint8)) and 1500 < inside64.sum() < 2000
    assert np.isnan(dist[~inside64]).all() and (grad[~inside64] == 0).all() and (flags[~inside64] == 0).all()
    sdf = f["sdf"].astype(np.float64)
    du = 2 * eps * (np.abs(np.array(PVT[:2])).max() + max(X, Y))
    checked = 0
    for p in np.flatnonzero(inside64):
        ix, iy = min(int(np.floor(u[p, 0])), X - 2), min(int(np.floor(u[p, 1])), Y - 2)
        tx, ty = u[p, 0] - ix, u[p, 1] - iy
        v = [sdf[iy, ix], sdf[iy, ix + 1], sdf[iy + 1, ix], sdf[iy + 1, ix + 1]]
        c0, c1 = v[0] * (1 - tx) + v[1] * tx, v[2] * (1 - tx) + v[3] * tx
        V, D = max(abs(x) for x in v), max(v) - min(v)
        assert abs(float(dist[p]) - (c0 * (1 - ty) + c1 * ty) * float(w32)) <= float(w32) * (16 * eps * V + 2 * D * du), p
        if min(abs(u[p, 0] - round(u[p, 0])), abs(u[p, 1] - round(u[p, 1]))) > 1e-3:
            gx, gy = (v[1] - v[0]) * (1 - ty) + (v[3] - v[2]) * ty, c1 - c0
            assert abs(float(grad[p, 0]) - gx) <= 12 * eps * D + 2 * D * du and abs(float(grad[p, 1]) - gy) <= 16 * eps * V + 2 * D * du, p
            checked += 1
        want = 1 | (2 if all(g["type"][y, x] != R.UNKNOWN for y in (iy, iy + 1) for x in (ix, ix + 1)) else 0) | \
            (4 if any(f["obs"][y, x] for y in (iy, iy + 1) for x in (ix, ix + 1)) else 0)
        if min(abs(u[p, 0] - round(u[p, 0])), abs(u[p, 1] - round(u[p, 1]))) > 1e-3:
            assert flags[p] == want, p
    assert checked > 1400 and len(set(flags.tolist())) >= 5


def test_query_faces_flat_axes_and_values_that_are_no_point():
    t = np.full((1, 9), R.FREE, np.int8)                        # 9 x 1: y is flat
    t[0, 3:8] = R.OCCUPIED
    g = {"type": t, "dist_sq": R.dist_sq(t == R.OCCUPIED)}
    f = S.field(g, (9, 1, 1))
    assert f["inside_dist_sq"][0].tolist() == [0, 0, 0, 1, 4, 9, 4, 1, 0]
    pv = (0, 0, 0)
    pts = np.array([[0.0, 0.0], [0.8, 0.0], [0.80001, 0.0], [0.5, -0.05], [0.5, 0.04999], [0.5, 0.05], [0.5, -0.0501], [0.45, 0.0],
                    [np.nan, 0.0], [0.1, np.inf], [-np.inf, 0.0], [1e30, 0.0], [0.1, -1e30]], np.float32)
    dist, grad, flags = S.query(f, g, pv, W, pts)
    assert flags.tolist() == [3, 7, 0, 7, 7, 0, 0, 7, 0, 0, 0, 0, 0]        # (u = 8 is the last face: the cell 7 | 8, and 7 is an obstacle)
    assert (grad[:, 1] == 0).all() and np.isnan(dist[flags == 0]).all() and (grad[flags == 0] == 0).all()
    assert dist[3] == np.float32(-2.0) * np.float32(W) and grad[3, 0] == 1        # the deepest cell's centre, 1 - sqrt(9), belongs to the cell 5 | 6: up to -1
    u = np.float32(0.45) / np.float32(W)
    assert 4 < u < 5 and grad[7, 0] == np.float32(-1.0) and dist[7] < 0            # between -1 and -2


def _literal(dist, grad, flags, margin):
    m = 0
    for k in range(len(dist)):
        if not flags[k] & 1:
            break
        m += 1
    best = None
    below = [k for k in range(m) if dist[k] < np.float32(margin)]
    inn = [k for k in range(m) if dist[k] <= 0]
    for k in range(m):
        if best is None or dist[k] < dist[best]:
            best = k
    return (m, -1 if best is None else best, np.float32(np.nan) if best is None else dist[best], (0, 0) if best is None else tuple(grad[best]),
            below[0] if below else -1, len(below), inn[0] if inn else -1)


def test_record_against_a_literal_loop():
    rng = np.random.default_rng(32)
    kinds = set()
    for rep in range(300):
        T = int(rng.integers(1, 140))
        dist = rng.choice(np.array([-0.3, -0.1, -0.0, 0.0, 0.1, 0.1, 0.25, 0.7], np.float32), T)
        grad = rng.standard_normal((T, 2)).astype(np.float32)
        flags = np.where(rng.random(T) < 0.02, 0, rng.choice([1, 3, 5, 7], T)).astype(np.uint8)
        if rep % 7 == 0:
            flags[0] = 0
        dist[flags == 0] = np.nan
        margin = float(rng.choice([0.0, 0.1, 0.2, 1.0]))
        r = S.record(dist, grad, flags, margin)
        want = _literal(dist, grad, flags, margin)
        got = (int(r["points"]), int(r["argmin"]), r["min_dist"], tuple(r["grad"]), int(r["first_below"]), int(r["n_below"]), int(r["first_in"]))
        assert got[:2] == want[:2] and got[4:] == want[4:] and got[3] == want[3], (rep, got, want)
        assert np.array([got[2]], np.float32).view(np.uint32) == np.array([want[2]], np.float32).view(np.uint32)
        kinds.add((want[0] == 0, want[0] == T, 0 <= want[4] < want[1], want[6] >= 0))
        assert want[4] <= want[1] and want[6] <= want[1]        # (the least dist is below the margin if any is: neither index can lie behind argmin)
    assert len(kinds) >= 6
    # the first of equal minima wins, -0 and +0 are equal, and margin 0 counts the points inside only
    d = np.array([0.5, 0.0, -0.0, 0.0, 0.5], np.float32)
    r = S.record(d, np.arange(10, dtype=np.float32).reshape(5, 2), np.ones(5, np.uint8), 0.0)
    assert (int(r["points"]), int(r["argmin"]), int(r["first_below"]), int(r["n_below"]), int(r["first_in"])) == (5, 1, -1, 0, 1) and r["grad"].tolist() == [2.0, 3.0]
    r = S.record(d, np.zeros((5, 2), np.float32), np.array([0, 1, 1, 1, 1], np.uint8), 1.0)
    assert (int(r["points"]), int(r["argmin"]), int(r["first_below"]), int(r["n_below"]), int(r["first_in"])) == (0, -1, -1, 0, -1) and np.isnan(r["min_dist"])


def test_rollouts_are_the_records_of_the_queries():
    rng = np.random.default_rng(33)
    g = _scene((20, 65), rng)
    f = S.field(g, (65, 20, 8))
    cells = rng.uniform(-2, [66, 21], (1, 1, 2)) + np.cumsum(rng.uniform(-1, 1, (30, 70, 2)), 1)
    xy = ((cells + np.array(PVT[:2])) * W).astype(np.float32)
    xy[3, 40:] = np.nan
    rec, dist, grad = S.rollouts(f, g, PVT, W, xy, 0.15)
    qd, qg, qf = S.query(f, g, PVT, W, xy.reshape(-1, 2))
    assert np.array_equal(dist.view(np.uint32).ravel(), qd.view(np.uint32)) and np.array_equal(grad.view(np.uint32).reshape(-1, 2), qg.view(np.uint32))
    for i in range(30):
        assert rec[i].tobytes() == S.record(qd.reshape(30, 70)[i], qg.reshape(30, 70, 2)[i], qf.reshape(30, 70)[i], 0.15).tobytes()
    assert rec.dtype == S.ROLLOUT_DTYPE and rec["points"][3] <= 40 and (rec["points"] > 0).sum() > 3


def test_struct_sizes_and_offsets():
    st = _capi.GroundSdfRolloutParam
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == (32, [("margin", 0, 4), ("flags", 4, 4), ("reserved", 8, 24)])
    st = _capi.GroundSdfRollout
    assert (C.sizeof(st), [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_]) == \
        (32, [("points", 0, 4), ("argmin", 4, 4), ("min_dist", 8, 4), ("grad", 12, 8), ("first_below", 20, 4), ("n_below", 24, 4), ("first_in", 28, 4)])
    dt = gie.GROUND_SDF_ROLLOUT_DTYPE
    assert dt == S.ROLLOUT_DTYPE and dt.itemsize == 32 and [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct gie_ground_sdf_rollout_param \{(.*?)\} gie_ground_sdf_rollout_param;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|float)\s+([\w, \[\]]+);", body) == [("float", "margin"), ("int32_t", "flags"), ("int32_t", "reserved[6]")]
    body = re.search(r"typedef struct gie_ground_sdf_rollout \{(.*?)\} gie_ground_sdf_rollout;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|float)\s+([\w, \[\]]+);", body) == [("int32_t", "points"), ("int32_t", "argmin"), ("float", "min_dist"), ("float", "grad[2]"),
                                                                     ("int32_t", "first_below"), ("int32_t", "n_below"), ("int32_t", "first_in")]


def test_header_binding_host_layer_and_library_have_the_six_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gie.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    if not os.path.exists(gie.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    lib = C.CDLL(gie.LIB_PATH)
    for n in NAMES:
        assert "gie_" + n in declared and n in _capi.DEVICE_ONLY and n not in _capi.SIGNATURES and n not in _capi.ROUND_API, n
        assert callable(getattr(gie.Mapper, n)) and hasattr(lib, "gie_" + n), n
    assert sorted(d for d in declared if "sdf" in d) == sorted(["gie_read_sdf", "gie_read_sdf_dev", "gie_query_sdf", "gie_query_sdf_dev"] + ["gie_" + n for n in NAMES])
    assert gie.GroundSdfRolloutParam is _capi.GroundSdfRolloutParam and gie.GroundSdfRollout is _capi.GroundSdfRollout
    assert re.search(r"int gie_ground_query_sdf\(gie_mapper \*h, const float \*xy, int n, float \*dist, float \*grad, uint8_t \*flags\);", txt)
    assert re.search(r"int gie_ground_sdf_rollouts\(gie_mapper \*h, const float \*xy, int n, int T, const gie_ground_sdf_rollout_param \*p, gie_ground_sdf_rollout \*out,\s*"
                     r"float \*dist, float \*grad\);", txt)
    assert txt.index("gie_ground_pose_nf1_path_dev") < txt.index("gie_ground_sdf_rollout_param") < txt.index("gie_costmat_compute")
    p = gie.Mapper.ground_sdf_rollout_param(None, 0.25)
    assert (p.margin, p.flags, list(p.reserved)) == (0.25, 0, [0] * 6)
    host = open(os.path.join(ROOT, "gie-mapping_amd", "host", "gie_host.hpp")).read()
    assert re.search(r"bool ground_distance\(const float \*xy, int n, std::vector<float> &dist, std::vector<float> &grad\)", host)
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_hip.hip")).read()
    assert src.index('#include "gie_ground_pose_nf1.inc.h"') < src.index('#include "gie_ground_sdf.inc.h"')

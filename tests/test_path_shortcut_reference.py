"""The numpy statement of path shortcutting (tests/path_ref.py) against a plain loop over los_ref.line, on hand-made cases and on the
pillar scenes whose answers are known; and the presence of the feature in the header, the library and the package.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gie
import los_ref as lr
import path_cases as pc
import path_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVT = (-7, 12, 3)


def _planes(lab, seed=0):
    """(edt, opq) for a label plane: occupied is opaque; edt is any float32 plane (the statement only reads it)"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 9.0, lab.shape).astype(np.float32), lab == 2


def _plain(opq, path, m, pvt, K):
    """the definition, written out: J from los_ref.line for every j of every window.  (indices, forced flags, the J of every leg)"""
    Z, Y, X = opq.shape
    loc = [tuple(int(path[t][k]) - int(pvt[k]) for k in range(3)) for t in range(m)]
    inside = [0 <= x < X and 0 <= y < Y and 0 <= z < Z for x, y, z in loc]

    def clear(a, b):
        return inside[a] and inside[b] and not any(opq[z, y, x] for x, y, z in lr.line(loc[a], loc[b]))
    idx, forced, Js = ([0] if m else []), [], []
    k = 0
    while k < m - 1:
        J = [j for j in range(k + 1, min(k + K, m - 1) + 1) if clear(k, j)]
        Js.append((k, J))
        k = max(J) if J else k + 1
        forced.append(0 if J else 1)
        idx.append(k)
    return idx, forced, Js, loc


def _check_against_plain(edt, opq, buf, lens, pvt, K, max_wp=None):
    n, max_len = buf.shape[:2]
    cap = max_len if max_wp is None else max_wp
    legs = []
    wp, info = pr.shortcut(edt, opq, buf, lens, pvt, K, cap, legs=legs)
    assert wp.dtype.itemsize == 24 and info.dtype.itemsize == 16
    for i in range(n):
        m = min(max(int(lens[i]), 0), max_len)
        idx, forced, Js, loc = _plain(opq, buf[i], m, pvt, K)
        assert info["count"][i] == len(idx) and info["forced"][i] == sum(forced) and info["reserved"][i] == 0
        w = wp[i, :min(len(idx), cap)]
        assert w["index"].tolist() == idx[:cap] and w["forced"].tolist() == ([0] + forced)[:cap] if m else len(w) == 0
        assert np.array_equal(w["xyz"], buf[i, idx[:cap]])
        assert (wp[i, len(idx):].view(np.uint8) == 0).all()
        length = np.float32(0)
        for t, (k, J) in enumerate(Js):
            j = idx[t + 1]
            top = min(k + K, m - 1)
            if forced[t]:
                assert J == [] and j == k + 1                             # forced iff the window has no clear index
                me = np.float32(-1)
            else:
                line = lr.line(loc[k], loc[j])                            # every unforced leg is clear ...
                assert not any(opq[z, y, x] for x, y, z in line) and k < j <= top
                assert not any(jj in J for jj in range(j + 1, top + 1))   # ... and no index above it in the window is
                me = min(edt[z, y, x] for x, y, z in line)
                d = np.array(loc[j]) - np.array(loc[k])
                length = np.float32(length + np.sqrt(np.float32(int((d * d).sum()))))
            if t + 1 < cap:
                assert w["min_edt"][t + 1].tobytes() == np.float32(me).tobytes()
            # the statement's own windows say the same
            assert legs[i][t][0] == k and legs[i][t][1] == top and (k + 1 + np.flatnonzero(legs[i][t][2])).tolist() == J
        assert info["length"][i].tobytes() == length.tobytes()
    return wp, info, legs


def _indices(wp, info, i=0):
    return wp["index"][i, :info["count"][i]].tolist()


# ---- the statement against the plain loop
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_against_a_plain_loop(seed):
    rng = np.random.default_rng(seed)
    size = (24, 20, 9)
    lab = pc.random_boxes_labels(rng, size, 10)
    edt, opq = _planes(lab, seed)
    max_len = 30
    paths = pc.polylines(rng, size, 16, max_len)
    for _ in range(8):                                                    # staircases through whatever is there
        paths.append(pc.staircase(int(rng.integers(5, max_len + 1)), rng.integers(0, 4, 3)))
    buf, lens = pc.pack(paths, max_len, PVT)
    lens[9] = -3
    nforced = nshort = 0
    for K in (1, 3, 8, 100):
        _, info, legs = _check_against_plain(edt, opq, buf, lens, PVT, K)
        nforced += int(info["forced"].sum())
        nshort += int((info["count"] * 2 < np.clip(lens, 0, max_len)).sum())
    assert nforced >= 10 and nshort >= 3, (nforced, nshort)


# ---- hand cases
def test_staircase_in_an_empty_volume():
    lab = np.ones((8, 8, 8), np.int8)
    edt, opq = _planes(lab)
    buf, lens = pc.pack([pc.staircase(12)], 12, PVT)
    for K, want in ((11, [0, 11]), (12, [0, 11]), (4096, [0, 11]), (5, [0, 5, 10, 11]), (1, list(range(12)))):
        wp, info, _ = _check_against_plain(edt, opq, buf, lens, PVT, K)
        assert _indices(wp, info) == want and info["forced"][0] == 0, (K, _indices(wp, info))
        assert (wp["forced"] == 0).all()
    # v_11 - v_0 = (4, 4, 3)
    wp, info = pr.shortcut(edt, opq, buf, lens, PVT, 11, 12)
    assert info["length"][0] == np.sqrt(np.float32(41)) and np.array_equal(wp["xyz"][0, 1], buf[0, 11])


def _pillar(long):
    size, lab, path = pc.pillar_scene(long)
    edt, opq = _planes(lab)
    buf, lens = pc.pack([path], len(path), PVT)
    return opq, edt, buf, lens, path


def test_pillar_scene_308_points():
    opq, edt, buf, lens, path = _pillar(True)
    assert len(path) == 308
    blocked = [j for j in range(1, 308) if any(opq[z, y, x] for x, y, z in lr.line(path[0], path[j]))]
    assert blocked == list(range(43, 55)) + list(range(114, 308))
    for K, below in ((200, 87), (250, 137), (280, 167), (5000, 194)):
        legs = []
        wp, info = pr.shortcut(edt, opq, buf, lens, PVT, K, 308, legs=legs)
        assert _indices(wp, info) == [0, 113, 307] and info["forced"][0] == 0, (K, _indices(wp, info))
        k, top, clear = legs[0][0]
        assert (k, top) == (0, min(K, 307)) and top - 113 == below
        assert pc.answer_chunks(legs)[0] == (below // 64, True)           # the second, third, third and fourth chunk; a gap below
    assert [b // 64 for b in (87, 137, 167, 194)] == [1, 2, 2, 3]
    _check_against_plain(edt, opq, buf, lens, PVT, 250)


def test_pillar_scene_138_points():
    opq, edt, buf, lens, path = _pillar(False)
    assert len(path) == 138
    for K, want in ((47, [0, 42, 89, 136, 137]), (64, [0, 64, 128, 137]), (127, [0, 113, 137]), (137, [0, 113, 137]), (4096, [0, 113, 137])):
        wp, info, _ = _check_against_plain(edt, opq, buf, lens, PVT, K)
        assert _indices(wp, info) == want and info["forced"][0] == 0, (K, _indices(wp, info))


# ---- other cases
def test_repeats_outside_points_and_short_paths():
    lab = np.ones((6, 10, 12), np.int8)
    lab[:, :, 6] = 2                                                      # a wall across x = 6
    edt, opq = _planes(lab)
    a = [(1, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (3, 1, 1), (3, 2, 1)]                    # a repeated point
    b = [(1, 1, 1), (2, 1, 1), (2, -1, 1), (3, 1, 1), (12, 1, 1), (4, 1, 1), (4, 2, 1)]       # points outside the volume
    c = [(4, 4, 4), (5, 4, 4), (6, 4, 4), (7, 4, 4), (8, 4, 4)]                                # through the wall
    d = [(6, 1, 1), (5, 1, 1), (4, 1, 1)]                                                      # an opaque v_0
    e = [(6, y, 2) for y in range(8)]                                                          # wholly in opaque voxels
    paths = [a, b, c, d, e, [], [(3, 3, 3)], [(3, 3, 3), (9, 8, 5)], [(3, 3, 3), (3, 3, 3)]]
    buf, lens = pc.pack(paths, 8, PVT)
    wp, info, _ = _check_against_plain(edt, opq, buf, lens, PVT, 100)
    assert _indices(wp, info, 0) == [0, 5]
    assert _indices(wp, info, 1) == [0, 6] and info["forced"][1] == 0                        # (the points outside are skipped ...
    wp1, info1, _ = _check_against_plain(edt, opq, buf, lens, PVT, 1)                         # ... unless the window ends on them)
    assert _indices(wp1, info1, 1) == [0, 1, 2, 3, 4, 5, 6] and wp1["forced"][1, :7].tolist() == [0, 0, 1, 1, 1, 1, 0]
    assert wp1["min_edt"][1, 2] == -1 and np.array_equal(wp1["xyz"][1, 4], np.array((12, 1, 1)) + PVT)
    assert _indices(wp, info, 2) == [0, 1, 2, 3, 4] and wp["forced"][2, :5].tolist() == [0, 0, 1, 1, 0]
    assert _indices(wp, info, 3) == [0, 1, 2] and wp["forced"][3, :3].tolist() == [0, 1, 0] and wp["min_edt"][3, 0] == edt[1, 1, 6]
    assert info["count"][4] == 8 and info["forced"][4] == 7 and info["length"][4] == 0 and (wp["min_edt"][4, 1:8] == -1).all()
    assert info["count"][5:].tolist() == [0, 1, 2, 2] and info["forced"][5:].tolist() == [0, 0, 1, 0]    # (3,3,3)-(9,8,5) crosses the wall
    assert info["length"][8] == 0 and wp["min_edt"][8, 1] == edt[3, 3, 3]
    # a first point outside the volume
    buf2, lens2 = pc.pack([[(-1, 0, 0), (0, 0, 0), (1, 0, 0)]], 4, PVT)
    wp2, info2, _ = _check_against_plain(edt, opq, buf2, lens2, PVT, 5)
    assert _indices(wp2, info2) == [0, 1, 2] and wp2["min_edt"][0, 0] == -1 and wp2["forced"][0, :3].tolist() == [0, 1, 0]


def test_lengths_beyond_the_buffer_and_below_zero():
    lab = np.ones((8, 8, 8), np.int8)
    edt, opq = _planes(lab)
    buf, lens = pc.pack([pc.staircase(12)] * 3, 9, PVT)                   # len 12 > max_len 9: the first 9 points
    assert lens.tolist() == [12, 12, 12]
    lens[1], lens[2] = -5, 9
    wp, info, _ = _check_against_plain(edt, opq, buf, lens, PVT, 100)
    assert _indices(wp, info, 0) == [0, 8] == _indices(wp, info, 2) and info["count"][1] == 0
    assert wp[0].tobytes() == wp[2].tobytes() and info[0] == info[2]


def test_capacity_leaves_the_rest_alone():
    opq, edt, buf, lens, path = _pillar(False)
    full, finfo = pr.shortcut(edt, opq, buf, lens, PVT, 47, 8)
    count = int(finfo["count"][0])
    assert count == 5
    for cap in (0, 1, count - 1, count, 8):
        init = np.frombuffer(bytes([0x5a]) * (24 * cap), pr.WAYPOINT_DTYPE).reshape(1, cap)
        wp, info = pr.shortcut(edt, opq, buf, lens, PVT, 47, cap, wp_init=init)
        assert info.tobytes() == finfo.tobytes()                          # info is complete whatever the capacity
        k = min(cap, count)
        assert wp[0, :k].tobytes() == full[0, :k].tobytes() and (wp[0, k:].view(np.uint8) == 0x5a).all()
        _check_against_plain(edt, opq, buf, lens, PVT, 47, max_wp=cap)


# ---- the feature is there (fails without it)
def test_the_feature_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))
    assert {"gie_path_shortcut", "gie_path_shortcut_dev"} <= declared
    for name in ("gie_shortcut_param", "gie_waypoint", "gie_shortcut_info"):
        assert re.search(r"typedef struct %s\b" % name, txt), name
    if not os.path.exists(gie.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    lib = C.CDLL(gie.LIB_PATH)
    assert hasattr(lib, "gie_path_shortcut") and hasattr(lib, "gie_path_shortcut_dev")
    assert callable(getattr(gie.Mapper, "path_shortcut", None)) and callable(getattr(gie.Mapper, "path_shortcut_dev", None))
    assert gie.WAYPOINT_DTYPE.itemsize == 24 and gie.SHORTCUT_INFO_DTYPE.itemsize == 16
    assert gie.WAYPOINT_DTYPE == pr.WAYPOINT_DTYPE and gie.SHORTCUT_INFO_DTYPE == pr.INFO_DTYPE
    assert C.sizeof(gie.Waypoint) == 24 and C.sizeof(gie.ShortcutInfo) == 16 and C.sizeof(gie.ShortcutParam) == 16

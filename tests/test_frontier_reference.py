"""The numpy / scipy statement of the frontier clusters (tests/frontier_ref.py) against a plain Python flood fill on small random
masks and on hand-made cases, and the presence of the feature in every layer that can be checked without a device: the header,
the two libraries' exports, the ctypes record and the Python methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frontier_ref as fr
import gie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gie_frontier_compute", "gie_frontier_compute_dev", "gie_read_frontier_clusters", "gie_read_frontier_clusters_dev",
                "gie_read_frontier_labels", "gie_read_frontier_labels_dev")


def _by_hand(mask, connectivity, min_size, max_clusters, pvt, w):
    """the statement again from the flood fill's member lists, in plain Python integers"""
    Z, Y, X = mask.shape
    comps = fr.flood_fill(mask, connectivity)
    labels = np.full(mask.size, -1, np.int32)
    recs = []
    for lab in sorted(comps):
        mem = comps[lab]
        if len(mem) < min_size:
            labels[mem] = -2
            continue
        labels[mem] = lab
        xyz = [(i % X, (i // X) % Y, i // (X * Y)) for i in mem]
        sz = len(mem)
        sm = [sum(v[k] for v in xyz) for k in range(3)]
        c = [(2 * sm[k] + sz) // (2 * sz) for k in range(3)]
        rep = min(range(sz), key=lambda j: (sum((xyz[j][k] - c[k]) ** 2 for k in range(3)), mem[j]))
        recs.append(dict(label=lab, size=sz, sum=sm, lo=[min(v[k] for v in xyz) + pvt[k] for k in range(3)],
                         hi=[max(v[k] for v in xyz) + pvt[k] for k in range(3)], rep=[xyz[rep][k] + pvt[k] for k in range(3)],
                         centroid=[(np.float32(sm[k] / sz) + np.float32(pvt[k])) * np.float32(w) for k in range(3)]))
    return labels.reshape(mask.shape), recs


def _compare(mask, connectivity, min_size, max_clusters, pvt=(0, 0, 0), w=1.0):
    got = fr.clusters(mask, connectivity, min_size, max_clusters, pvt, w)
    labels, recs = _by_hand(mask, connectivity, min_size, max_clusters, pvt, w)
    assert np.array_equal(got["labels"], labels)
    assert got["n_clusters"] == len(recs) and got["n_voxels"] == sum(r["size"] for r in recs)
    assert len(got["records"]) == min(len(recs), max_clusters) and got["goals"].shape == (max_clusters, 3)
    for q, r in zip(got["records"], recs):
        for k in ("label", "size"):
            assert int(q[k]) == r[k], k
        for k in ("sum", "lo", "hi", "rep"):
            assert q[k].tolist() == r[k], k
        assert q["centroid"].view(np.uint32).tolist() == np.array(r["centroid"], np.float32).view(np.uint32).tolist()
    n = len(got["records"])
    assert np.array_equal(got["goals"][:n], got["records"]["rep"].astype(np.float32) * np.float32(w))
    assert np.isnan(got["goals"][n:]).all()
    return got


def test_reference_against_flood_fill_on_random_masks():
    rng = np.random.default_rng(10)
    sizes = [(1, 7, 9), (5, 9, 1), (7, 1, 5), (3, 5, 7), (5, 5, 5), (9, 7, 3), (1, 1, 11), (7, 3, 5)]      # [Z][Y][X]
    dens = (0.02, 0.08, 0.2, 0.35, 0.5, 0.7, 0.9)
    n = 0
    for i in range(112):
        shape = sizes[i % len(sizes)]
        mask = rng.random(shape) < dens[i % len(dens)]
        for conn in (6, 26):
            _compare(mask, conn, int(rng.integers(1, 5)), int(rng.integers(0, 7)), tuple(rng.integers(-40, 40, 3)), (0.1, 0.05, 0.25)[i % 3])
            n += 1
    assert n >= 200


def test_corner_contact_is_one_component_at_26_and_two_at_6():
    mask = np.zeros((4, 4, 4), bool)
    mask[1, 1, 1] = mask[2, 2, 2] = True
    a = _compare(mask, 26, 1, 8)
    b = _compare(mask, 6, 1, 8)
    assert a["n_clusters"] == 1 and a["records"]["size"].tolist() == [2] and a["records"]["label"].tolist() == [21]
    assert b["n_clusters"] == 2 and b["records"]["label"].tolist() == [21, 42]


def test_component_that_closes_around_a_tile_border():
    """a ring in the x-y plane around the corner where the 64-voxel words and the 8-row tiles meet, and a second ring through z"""
    mask = np.zeros((18, 20, 132), bool)
    mask[3, 5:12, 60] = mask[3, 5:12, 69] = True
    mask[3, 5, 60:70] = mask[3, 11, 60:70] = True
    mask[5:12, 15, 126] = mask[5:12, 15, 130] = True
    mask[5, 15, 126:131] = mask[11, 15, 126:131] = True
    for conn in (6, 26):
        got = _compare(mask, conn, 1, 8)
        assert got["n_clusters"] == 2
        assert got["records"]["size"].tolist() == [30, 20]
        ring = got["labels"][3][got["labels"][3] >= 0]
        assert (ring == (3 * 20 + 5) * 132 + 60).all()


def test_min_size_exactly_at_a_size():
    mask = np.zeros((1, 3, 12), bool)
    mask[0, 0, 0:3] = True          # size 3
    mask[0, 2, 0:4] = True          # size 4
    mask[0, 0, 8] = True            # size 1
    assert _compare(mask, 26, 3, 8)["records"]["size"].tolist() == [3, 4]
    got = _compare(mask, 26, 4, 8)
    assert got["records"]["size"].tolist() == [4] and got["n_voxels"] == 4
    assert sorted(set(got["labels"].ravel().tolist())) == [-2, -1, 24]
    assert _compare(mask, 26, 5, 8)["n_clusters"] == 0


def test_capacity_zero_and_below_the_kept_count():
    rng = np.random.default_rng(3)
    mask = rng.random((5, 7, 9)) < 0.15
    full = _compare(mask, 6, 1, 64)
    assert full["n_clusters"] >= 6
    for cap in (0, 1, full["n_clusters"] - 1, full["n_clusters"], full["n_clusters"] + 5):
        got = _compare(mask, 6, 1, cap)
        assert got["n_clusters"] == full["n_clusters"] and got["n_voxels"] == full["n_voxels"]
        assert np.array_equal(got["labels"], full["labels"])
        n = min(cap, full["n_clusters"])
        assert got["records"].tobytes() == full["records"][:n].tobytes()
    with pytest.raises(ValueError):
        fr.clusters(mask, 6, 0, 4)
    with pytest.raises(ValueError):
        fr.clusters(mask, 6, 1, -1)
    with pytest.raises(ValueError):
        fr.clusters(mask, 18, 1, 4)


def test_tie_for_rep_goes_to_the_smaller_index():
    mask = np.zeros((1, 3, 3), bool)
    mask[0, 0, 1] = mask[0, 1, 0] = mask[0, 1, 2] = mask[0, 2, 1] = True       # a diamond around the empty centre (1, 1, 0)
    got = _compare(mask, 26, 1, 4, pvt=(10, 20, 30), w=0.5)
    q = got["records"][0]
    assert q["sum"].tolist() == [4, 4, 0] and q["rep"].tolist() == [11, 20, 30] and q["label"] == 1
    assert q["centroid"].tolist() == [5.5, 10.5, 15.0]
    two = np.zeros((1, 1, 4), bool)
    two[0, 0, 1] = two[0, 0, 2] = True                                          # centroid 1.5 rounds half up to 2
    assert _compare(two, 6, 1, 4)["records"]["rep"].tolist() == [[2, 0, 0]]


def test_members_follow_nf1s_clearance_rule():
    T = np.array([[[0, 3, 3, 3, 1, 2, 3]]], np.int8)
    edt = np.array([[[0, 1, 1.5, 2, 3, 0, np.float32(1.4999999)]]], np.float32)
    assert fr.members(T, edt, 1.5).tolist() == [[[False, False, True, True, False, False, False]]]
    assert fr.members(T, edt, 0.0).tolist() == [[[False, True, True, True, False, False, True]]]


def _declared():
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))


def test_every_layer_has_the_feature():
    import __graft_entry__
    declared = _declared()
    assert set(ENTRY_POINTS) <= declared
    if not os.path.exists(gie.LIB_PATH):
        __graft_entry__.build_hip()
    for path in (gie.LIB_PATH, __graft_entry__.build_hip_test_hooks()):
        lib = C.CDLL(path)
        assert [n for n in ENTRY_POINTS if not hasattr(lib, n)] == [], path
    from gie._capi import DEVICE_ONLY, FrontierCluster, FrontierParam
    assert C.sizeof(FrontierCluster) == 80 and FrontierCluster.sum.offset == 56 and FrontierCluster.rep.offset == 32
    assert FrontierCluster.centroid.offset == 44 and FrontierCluster.lo.offset == 8 and FrontierCluster.hi.offset == 20
    assert C.sizeof(FrontierParam) == 24 and FrontierParam.max_clusters.offset == 12
    assert gie.FRONTIER_CLUSTER_DTYPE == fr.CLUSTER_DTYPE
    for n in ENTRY_POINTS:
        assert n[4:] in DEVICE_ONLY
    for n in ("frontier_compute", "frontier_compute_dev", "read_frontier_clusters", "read_frontier_clusters_dev", "read_frontier_labels",
              "read_frontier_labels_dev"):
        assert callable(getattr(gie.Mapper, n))
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    assert "You may need to do some post-process" in txt and "typedef struct gie_frontier_cluster" in txt

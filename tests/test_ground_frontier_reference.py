"""The numpy / scipy statement of the ground frontier clusters (tests/ground_frontier_ref.py) against a plain Python flood fill on
small random masks and on hand-made cases, and the presence of the feature in every layer that can be checked without a device: the
header, the ctypes records, the binding's tables and the Python methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ground_frontier_ref as F
import ground_nf1_ref as N
import ground_ref as G
import gie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gie_ground_frontier_compute", "gie_ground_frontier_compute_dev", "gie_read_ground_frontier_clusters",
                "gie_read_ground_frontier_clusters_dev", "gie_read_ground_frontier_labels", "gie_read_ground_frontier_labels_dev",
                "gie_ground_nf1_query", "gie_ground_nf1_query_dev")
CLEARANCES = (0, 1, 2, 4, 5, 9)


def _by_hand(mask, dist, connectivity, min_size, pvt, w):
    """the statement again from the flood fill's member lists, in plain Python integers"""
    Y, X = mask.shape
    comps = F.flood_fill(mask, connectivity)
    labels = np.full(mask.size, -1, np.int32)
    recs = []
    for lab in sorted(comps):
        mem = comps[lab]
        if len(mem) < min_size:
            labels[mem] = -2
            continue
        labels[mem] = lab
        xy = [(i % X, i // X) for i in mem]
        sz = len(mem)
        sm = [sum(v[k] for v in xy) for k in range(2)]
        c = [(2 * sm[k] + sz) // (2 * sz) for k in range(2)]
        rep = min(range(sz), key=lambda j: (sum((xy[j][k] - c[k]) ** 2 for k in range(2)), mem[j]))
        recs.append(dict(label=lab, size=sz, sum=sm, lo=[min(v[k] for v in xy) + pvt[k] for k in range(2)],
                         hi=[max(v[k] for v in xy) + pvt[k] for k in range(2)], rep=[xy[rep][k] + pvt[k] for k in range(2)],
                         rep_dist_sq=int(dist[xy[rep][1], xy[rep][0]]),
                         centroid=[(np.float32(sm[k] / sz) + np.float32(pvt[k])) * np.float32(w) for k in range(2)]))
    return labels.reshape(mask.shape), recs


def _compare(mask, connectivity, min_size, max_clusters, pvt=(0, 0), w=1.0, dist=None):
    mask = np.asarray(mask, bool)
    dist = np.full(mask.shape, -1, np.int32) if dist is None else dist
    got = F.clusters_of_mask(mask, dist, connectivity, min_size, max_clusters, pvt, w)
    labels, recs = _by_hand(mask, dist, connectivity, min_size, pvt, w)
    assert np.array_equal(got["labels"], labels)
    assert got["n_clusters"] == len(recs) and got["n_cells"] == sum(r["size"] for r in recs)
    assert len(got["records"]) == min(len(recs), max_clusters) and got["goals"].shape == (max_clusters, 2)
    for q, r in zip(got["records"], recs):
        for k in ("label", "size", "rep_dist_sq"):
            assert int(q[k]) == r[k], k
        for k in ("sum", "lo", "hi", "rep"):
            assert q[k].tolist() == r[k], k
        assert q["centroid"].view(np.uint32).tolist() == np.array(r["centroid"], np.float32).view(np.uint32).tolist()
        assert q["reserved"] == 0
    n = len(got["records"])
    assert np.array_equal(got["goals"][:n], got["records"]["rep"].astype(np.float32) * np.float32(w))
    assert np.isnan(got["goals"][n:]).all()
    return got


def test_reference_against_flood_fill_on_random_masks():
    rng = np.random.default_rng(22)
    sizes = [(7, 9), (9, 1), (1, 5), (5, 7), (5, 5), (7, 3), (1, 11), (3, 5), (1, 1), (11, 13)]      # [Y][X]
    dens = (0.02, 0.08, 0.2, 0.35, 0.5, 0.7, 0.9)
    n = 0
    for i in range(140):
        shape = sizes[i % len(sizes)]
        mask = rng.random(shape) < dens[i % len(dens)]
        dist = rng.integers(-1, 30, shape).astype(np.int32)
        for conn in (4, 8):
            _compare(mask, conn, int(rng.integers(1, 5)), int(rng.integers(0, 7)), tuple(rng.integers(-40, 40, 2)), (0.1, 0.05, 0.25)[i % 3], dist)
            n += 1
    assert n >= 280


def test_four_cells_around_a_hole_are_one_component_at_8_and_four_at_4():
    mask = np.zeros((5, 5), bool)
    mask[1, 2] = mask[2, 1] = mask[2, 3] = mask[3, 2] = True
    a = _compare(mask, 8, 1, 8)
    b = _compare(mask, 4, 1, 8)
    assert a["n_clusters"] == 1 and a["records"]["size"].tolist() == [4] and a["records"]["label"].tolist() == [7]
    assert b["n_clusters"] == 4 and b["records"]["label"].tolist() == [7, 11, 13, 17] and b["records"]["size"].tolist() == [1] * 4


def test_rings_across_the_word_boundary():
    """a ring around x = 63 / 64, a second one whose left side IS column 63 and a third whose left side is column 64"""
    mask = np.zeros((30, 132), bool)
    mask[2:9, 60] = mask[2:9, 69] = True
    mask[2, 60:70] = mask[8, 60:70] = True
    mask[12:17, 63] = mask[12:17, 66] = True
    mask[12, 63:67] = mask[16, 63:67] = True
    mask[20:25, 64] = mask[20:25, 127] = True
    mask[20, 64:128] = mask[24, 64:128] = True
    for conn in (4, 8):
        got = _compare(mask, conn, 1, 8)
        assert got["n_clusters"] == 3
        assert got["records"]["size"].tolist() == [30, 14, 134]
        assert got["records"]["label"].tolist() == [2 * 132 + 60, 12 * 132 + 63, 20 * 132 + 64]
        assert (got["labels"][2:9][got["labels"][2:9] >= 0] == 2 * 132 + 60).all()


def test_min_size_exactly_at_a_size():
    mask = np.zeros((3, 12), bool)
    mask[0, 0:3] = True             # size 3
    mask[2, 0:4] = True             # size 4
    mask[0, 8] = True               # size 1
    assert _compare(mask, 8, 3, 8)["records"]["size"].tolist() == [3, 4]
    got = _compare(mask, 8, 4, 8)
    assert got["records"]["size"].tolist() == [4] and got["n_cells"] == 4
    assert sorted(set(got["labels"].ravel().tolist())) == [-2, -1, 24]
    assert _compare(mask, 8, 5, 8)["n_clusters"] == 0


def test_capacities_from_zero_to_beyond_the_kept_count():
    rng = np.random.default_rng(3)
    mask = rng.random((9, 13)) < 0.2
    full = _compare(mask, 4, 1, 64)
    kept = full["n_clusters"]
    assert kept >= 6
    for cap in range(0, kept + 6):
        got = _compare(mask, 4, 1, cap)
        assert got["n_clusters"] == kept and got["n_cells"] == full["n_cells"]
        assert np.array_equal(got["labels"], full["labels"])
        assert got["records"].tobytes() == full["records"][:min(cap, kept)].tobytes()
    dist = np.zeros(mask.shape, np.int32)
    for bad in ((mask, dist, 4, 0, 4), (mask, dist, 4, 1, -1), (mask, dist, 6, 1, 4), (mask, dist, 26, 1, 4)):
        with pytest.raises(ValueError):
            F.clusters_of_mask(*bad)


def test_tie_for_rep_goes_to_the_smaller_index():
    mask = np.zeros((3, 3), bool)
    mask[0, 1] = mask[1, 0] = mask[1, 2] = mask[2, 1] = True       # a diamond around the empty centre (1, 1)
    dist = np.arange(9, dtype=np.int32).reshape(3, 3) + 10
    got = _compare(mask, 8, 1, 4, pvt=(10, 20), w=0.5, dist=dist)
    q = got["records"][0]
    assert q["sum"].tolist() == [4, 4] and q["rep"].tolist() == [11, 20] and q["label"] == 1 and q["rep_dist_sq"] == 11
    assert q["centroid"].tolist() == [5.5, 10.5]
    two = np.zeros((1, 4), bool)
    two[0, 1] = two[0, 2] = True                                    # centroid 1.5 rounds half up to 2
    assert _compare(two, 4, 1, 4)["records"]["rep"].tolist() == [[2, 0]]


def test_members_follow_ground_nf1s_clearance_rule():
    T = np.array([[0, 3, 3, 3, 1, 2, 3, 3, 3]], np.int8)
    D = np.array([[0, 0, 1, 2, 9, 0, 4, 5, 9]], np.int32)
    for csq in CLEARANCES:
        f = {"type": T, "dist_sq": D}
        want = [[t == 3 and d >= csq for t, d in zip(T[0], D[0])]]
        assert F.members(f, csq).tolist() == want
        assert np.array_equal(F.members(f, csq), N.traversable(f, csq) & (T == G.FNT))
        none = {"type": T, "dist_sq": np.full(T.shape, -1, np.int32)}            # no obstacle column: every clearance passes
        assert F.members(none, csq).tolist() == [[t == 3 for t in T[0]]]
    assert F.members({"type": T, "dist_sq": np.full(T.shape, -1, np.int32)}, 2 ** 31 - 1).sum() == 6
    with pytest.raises(ValueError):
        F.clusters({"type": T, "dist_sq": D}, -1)
    got = F.clusters({"type": T, "dist_sq": D}, 4, 4, 1, 4)
    assert got["records"]["size"].tolist() == [3] and got["records"]["rep_dist_sq"].tolist() == [5]


def test_gather_and_route_steps():
    T = np.ones((5, 7), np.int8)
    T[:, 3] = 2
    T[4, 3] = 1                                                  # a wall with a gap at the far end
    T[0, 6] = 3
    f = G.field(T[None], (0, 0, 0), 0, 0)
    pvt, w = (4, -3), 0.1
    xy = lambda cells: ((np.asarray(cells, np.float64) + np.array(pvt)).astype(np.float32) * np.float32(w)).astype(np.float32)      # noqa: E731
    goals = np.concatenate([xy([(6, 0), (0, 0), (3, 0), (-1, 0), (7, 4)]), np.array([[np.nan, 0.0], [np.inf, 1.0]], np.float32)])
    steps = F.route_steps(f, xy([(0, 0)]), goals, pvt, w)
    assert steps.tolist() == [4 + 6 + 4, 0, -1, -1, -1, -1, -1]
    assert (F.route_steps(f, xy([(3, 1)]), goals, pvt, w) == -1).all()          # the robot in an obstacle column: no source
    assert F.gather(np.zeros((5, 7), np.int32), np.zeros((0, 2), np.float32), pvt, w).shape == (0,)


def _declared():
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gie_[a-z0-9_]+)\s*\(", txt))


def test_every_layer_has_the_feature():
    assert set(ENTRY_POINTS) <= _declared()
    from gie._capi import DEVICE_ONLY, SIGNATURES, GroundFrontierCluster, GroundFrontierParam
    assert C.sizeof(GroundFrontierCluster) == 64 and GroundFrontierCluster.sum.offset == 40 and GroundFrontierCluster.rep.offset == 24
    assert GroundFrontierCluster.centroid.offset == 32 and GroundFrontierCluster.rep_dist_sq.offset == 56
    assert C.sizeof(GroundFrontierParam) == 32 and GroundFrontierParam.max_clusters.offset == 12 and GroundFrontierParam.flags.offset == 16
    assert gie.GROUND_FRONTIER_CLUSTER_DTYPE == F.CLUSTER_DTYPE
    for n in ENTRY_POINTS:
        assert n[4:] in DEVICE_ONLY and n[4:] not in SIGNATURES
    for n in ("ground_frontier_param", "ground_frontier_compute", "ground_frontier_compute_dev", "read_ground_frontier_clusters",
              "read_ground_frontier_clusters_dev", "read_ground_frontier_labels", "read_ground_frontier_labels_dev", "ground_nf1_query",
              "ground_nf1_query_dev"):
        assert callable(getattr(gie.Mapper, n))
    p = gie.Mapper.ground_frontier_param(None, 4, 3, 4, 17)
    assert (p.clearance_sq, p.min_size, p.connectivity, p.max_clusters, p.flags, list(p.reserved)) == (4, 3, 4, 17, 0, [0, 0, 0])
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    assert "typedef struct gie_ground_frontier_cluster" in txt and txt.index("---- ground line of sight") < txt.index("---- ground frontier clusters")

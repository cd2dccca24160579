"""The numpy reference of the global block routes (tests/routes_ref.py) against a literal per-voxel, per-block loop on hand-made
tables, the host layer's goal order, and the binding's structs against the header.  No device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import blocks_ref as B
import gie
import routes_ref as R
from gie import _capi
from test_blocks_reference import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.1
VLO, VHI = (-24, -16, -8), (16, 8, 8)                            # blocks x -3..1, y -2..0, z -1..0
BLO, BHI = (-3, -2, -1), (1, 0, 0)
E = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


class World:
    """a dictionary of global voxels (UNKNOWN where absent) inside the box [VLO, VHI)"""

    def __init__(self):
        self.vox = {}

    def fill(self, block, ty):
        for x in range(8):
            for y in range(8):
                for z in range(8):
                    self.vox[(block[0] * 8 + x, block[1] * 8 + y, block[2] * 8 + z)] = ty
        return self

    def set(self, block, v, ty):
        self.vox[tuple(block[k] * 8 + v[k] for k in range(3))] = ty
        return self

    def table(self):
        xyz = B.box_coords(VLO, VHI)
        ty = np.array([self.vox.get(tuple(g), R.UNKNOWN) for g in xyz.tolist()], np.int8)
        return B.block_table(ty, np.zeros(len(xyz), np.int32), VLO, VHI)


def centre(block):
    """a world point inside the block"""
    return tuple(np.float32((block[k] * 8 + 3) * W) for k in range(3))


def literal(vox, lo, hi, min_free, min_open, min_fnt, goals, flags, starts=(), max_len=1, fill=0):
    """include/gie.h word for word: dictionaries of blocks, Bellman-Ford relaxation for the steps"""
    def passable(g):
        return vox.get(g, R.UNKNOWN) in (R.FREE, R.FNT)

    def voxels(k):
        return [(k[0] * 8 + x, k[1] * 8 + y, k[2] * 8 + z) for x in range(8) for y in range(8) for z in range(8)]

    def block_of(p):
        k = []
        for v in p:
            u = np.float32(v) / np.float32(W) + np.float32(0.5)
            if not math.isfinite(u):
                return None
            k.append(int(math.floor(u)) >> 3)
        return tuple(k)
    box = [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)]      # x fastest
    inbox = set(box)
    node = {k: sum(passable(g) for g in voxels(k)) >= min_free for k in box}
    pairs, link = {}, {}
    for k in box:
        for a in range(3):
            n = 0
            for g in voxels(k):
                if (g[a] & 7) == 7:
                    h = tuple(g[i] + E[a][i] for i in range(3))
                    n += passable(g) and passable(h)
            pairs[k, a] = n
            kk = tuple(k[i] + E[a][i] for i in range(3))
            link[k, a] = node[k] and kk in inbox and node[kk] and n >= min_open
    frontier = {k: node[k] and sum(vox.get(g, 0) == R.FNT for g in voxels(k)) >= min_fnt for k in box}
    source = {k: bool(flags & R.FROM_FRONTIERS) and frontier[k] for k in box}
    for p in goals:
        k = block_of(p)
        if k is not None and k in inbox and node[k]:
            source[k] = True

    def joined(k):                                               # in the descent's order
        out = []
        for a in range(3):
            m = tuple(k[i] - E[a][i] for i in range(3))
            if m in inbox and link[m, a]:
                out.append(m)
            if link[k, a]:
                out.append(tuple(k[i] + E[a][i] for i in range(3)))
        return out
    big = 10 ** 9
    steps = {k: 0 if source[k] else big for k in box}
    changed = True
    while changed:
        changed = False
        for k in box:
            for m in joined(k):
                if steps[m] + 1 < steps[k]:
                    steps[k], changed = steps[m] + 1, True
    steps = {k: (-1 if v == big else v) for k, v in steps.items()}
    cells = [(1 | link[k, 0] * 2 | link[k, 1] * 4 | link[k, 2] * 8 | frontier[k] * 16 | source[k] * 32) if node[k] else 0 for k in box]
    info = (sum(node.values()), sum(link.values()), sum(frontier.values()), sum(source.values()), sum(v >= 0 for v in steps.values()),
            max(steps.values()), 0, 0)
    path = np.full((len(starts), max_len, 3), fill, np.int32)
    ln = []
    for i, p in enumerate(starts):
        k = block_of(p)
        s = steps[k] if k is not None and k in inbox else -1
        ln.append(s + 1)
        j = 0
        while s >= 0 and j < max_len:
            path[i, j] = k
            j += 1
            if s == 0:
                break
            k = [m for m in joined(k) if steps[m] == s - 1][0]
            s -= 1
    return dict(node=node, pairs=pairs, link=link, frontier=frontier, source=source, steps=steps, cells=cells, info=info, path=path, len=ln, box=box,
                query=lambda pts: [steps[block_of(p)] if block_of(p) in inbox else -1 for p in pts])


def both(world, lo=BLO, hi=BHI, min_free=1, min_open=1, min_fnt=1, goals=(), flags=0, starts=(), max_len=4, probes=()):
    """the reference and the literal loop on one world, compared plane by plane -> (reference graph, literal result)"""
    g = R.Graph(world.table(), lo, hi, min_free, min_open, min_fnt)
    gb, ok = R.point_blocks(np.asarray(goals, np.float32).reshape(-1, 3), W)
    g.solve(gb, ok, flags)
    lit = literal(world.vox, lo, hi, min_free, min_open, min_fnt, goals, flags, starts, max_len, fill=-7)
    box = lit["box"]
    assert g.node.ravel().tolist() == [lit["node"][k] for k in box]
    assert g.frontier.ravel().tolist() == [lit["frontier"][k] for k in box]
    assert g.source.ravel().tolist() == [lit["source"][k] for k in box]
    for a in range(3):
        assert g.link[a].ravel().tolist() == [lit["link"][k, a] for k in box], a
        kept = [(int(p), lit["pairs"][k, a]) for p, k in zip(g.pairs[a].ravel(), box) if k[a] < hi[a]]      # (the reference keeps no pairs towards outside the box)
        assert all(p == q for p, q in kept), a
    assert g.steps.ravel().tolist() == [lit["steps"][k] for k in box]
    assert g.cells.dtype == np.uint8 and g.cells.ravel().tolist() == lit["cells"]
    assert g.steps.dtype == np.int32 and g.steps.shape == (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    assert tuple(int(v) for v in g.info.tolist()[:6]) + (0, 0) == lit["info"]
    if len(starts):
        path, ln = g.path(starts, W, max_len, fill=-7)
        assert ln.tolist() == lit["len"] and np.array_equal(path, lit["path"])
    if len(probes):
        assert g.query(probes, W).tolist() == lit["query"](probes)
    return g, lit


def cell(g, k):
    return tuple(int(k[2 - i] - g.lo[2 - i]) for i in range(3))   # (z, y, x) index of block k


# ---------------------------------------------------------------------------------------------------------- pairs and min_open
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_open_pair_in_a_faces_corner(axis):
    a, b = (-1, -1, -1), tuple(-1 + E[axis][i] for i in range(3))    # negative block coordinates: voxel -1 lies in block -1
    w = World().fill(a, R.OCCUPIED).fill(b, R.OCCUPIED)
    w.set(a, (7, 7, 7), R.FREE)
    w.set(b, tuple(0 if i == axis else 7 for i in range(3)), R.FREE)
    assert (a[axis] * 8 + 7) == -1                               # the pair's own voxel is global voxel -1 on that axis
    g, lit = both(w, goals=[centre(a)], starts=[centre(b)], probes=[centre(a), centre(b)])
    assert lit["pairs"][a, axis] == 1 and g.pairs[axis][cell(g, a)] == 1
    assert g.link[axis][cell(g, a)] and g.link.sum() == 1 and g.steps[cell(g, b)] == 1
    g2, _ = both(w, min_open=2, goals=[centre(a)])
    assert g2.link.sum() == 0 and g2.steps[cell(g2, b)] == -1
    # the same two free voxels, not facing each other: no pair
    w.set(b, tuple(0 if i == axis else 7 for i in range(3)), R.OCCUPIED)
    w.set(b, tuple(0 if i == axis else 6 for i in range(3)), R.FREE)
    g3, lit3 = both(w, goals=[centre(a)])
    assert lit3["pairs"][a, axis] == 0 and g3.link.sum() == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_min_open_at_the_count_and_a_fully_open_face(axis):
    a, b = (-2, -1, -1), tuple((-2, -1, -1)[i] + E[axis][i] for i in range(3))
    w = World().fill(a, R.FREE).fill(b, R.FREE)
    g, lit = both(w, min_open=64)
    assert lit["pairs"][a, axis] == 64 and g.link[axis][cell(g, a)]
    rng = np.random.default_rng(axis)
    closed = rng.choice(64, 23, replace=False)                   # 23 of the own face's voxels OCCUPIED: 41 pairs
    for c in closed.tolist():
        v = [c >> 3, c & 7]
        v.insert(axis, 7)
        w.set(a, v, R.OCCUPIED)
    for min_open, linked in ((1, True), (41, True), (42, False), (64, False)):
        g, lit = both(w, min_open=min_open)
        assert lit["pairs"][a, axis] == 41 and bool(g.link[axis][cell(g, a)]) == linked, min_open


def test_pairs_count_fnt_sides_and_no_unknown_or_occupied_side():
    a, b = (0, -1, 0), (1, -1, 0)
    w = World().fill(a, R.OCCUPIED).fill(b, R.OCCUPIED)
    for y, (ta, tb) in enumerate(((R.FREE, R.FNT), (R.FNT, R.FREE), (R.FNT, R.FNT), (R.FREE, R.UNKNOWN), (R.UNKNOWN, R.FREE), (R.FREE, R.OCCUPIED),
                                  (R.OCCUPIED, R.FNT), (R.FREE, R.FREE))):
        w.set(a, (7, y, 2), ta).set(b, (0, y, 2), tb)
    g, lit = both(w)
    assert lit["pairs"][a, 0] == 4 and g.pairs[0][cell(g, a)] == 4
    assert both(w, min_open=4)[0].link.sum() == 1 and both(w, min_open=5)[0].link.sum() == 0


# ---------------------------------------------------------------------------------------------------------- nodes
def test_min_free_at_the_count_and_a_neighbour_that_fails_it():
    a, b = (-1, 0, -1), (0, 0, -1)
    w = World().fill(a, R.FREE).fill(b, R.OCCUPIED)
    for y in range(8):
        for z in range(3):
            w.set(b, (0, y, z), R.FNT if z == 0 else R.FREE)     # 24 passable voxels, 8 of them FNT, 24 pairs
    g, lit = both(w, min_free=24, min_open=24)
    assert g.n_pass[cell(g, b)] == 24 and g.node[cell(g, b)] and g.link[0][cell(g, a)]
    g, lit = both(w, min_free=25, min_open=24)                   # the neighbour fails min_free although the pairs suffice
    assert not g.node[cell(g, b)] and lit["pairs"][a, 0] == 24 and not g.link.any() and g.cells[cell(g, b)] == 0
    assert both(w, min_fnt=8)[0].frontier[cell(g, b)] and not both(w, min_fnt=9)[0].frontier[cell(g, b)]
    assert not both(w, min_free=25, min_fnt=8)[0].frontier.any() # no frontier without a node


def test_a_link_whose_other_end_is_outside_the_box():
    w = World()
    for x in range(-3, 2):
        w.fill((x, -1, 0), R.FREE)
    g, _ = both(w, goals=[centre((-3, -1, 0))])
    assert g.link.sum() == 4 and g.steps[cell(g, (1, -1, 0))] == 4
    g, _ = both(w, lo=(-2, -1, 0), hi=(0, -1, 0), goals=[centre((-3, -1, 0)), centre((0, -1, 0))], probes=[centre((1, -1, 0)), centre((-3, -1, 0)), centre((-2, -1, 0))])
    assert g.link.sum() == 2 and not g.link[0][cell(g, (0, -1, 0))] and g.cells[cell(g, (0, -1, 0))] == R.NODE | R.SOURCE
    assert g.steps.ravel().tolist() == [2, 1, 0] and g.info["n_sources"] == 1


# ---------------------------------------------------------------------------------------------------------- sources and the field
def test_goals_on_a_non_node_outside_the_box_and_not_finite():
    w = World().fill((-1, -1, 0), R.FREE).fill((0, -1, 0), R.FREE).fill((1, -1, 0), R.OCCUPIED)
    nan, inf = float("nan"), float("inf")
    goals = [centre((1, -1, 0)), centre((40, 0, 0)), (nan, 0.0, 0.0), (0.0, -inf, 0.0), (3.0e9, 0.0, 0.0)]
    g, _ = both(w, goals=goals, probes=goals + [centre((0, -1, 0))])
    assert g.info["n_sources"] == 0 and g.info["max_steps"] == -1 and g.info["n_reached"] == 0 and (g.steps == -1).all()
    g, _ = both(w, goals=goals + [centre((0, -1, 0))], probes=goals + [centre((0, -1, 0))], starts=goals + [centre((-1, -1, 0))])
    assert g.info["n_sources"] == 1 and g.info["max_steps"] == 1 and g.info["n_reached"] == 2
    assert g.query(goals, W).tolist() == [-1] * 5


def test_two_sources_at_equal_distance_an_island_and_frontier_sources():
    w = World()
    for x in range(-3, 2):
        w.fill((x, -2, -1), R.FREE)                              # a corridor of five blocks
    w.fill((-3, 0, 0), R.FREE).set((-3, 0, 0), (1, 1, 1), R.FNT) # an island with a FNT voxel
    w.set((1, -2, -1), (3, 3, 3), R.FNT)
    ends = [centre((-3, -2, -1)), centre((1, -2, -1))]
    g, _ = both(w, goals=ends, starts=[centre((-1, -2, -1)), centre((-3, 0, 0))], max_len=5)
    assert g.steps[0, 0].tolist() == [0, 1, 2, 1, 0]             # the middle block is two links from both
    assert g.steps[cell(g, (-3, 0, 0))] == -1 and g.info["n_reached"] == 5 and g.info["n_nodes"] == 6
    path, ln = g.path([centre((-1, -2, -1))], W, 5)
    assert ln[0] == 3 and path[0, :3].tolist() == [[-1, -2, -1], [-2, -2, -1], [-3, -2, -1]]      # -x comes before +x
    g, _ = both(w, flags=R.FROM_FRONTIERS)
    assert g.info["n_sources"] == 2 == g.info["n_frontier"] and g.steps[cell(g, (-3, 0, 0))] == 0 and g.steps[0, 0].tolist() == [4, 3, 2, 1, 0]
    g, _ = both(w, flags=R.FROM_FRONTIERS, min_fnt=2, goals=ends[:1])
    assert g.info["n_frontier"] == 0 and g.steps[0, 0].tolist() == [0, 1, 2, 3, 4]


def test_a_descent_where_the_order_decides_and_max_len():
    w = World()
    for x in (-1, 0, 1):
        for y in (-2, -1, 0):
            for z in (-1, 0):
                w.fill((x, y, z), R.FREE)                        # 3 x 3 x 2 free blocks, the source in a corner
    src, start = (-1, -2, -1), (1, 0, 0)
    for max_len in (1, 2, 5, 6, 7, 9):                           # below, at (steps 5: six blocks) and above the path's length
        g, lit = both(w, lo=(-1, -2, -1), hi=(1, 0, 0), goals=[centre(src)], starts=[centre(start), centre(src), centre((5, 5, 5))], max_len=max_len)
        path, ln = g.path([centre(start)], W, max_len, fill=-7)
        assert ln[0] == 6
        want = [[1, 0, 0], [0, 0, 0], [-1, 0, 0], [-1, -1, 0], [-1, -2, 0], [-1, -2, -1]]      # -x while it descends, then -y, then -z
        n = min(max_len, 6)
        assert path[0, :n].tolist() == want[:n] and (path[0, n:] == -7).all()


# ---------------------------------------------------------------------------------------------------------- the stated approximation
def test_a_wall_inside_a_block_does_not_cut_and_the_same_wall_on_a_face_does():
    blocks = [(-1, -1, 0), (0, -1, 0), (1, -1, 0)]
    w = World()
    for b in blocks:
        w.fill(b, R.FREE)
    for y in range(8):
        for z in range(8):
            w.set((0, -1, 0), (4, y, z), R.OCCUPIED)             # a closed wall through the middle of the middle block
    g, _ = both(w, lo=(-1, -1, 0), hi=(1, -1, 0), goals=[centre(blocks[0])])
    assert g.steps.ravel().tolist() == [0, 1, 2]                 # optimistic: the block is one node, the wall inside it is not seen
    for y in range(8):
        for z in range(8):
            w.set((0, -1, 0), (4, y, z), R.FREE).set((0, -1, 0), (7, y, z), R.OCCUPIED)     # the same wall on the block's +x face
    g, lit = both(w, lo=(-1, -1, 0), hi=(1, -1, 0), goals=[centre(blocks[0])])
    assert g.steps.ravel().tolist() == [0, 1, -1] and lit["pairs"][(0, -1, 0), 0] == 0
    w.set((0, -1, 0), (7, 2, 5), R.FREE)                         # a door of one voxel
    assert both(w, lo=(-1, -1, 0), hi=(1, -1, 0), goals=[centre(blocks[0])])[0].steps.ravel().tolist() == [0, 1, 2]
    assert both(w, lo=(-1, -1, 0), hi=(1, -1, 0), goals=[centre(blocks[0])], min_open=2)[0].steps.ravel().tolist() == [0, 1, -1]


def test_random_worlds():
    rng = np.random.default_rng(5)
    for trial in range(3):
        w = World()
        xyz = B.box_coords(VLO, VHI)
        ty = rng.choice(4, len(xyz), p=(0.25, 0.45, 0.25, 0.05))
        w.vox = {tuple(g): int(t) for g, t in zip(xyz.tolist(), ty.tolist())}
        for k in ((-2, -1, 0), (0, 0, -1)):
            w.fill(k, R.OCCUPIED)
        pts = (rng.uniform(-3.0, 2.0, (12, 3))).astype(np.float32)
        g, _ = both(w, min_free=240 + 8 * trial, min_open=14 + 2 * trial, min_fnt=20, goals=pts[:2], flags=trial & 1, starts=pts, max_len=3, probes=pts)
        assert g.link.any() and not g.link.all()


# ---------------------------------------------------------------------------------------------------------- the host layer's order
def test_goal_order_by_route_steps():
    w = World()
    for x in range(-3, 2):
        w.fill((x, -2, -1), R.FREE)
    w.fill((0, 0, 0), R.FREE)                                    # an island, close to the robot as the crow flies
    rec = np.zeros(3, B.BLOCK_SUMMARY_DTYPE)
    rec["key"] = [(-3, -2, -1), (0, 0, 0), (0, -2, -1)]
    rec["n_fnt"], rec["fnt_voxel"], rec["min_dist_sq"] = [4, 5, 6], [0, 9, 511], [1, 2, 3]
    robot = centre((1, -2, -1))
    old_pos, old_n, _ = B.goals(rec, robot, W, 3)
    assert old_n.tolist() == [6, 5, 4]                           # straight-line order: (0,-2,-1) at 1, the island at 6, (-3,-2,-1) at 16
    pos, keys, n_fnt, dmin, steps = R.route_goals(w.table(), rec, robot, W, 3)
    assert steps.tolist() == [1, 4, -1] and n_fnt.tolist() == [6, 4, 5] and keys.tolist() == [[0, -2, -1], [-3, -2, -1], [0, 0, 0]]
    assert pos.tobytes() == old_pos[[0, 2, 1]].tobytes() and dmin.tolist() == [3, 1, 2]
    lo, hi = R.routes_box(rec["key"], (1, -2, -1))
    assert lo.tolist() == [-4, -3, -2] and hi.tolist() == [2, 1, 1]


def test_the_hosts_box_is_cut_around_the_robot():
    lo, hi = R.routes_box([(-20000, 0, 0), (30, 40, 3)], (0, 0, 0))
    assert R.words(lo, hi) <= R.MAX_WORDS and (lo <= 0).all() and (hi >= 0).all()
    assert lo.tolist() == [-2500, -1, -1] and hi.tolist() == [31, 41, 4]          # h = 20001 -> 10000 -> 5000 -> 2500 fits: 40 * 43 * 6 words
    lo, hi = R.routes_box([(5, 5, 5)], (4, 4, 4))
    assert lo.tolist() == [3, 3, 3] and hi.tolist() == [6, 6, 6]


# ---------------------------------------------------------------------------------------------------------- the structs
@pytest.mark.parametrize("name,ctype,dtype,size", [("gie_routes_param", _capi.RoutesParam, gie.ROUTES_PARAM, 48),
                                                    ("gie_routes_info", _capi.RoutesInfo, gie.ROUTES_INFO, 32)])
def test_binding_structs_match_the_header(name, ctype, dtype, size):
    fields, total = header_struct(name)
    assert total == size == C.sizeof(ctype) == dtype.itemsize
    assert [f[0] for f in fields] == [f[0] for f in ctype._fields_] == list(dtype.names)
    for fname, off, nbytes in fields:
        desc = getattr(ctype, fname)
        assert (desc.offset, desc.size) == (off, nbytes), fname
        assert dtype.fields[fname][1] == off and dtype.fields[fname][0].itemsize == nbytes, fname
    assert gie.ROUTES_INFO == R.ROUTES_INFO
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    assert re.search(r"#define GIE_ROUTES_FROM_FRONTIERS 1\b", txt) and _capi.ROUTES_FROM_FRONTIERS == R.FROM_FRONTIERS == 1
    src = open(os.path.join(ROOT, "gie-mapping_amd", "csrc", "gie_routes.inc.h")).read()
    assert re.search(r"static_assert\(sizeof\(gie_routes_param\) == 48 && sizeof\(gie_routes_info\) == 32", src)
    assert re.search(r"#define GIE_ROUTES_MAX_WORDS %d\b" % R.MAX_WORDS, src) and R.LDS_WORDS == 144 * 1024 // 48

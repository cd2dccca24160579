"""numpy reference of the global block routes (include/gie.h "global block routes"): from a block table of blocks_ref (the
gie_query_global records of a box of voxels, by block) the node / pairs / link / frontier planes of a box of blocks, the cell bytes,
the BFS field by a plain queue, the info record, the gather, the descent with its neighbour order and the host layer's goal order.
Every value is an integer, so a device result and its reference are equal byte for byte."""
from collections import deque

import numpy as np

import blocks_ref as B
from blocks_ref import FNT, FREE, OCCUPIED, UNKNOWN  # noqa: F401

FROM_FRONTIERS = 1                      # GIE_ROUTES_FROM_FRONTIERS
NODE, LINK_X, LINK_Y, LINK_Z, FRONTIER, SOURCE = 1, 2, 4, 8, 16, 32
MAX_WORDS = 16384                       # the size limit: ceil(nx / 64) * ny * nz 64-bit words a plane
LDS_WORDS = 3072                        # up to here the BFS keeps all six planes in LDS
ROUTES_INFO = np.dtype([("n_nodes", "<i4"), ("n_links", "<i4"), ("n_frontier", "<i4"), ("n_sources", "<i4"), ("n_reached", "<i4"), ("max_steps", "<i4"),
                        ("reserved", "<i4", (2,))])
STEP = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # the descent's neighbour order: -x +x -y +y -z +z


def words(lo, hi):
    n = [int(hi[k]) - int(lo[k]) + 1 for k in range(3)]
    return (n[0] + 63) // 64 * n[1] * n[2]


def point_blocks(xyz, w):
    """block coordinate of n points (metres): gie_pos2coord per axis in fp32, then >> 3 -> (blocks int64 [n, 3], finite [n])"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = np.floor(xyz / np.float32(w) + np.float32(0.5))
    ok = ((u >= np.float32(-1.0e9)) & (u <= np.float32(1.0e9))).all(1)           # (NaN compares false)
    return np.where(ok[:, None], u, 0).astype(np.int64) >> 3, ok


def dense_types(table, lo, hi):
    """the types of the box's blocks, [nz, ny, nx, 8 (x), 8 (y), 8 (z)]; UNKNOWN where the table has no block"""
    keys, ty, _ = table
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    n = hi - lo + 1
    t = np.zeros((n[2], n[1], n[0], 512), np.int64)
    k = keys.astype(np.int64) - lo
    sel = ((k >= 0) & (k < n)).all(1)
    t[k[sel, 2], k[sel, 1], k[sel, 0]] = ty[sel]
    return t.reshape(n[2], n[1], n[0], 8, 8, 8)


class Graph:
    """node, pairs, link and frontier planes of the box lo..hi ([nz, ny, nx]; pairs and link [3 (axis x y z), nz, ny, nx])"""

    def __init__(self, table, lo, hi, min_free=1, min_open=1, min_fnt=1):
        self.lo, self.hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        n = self.hi - self.lo + 1
        self.shape = (int(n[2]), int(n[1]), int(n[0]))
        self.n_pass = np.zeros(self.shape, np.int64)
        self.node, self.frontier = np.zeros(self.shape, bool), np.zeros(self.shape, bool)
        self.pairs, self.link = np.zeros((3,) + self.shape, np.int64), np.zeros((3,) + self.shape, bool)
        # the part of the box the table has blocks in: beyond it every voxel is UNKNOWN, so there is no node, no pair and no link
        clo, chi = np.maximum(self.lo, table[0].min(0)), np.minimum(self.hi, table[0].max(0))
        if (clo > chi).any():
            return
        t = dense_types(table, clo, chi)
        p = (t == FREE) | (t == FNT)
        n_pass = p.sum((3, 4, 5))
        node = n_pass >= min_free
        frontier = node & ((t == FNT).sum((3, 4, 5)) >= min_fnt)
        pairs = np.zeros((3,) + node.shape, np.int64)
        pairs[0][:, :, :-1] = (p[:, :, :-1, 7, :, :] & p[:, :, 1:, 0, :, :]).sum((3, 4))
        pairs[1][:, :-1, :] = (p[:, :-1, :, :, 7, :] & p[:, 1:, :, :, 0, :]).sum((3, 4))
        pairs[2][:-1, :, :] = (p[:-1, :, :, :, :, 7] & p[1:, :, :, :, :, 0]).sum((3, 4))
        beyond = np.zeros((3,) + node.shape, bool)                              # node(k + e_a), false beyond the box
        beyond[0][:, :, :-1], beyond[1][:, :-1, :], beyond[2][:-1, :, :] = node[:, :, 1:], node[:, 1:, :], node[1:, :, :]
        o = clo - self.lo
        at = (slice(o[2], o[2] + node.shape[0]), slice(o[1], o[1] + node.shape[1]), slice(o[0], o[0] + node.shape[2]))
        self.n_pass[at], self.node[at], self.frontier[at] = n_pass, node, frontier
        for a in range(3):
            self.pairs[a][at], self.link[a][at] = pairs[a], node & beyond[a] & (pairs[a] >= min_open)

    def cell_of(self, blocks, ok=None):
        """(cells [n, 3] as (x, y, z) offsets into the box, inside [n])"""
        c = np.asarray(blocks, np.int64).reshape(-1, 3) - self.lo
        inside = ((c >= 0) & (c < np.array(self.shape[::-1]))).all(1)
        if ok is not None:
            inside &= ok
        return np.where(inside[:, None], c, 0), inside

    def solve(self, goal_blocks=(), goal_ok=None, flags=0):
        """the sources, the BFS by a plain queue -> self (source, steps, cells, info)"""
        src = self.frontier.copy() if flags & FROM_FRONTIERS else np.zeros(self.shape, bool)
        c, inside = self.cell_of(np.asarray(goal_blocks, np.int64).reshape(-1, 3), goal_ok)
        for (x, y, z), ins in zip(c.tolist(), inside.tolist()):
            if ins and self.node[z, y, x]:
                src[z, y, x] = True
        steps = np.full(self.shape, -1, np.int32)
        q = deque()
        for z, y, x in np.argwhere(src).tolist():
            steps[z, y, x] = 0
            q.append((x, y, z))
        while q:
            x, y, z = q.popleft()
            for nb in self.neighbours(x, y, z):
                if steps[nb[2], nb[1], nb[0]] < 0:
                    steps[nb[2], nb[1], nb[0]] = steps[z, y, x] + 1
                    q.append(nb)
        self.source, self.steps = src, steps
        self.cells = np.where(self.node, NODE | self.link[0] * LINK_X | self.link[1] * LINK_Y | self.link[2] * LINK_Z | self.frontier * FRONTIER | src * SOURCE,
                              0).astype(np.uint8)
        self.info = np.zeros((), ROUTES_INFO)
        self.info["n_nodes"], self.info["n_links"], self.info["n_frontier"] = self.node.sum(), self.link.sum(), self.frontier.sum()
        self.info["n_sources"], self.info["n_reached"], self.info["max_steps"] = src.sum(), (steps >= 0).sum(), steps.max()
        return self

    def neighbours(self, x, y, z):
        """the cells joined to (x, y, z) by a link, in the descent's order"""
        out = []
        for a, (dx, dy, dz) in enumerate(STEP):
            nx, ny, nz = x + dx, y + dy, z + dz
            if not (0 <= nx < self.shape[2] and 0 <= ny < self.shape[1] and 0 <= nz < self.shape[0]):
                continue
            ok = self.link[a // 2][z, y, x] if a & 1 else self.link[a // 2][nz, ny, nx]      # +a: the link of this cell; -a: the neighbour's
            if ok:
                out.append((nx, ny, nz))
        return out

    def query(self, xyz, w):
        blocks, ok = point_blocks(xyz, w)
        c, inside = self.cell_of(blocks, ok)
        return np.where(inside, self.steps[c[:, 2], c[:, 1], c[:, 0]], -1).astype(np.int32)

    def path(self, starts, w, max_len, fill=0):
        """(path_key [n, max_len, 3] with `fill` where nothing is written, len [n])"""
        blocks, ok = point_blocks(starts, w)
        c, inside = self.cell_of(blocks, ok)
        path = np.full((len(c), max_len, 3), fill, np.int32)
        ln = np.zeros(len(c), np.int32)
        for i, ((x, y, z), ins) in enumerate(zip(c.tolist(), inside.tolist())):
            cur = int(self.steps[z, y, x]) if ins else -1
            ln[i] = cur + 1
            if cur < 0:
                continue
            for j in range(max_len):
                path[i, j] = (x + self.lo[0], y + self.lo[1], z + self.lo[2])
                if cur == 0:
                    break
                x, y, z = next(nb for nb in self.neighbours(x, y, z) if self.steps[nb[2], nb[1], nb[0]] == cur - 1)
                cur -= 1
        return path, ln


def routes_box(keys, rb):
    """the host layer's box: the bounding box of the goals' keys and the robot's block rb, widened by one block; over the size limit it
    is cut to rb +- h on every axis, h halving from the longest reach until the box fits"""
    k = np.concatenate([np.asarray(keys, np.int64).reshape(-1, 3), np.asarray(rb, np.int64).reshape(1, 3)])
    lo, hi = k.min(0) - 1, k.max(0) + 1
    rb = np.asarray(rb, np.int64)
    h = int(max((rb - lo).max(), (hi - rb).max()))
    while words(lo, hi) > MAX_WORDS:
        h //= 2
        lo, hi = np.maximum(lo, rb - h), np.minimum(hi, rb + h)
    return lo, hi


def route_goals(table, rec, robot_pos, w, max_goals, min_free=1, min_open=1, min_fnt=1):
    """VolumetricMapper::global_frontier_routes: blocks_ref.goals' goals, the routes from the robot's position over routes_box, the
    goals ordered by steps (unreachable last, ties and the unreachable in the old order) -> (positions, keys, n_fnt, min_dist_sq, steps)"""
    pos, n_fnt, dmin = B.goals(rec, robot_pos, w, max_goals)
    keys, _ = point_blocks(pos, w)
    rb, _ = point_blocks(np.asarray(robot_pos, np.float32).reshape(1, 3), w)
    lo, hi = routes_box(keys, rb[0])
    g = Graph(table, lo, hi, min_free, min_open, min_fnt).solve(rb, None, 0)
    steps = g.query(pos, w)
    order = np.argsort(np.where(steps < 0, np.iinfo(np.int64).max, steps.astype(np.int64)), kind="stable")
    return pos[order], keys[order].astype(np.int32), n_fnt[order], dmin[order], steps[order]

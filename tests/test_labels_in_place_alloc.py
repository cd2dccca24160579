"""A label plane left in place (gie_ogm_labels_dev_borrow) launches nothing of its own: gie_fuse's block allocation looks at the
labels of the table cells that have no block yet (k_cell_alloc, gie_block_observed) instead of at flags a pass over the whole plane
has set.  Every test drives two mappers with the same poses and planes — one borrows, the other has its plane copied (the storing
kernel flags the blocks as before) — and compares the local map bit for bit and the pool's block count after every update; where
the expected set of blocks can be written down, it is counted too."""
import numpy as np
import pytest

import gie
from gie import scenes

pytestmark = pytest.mark.gpu

W = 0.05
KEYS = ("edt", "type", "dist_sq", "coc")


def _pose_for_pivot_mod(size, mods, shift=(0, 0, 0)):
    """A position whose local pivot is congruent to `mods` modulo 8 on every axis (plus `shift` blocks)."""
    cell = [(size[i] // 2 + mods[i]) % 8 + 8 * int(shift[i]) for i in range(3)]      # pivot = cell - size // 2
    pos = tuple(np.float32(c * W) for c in cell)
    pvt = scenes.local_pivot(pos, W, size)
    assert tuple(p % 8 for p in pvt) == tuple(mods)
    return pos, pvt


def _blocks_of(lab, pvt):
    """global block coordinates that hold an observed voxel of plane `lab` [Z][Y][X]"""
    z, y, x = np.nonzero((lab == 1) | (lab == 2))
    return set(zip(((x + pvt[0]) >> 3).tolist(), ((y + pvt[1]) >> 3).tolist(), ((z + pvt[2]) >> 3).tolist()))


class Pair:
    """the borrowing mapper and its copying twin"""

    def __init__(self, size, **cfg):
        import torch
        self.torch, self.size = torch, size
        self.dev = torch.device("cuda", 0)
        c = gie.make_config(W, size, cutoff_dist=cfg.pop("cutoff_dist", 0.5), **cfg)
        self.cfg = c
        self.a, self.b = gie.Mapper(c), gie.Mapper(c)
        self.step_no = 0

    def close(self):
        self.a.close(); self.b.close()

    def upload(self, lab):
        d = self.torch.from_numpy(np.ascontiguousarray(lab.astype(np.int8))).to(self.dev)
        self.torch.cuda.synchronize()
        return d

    def feed(self, pos, ptr, q=(1.0, 0.0, 0.0, 0.0)):
        self.a.set_pose(pos, q); self.b.set_pose(pos, q)
        assert self.a.ogm_labels_dev(ptr, borrow=True) is True
        assert self.b.ogm_labels_dev(ptr, borrow=False) is False

    def step_and_compare(self, blocks=None):
        self.a.step(); self.b.step()
        self.a.sync(); self.b.sync()
        ra, rb = self.a.read_local(), self.b.read_local()
        for key in KEYS:
            assert np.array_equal(ra[key].view(np.uint8), rb[key].view(np.uint8)), (self.step_no, key)      # bit for bit (edt is fp32)
        na, nb = self.a.stats()["blocks_total"], self.b.stats()["blocks_total"]
        assert na == nb, (self.step_no, na, nb)
        if blocks is not None:
            assert na == blocks, (self.step_no, na, blocks)
        self.step_no += 1
        return ra

    def update(self, pos, lab, blocks=None):
        d = self.upload(lab)
        self.feed(pos, d.data_ptr())
        return self.step_and_compare(blocks)


def _oracle_update(o, pos, lab, q=(1.0, 0.0, 0.0, 0.0)):
    o.set_pose(pos, q)
    o.ogm_labels(np.ascontiguousarray(lab.astype(np.int8)))
    o.fuse(); o.batch_edt(); o.merge()
    return o.read_local()


SIZES = [(16, 9, 17), (32, 24, 8)]
MODS = [(0, 0, 0), (1, 1, 1), (7, 7, 7), (0, 1, 7), (7, 0, 1), (1, 7, 0)]     # 0, 1 and 7 on each axis; 1 / 7 leave one-voxel slivers at a face


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mods", MODS, ids=lambda m: "pvt%d%d%d" % m)
def test_unaligned_pivot_partly_observed(size, mods, oracle_lib):
    """Blocks cut by every face of the volume (pivot mod 8 = 0, 1, 7 on each axis; a sliver one voxel thick included), a partly
    observed hash world over two updates: the borrowed form against the copied one and against the oracle."""
    from oracle_py import OracleMapper
    X, Y, Z = size
    p = Pair(size)
    o = OracleMapper(p.cfg)
    rng = np.random.default_rng(11 + sum(mods))
    try:
        for k in range(2):
            pos, pvt = _pose_for_pivot_mod(size, mods, shift=(k, 0, 0))
            lab = scenes.hash_world_labels(pvt, size, k, seed=4, p_occ=0.03).astype(np.int8)
            # whole blocks unobserved (block-sized hash on the global block coordinates), the others sparsely observed
            gz, gy, gx = np.meshgrid(np.arange(Z) + pvt[2], np.arange(Y) + pvt[1], np.arange(X) + pvt[0], indexing="ij")
            hb = ((gx >> 3) * 7 + (gy >> 3) * 13 + (gz >> 3) * 29 + k) % 3
            lab[hb == 0] = 0
            lab[rng.random(lab.shape) < 0.6] = 0
            got = p.update(pos, lab)
            want = _oracle_update(o, pos, lab)
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(want[key], got[key]), (k, key)
    finally:
        p.close(); o.close()


def _one_voxel_cases(size, pvt):
    """(name, plane, number of blocks) with one observed voxel per chosen block, everything else unknown"""
    X, Y, Z = size
    out = []

    def block_box(b):       # local box of global block b clipped to the volume
        lo = [max(b[i] * 8 - pvt[i], 0) for i in range(3)]
        hi = [min(b[i] * 8 + 8 - pvt[i], size[i]) for i in range(3)]
        return lo, hi

    rng = [range(pvt[i] >> 3, ((pvt[i] + size[i] - 1) >> 3) + 1) for i in range(3)]
    blocks = [(bx, by, bz) for bz in rng[2] for by in rng[1] for bx in rng[0]]          # every block that overlaps the volume
    # the last voxel of every block's clipped box (in-block index 511 for an uncut block: last row of the last layer)
    lab = np.zeros((Z, Y, X), np.int8)
    for b in blocks:
        lo, hi = block_box(b)
        lab[hi[2] - 1, hi[1] - 1, hi[0] - 1] = 1 + (sum(b) & 1)
    out.append(("last", lab, len(blocks)))
    # ... the first
    lab = np.zeros((Z, Y, X), np.int8)
    for b in blocks:
        lo, hi = block_box(b)
        lab[lo[2], lo[1], lo[0]] = 2 - (sum(b) & 1)
    out.append(("first", lab, len(blocks)))
    # the corner voxels of the volume: with pivot mod 8 = 1 / 7 they are the corner voxels of one-voxel slivers
    lab = np.zeros((Z, Y, X), np.int8)
    for cz in (0, Z - 1):
        for cy in (0, Y - 1):
            for cx in (0, X - 1):
                lab[cz, cy, cx] = 1
    out.append(("corners", lab, len(_blocks_of(lab, pvt))))
    # "the voxel just outside the volume in the same block": the blocks the faces cut hold no observed voxel inside, the blocks
    # that lie wholly inside hold one — only those may exist
    lab = np.zeros((Z, Y, X), np.int8)
    n = 0
    for b in blocks:
        lo, hi = block_box(b)
        if all(hi[i] - lo[i] == 8 for i in range(3)):
            lab[hi[2] - 1, hi[1] - 1, hi[0] - 1] = 2
            n += 1
    out.append(("outside", lab, n))
    # the voxels on the low x (y) face observed, nothing else: a row of a block the high face cuts, read past the face, would run
    # on into the next row's (layer's) first voxels — inside the plane, and observed
    for name, sl in (("xface", (slice(None), slice(None), 0)), ("yface", (slice(None), 0, slice(None)))):
        lab = np.zeros((Z, Y, X), np.int8)
        lab[sl] = 1
        out.append((name, lab, len(_blocks_of(lab, pvt))))
    return out


@pytest.mark.parametrize("size", SIZES + [(32, 24, 24)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mods", [(0, 0, 0), (1, 1, 1), (7, 7, 7), (1, 7, 0)], ids=lambda m: "pvt%d%d%d" % m)
def test_one_observed_voxel_per_block(size, mods):
    """One observed voxel per block, where the scan of a block finds it last, first, in the corner of a one-voxel sliver — or
    not at all, for the blocks whose only voxels of interest lie outside the volume.  Exactly the blocks that hold an observed voxel
    exist afterwards (fresh mappers: the pool's count is the number of blocks allocated), and their voxels are known."""
    pos, pvt = _pose_for_pivot_mod(size, mods)
    for name, lab, nblk in _one_voxel_cases(size, pvt):
        assert nblk == len(_blocks_of(lab, pvt)), name
        p = Pair(size)
        try:
            got = p.update(pos, lab, blocks=nblk)
            obs = lab != 0
            # (a voxel of a missing block would have stayed unknown; a free voxel beside unknown ones reads as a frontier)
            assert got["type"][obs].all() and np.array_equal(got["type"][obs] == 2, lab[obs] == 2), name
            assert not got["type"][~obs].any(), name
        finally:
            p.close()


def test_labels_that_are_not_observations():
    """Bytes 3, 127, -1 and -128 spread over otherwise unknown blocks are no observations: no block for them; one true observation
    among them gets its block."""
    size = (32, 24, 8)
    pos, pvt = _pose_for_pivot_mod(size, (7, 1, 0))
    X, Y, Z = size
    rng = np.random.default_rng(5)
    lab = np.zeros((Z, Y, X), np.int8)
    m = rng.random(lab.shape) < 0.25
    lab[m] = rng.choice(np.array([3, 127, -1, -128], np.int8), size=int(m.sum()))
    p = Pair(size)
    try:
        got = p.update(pos, lab, blocks=0)
        assert not got["type"].any()
        lab[Z - 1, Y - 1, X - 1] = 2
        lab[0, 0, 0] = 1
        got = p.update(pos, lab, blocks=2)
        assert int((got["type"] != 0).sum()) == 2
    finally:
        p.close()


def test_fresh_map_sparse_then_other_blocks_then_jump():
    """First update of a fresh map with one observed voxel in every 64th block (nearly every cell is scanned to its last layer), a second
    update that observes other blocks (existing blocks, new ones and cells without any), then a jump of more than the volume."""
    size = (64, 48, 40)
    X, Y, Z = size
    p = Pair(size)
    try:
        pos, pvt = _pose_for_pivot_mod(size, (3, 5, 6))
        gz, gy, gx = np.meshgrid(np.arange(Z) + pvt[2], np.arange(Y) + pvt[1], np.arange(X) + pvt[0], indexing="ij")
        bid = (gx >> 3) + 9 * (gy >> 3) + 61 * (gz >> 3)
        inb = (gx & 7) | ((gy & 7) << 3) | ((gz & 7) << 6)
        lab1 = np.where((bid % 64 == 0) & (inb == (bid // 64 * 37) % 512), 2, 0).astype(np.int8)
        n1 = _blocks_of(lab1, pvt)
        assert len(n1) >= 3
        p.update(pos, lab1, blocks=len(n1))
        lab2 = np.where((bid % 5 < 2) & (inb % 97 == bid % 97), 1, 0).astype(np.int8)
        lab2[lab1 != 0] = 1
        n2 = n1 | _blocks_of(lab2, pvt)
        assert len(n2) > len(n1) and len(n2) < (X // 8 + 1) * (Y // 8 + 1) * (Z // 8 + 1)
        p.update(pos, lab2, blocks=len(n2))
        pos3, pvt3 = _pose_for_pivot_mod(size, (1, 0, 7), shift=(20, 0, 0))       # 160 voxels further: no cell has a block
        assert pvt3[0] - pvt[0] > X
        lab3 = scenes.hash_world_labels(pvt3, size, 0, seed=8, p_occ=0.02).astype(np.int8)
        lab3[:, :, :24] = 0
        p.update(pos3, lab3, blocks=len(n2) + len(_blocks_of(lab3, pvt3)))
    finally:
        p.close()


def test_block_retention_straight_drive():
    """retain_radius_blocks > 0 on a straight drive of a dozen updates: erased cells come back as "no block" and are scanned again."""
    size = (32, 32, 16)
    p = Pair(size, retain_radius_blocks=1)
    rng = np.random.default_rng(2)
    try:
        for k in range(12):
            back = k if k < 8 else 14 - k                  # out, and back over the erased blocks
            pos, q = scenes.pose(back, W, delta_vox=7, yaw_deg=0.0)
            pvt = scenes.local_pivot(pos, W, size)
            lab = scenes.hash_world_labels(pvt, size, k, seed=5, p_occ=0.01).astype(np.int8)
            lab[rng.random(lab.shape) < 0.7] = 0
            lab[:, :, 8:16] = 0                            # a slab that is never observed
            p.update(pos, lab)
    finally:
        p.close()


def test_borrowed_scan_then_second_scan_before_step():
    """a second scan laid over a borrowed one materialises it (the storing kernel, with its flags): same map as the copied pair"""
    size = (32, 24, 24)
    p = Pair(size)
    rng = np.random.default_rng(9)
    try:
        for k in range(3):
            pos, pvt = _pose_for_pivot_mod(size, (5, 2, 1), shift=(k, 0, 0))
            lab1 = scenes.hash_world_labels(pvt, size, k, seed=3, p_occ=0.02).astype(np.int8)
            lab1[rng.random(lab1.shape) < 0.8] = 0
            lab1[:, 8:, :] = 0
            lab2 = scenes.hash_world_labels(pvt, size, k + 1, seed=3, p_occ=0.02).astype(np.int8)
            lab2[rng.random(lab2.shape) < 0.8] = 0
            lab2[:, :16, :] = 0
            d1, d2 = p.upload(lab1), p.upload(lab2)
            p.feed(pos, d1.data_ptr())
            # the second borrow of the same update: the first plane is copied, the second one stays in place
            assert p.a.ogm_labels_dev(d2.data_ptr(), borrow=True) is True
            assert p.b.ogm_labels_dev(d2.data_ptr(), borrow=False) is False
            p.step_and_compare()
    finally:
        p.close()


@pytest.mark.parametrize("mods", [(1, 7, 7), (7, 1, 1)], ids=lambda m: "pvt%d%d%d" % m)
def test_guarded_plane_reads_nothing_outside(mods):
    """The plane lies inside a larger tensor (16-byte alignment kept) whose bytes before and after it are all OCCUPIED; the plane itself is
    all unknown and the pivot unaligned: a read past the plane would find an observation and allocate a block.  None may exist."""
    import torch
    size = (16, 9, 17)
    n = size[0] * size[1] * size[2]
    guard = 4096
    pos, pvt = _pose_for_pivot_mod(size, mods)
    p = Pair(size)
    try:
        buf = torch.full((guard + n + guard,), 2, dtype=torch.int8, device=p.dev)
        assert buf.data_ptr() % 16 == 0
        buf[guard:guard + n] = 0
        torch.cuda.synchronize()
        p.feed(pos, buf.data_ptr() + guard)
        got = p.step_and_compare(blocks=0)
        assert not got["type"].any()
    finally:
        p.close()


def test_full_size_256_hash_world():
    """BASELINE config 5's generator at 256^3: three updates of the drive, borrowed against copied."""
    import torch
    import bench
    size = (256, 256, 256)
    p = Pair(size, cutoff_dist=2.0)
    try:
        feed = bench.HashWorldFeed(torch, scenes, p.dev, W, size, (0, 0, 0))
        feed.prepare(0, 3)
        for i in range(3):
            pos, q = feed.pose(i)
            p.feed(pos, feed.ptrs[i], q)
            p.step_and_compare()
        assert p.a.stats()["blocks_total"] >= 32 ** 3
    finally:
        p.close()

"""The numpy reference of the global block summaries (tests/blocks_ref.py) against a literal voxel-by-voxel loop on hand-made
records, the binding's structs against the header, and the grid's indexing.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blocks_ref as R
import gie
from gie import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VLO, VHI = (-16, -8, -8), (8, 8, 16)                             # blocks x -2..0, y -1..0, z -1..1


def hand_made():
    """types and distances of the box [VLO, VHI) in box_coords' order, and the blocks with a story by name"""
    rng = np.random.default_rng(11)
    xyz = R.box_coords(VLO, VHI)
    ty = rng.integers(0, 4, len(xyz)).astype(np.int8)
    d = rng.integers(1, 400, len(xyz)).astype(np.int32)
    blk = xyz >> 3
    named = {"unknown": (-1, 0, 0), "corner": (0, -1, -1), "all_fnt": (-2, -1, 0), "none_valid": (-1, -1, -1), "edge_valid": (0, 0, 0),
             "zero": (-2, 0, 1), "occupied_near": (0, -1, 1)}

    def of(name):
        return (blk == np.array(named[name])).all(1)

    def vox(name, v):
        return of(name) & ((xyz & 7) == np.array(v)).all(1)
    ty[of("unknown")] = R.UNKNOWN
    ty[of("corner")] = R.UNKNOWN
    ty[vox("corner", (7, 7, 7))] = R.OCCUPIED                    # exactly one known voxel, in the last corner
    ty[of("all_fnt")] = R.FNT                                    # 512 in a 10-bit field
    for name in ("none_valid", "edge_valid", "zero", "occupied_near"):
        ty[of(name)] = R.UNKNOWN
    for v, t, dist in (((0, 0, 0), R.FREE, -1), ((1, 0, 0), R.FNT, 900000), ((2, 0, 0), R.FREE, R.EMPTY_VALUE)):
        ty[vox("none_valid", v)], d[vox("none_valid", v)] = t, dist
    for v, t, dist in (((3, 1, 2), R.FREE, 900000), ((3, 1, 3), R.FNT, 899999), ((0, 0, 1), R.FREE, R.EMPTY_VALUE)):
        ty[vox("edge_valid", v)], d[vox("edge_valid", v)] = t, dist
    for v, t, dist in (((5, 5, 5), R.FNT, 0), ((5, 5, 6), R.FREE, -1), ((1, 1, 1), R.FREE, 7)):
        ty[vox("zero", v)], d[vox("zero", v)] = t, dist
    for v, t, dist in (((4, 4, 4), R.OCCUPIED, 0), ((4, 4, 5), R.FREE, 5), ((4, 5, 5), R.FNT, 9)):
        ty[vox("occupied_near", v)], d[vox("occupied_near", v)] = t, dist
    return xyz, ty, d, named


def literal(xyz, ty, d, flags, min_fnt, lo, hi, for_grid=False):
    """one pass over the voxels, a dictionary of blocks: the definition of include/gie.h word for word"""
    blocks = {}
    for (x, y, z), t, dist in zip(xyz.tolist(), ty.tolist(), d.tolist()):
        key = (x >> 3, y >> 3, z >> 3)
        b = blocks.setdefault(key, dict(n={R.FREE: 0, R.OCCUPIED: 0, R.FNT: 0}, fnt=R.NONE, free=R.NONE, dmin=None))
        idx = (x & 7) * 64 + (y & 7) * 8 + (z & 7)
        if t in b["n"]:
            b["n"][t] += 1
        if t == R.FNT:
            b["fnt"] = min(b["fnt"], idx)
        if t in (R.FREE, R.FNT):
            b["free"] = min(b["free"], idx)
            if (flags & R.DIST) and 0 <= dist < 900000:
                b["dmin"] = dist if b["dmin"] is None else min(b["dmin"], dist)
    out = []
    for key in sorted(blocks, key=lambda k: (k[2], k[1], k[0])):
        b = blocks[key]
        if sum(b["n"].values()) == 0 or not all(lo[k] <= key[k] <= hi[k] for k in range(3)):
            continue
        if not for_grid and b["n"][R.FNT] < min_fnt:
            continue
        out.append((key, b["n"][R.FREE], b["n"][R.OCCUPIED], b["n"][R.FNT], b["fnt"], b["free"], flags,
                    R.EMPTY_VALUE if b["dmin"] is None else b["dmin"], 0))
    return np.array(out, R.BLOCK_SUMMARY_DTYPE) if out else np.zeros(0, R.BLOCK_SUMMARY_DTYPE)


@pytest.fixture(scope="module")
def data():
    xyz, ty, d, named = hand_made()
    return xyz, ty, d, named, R.block_table(ty, d, VLO, VHI)


def by_key(rec, key):
    hit = rec[(rec["key"] == np.array(key)).all(1)]
    return hit[0] if len(hit) else None


@pytest.mark.parametrize("flags", [0, R.DIST])
def test_reference_agrees_with_the_literal_loop(data, flags):
    xyz, ty, d, named, table = data
    for lo, hi in ((R.OPEN[:1] * 3, R.OPEN[1:] * 3), ((-2, -1, -1), (0, 0, 1)), ((-1, -1, 0), (5, 0, 0)), ((1, 1, 2), (3, 3, 3))):
        for min_fnt in (0, 1, 3, 512):
            want = literal(xyz, ty, d, flags, min_fnt, lo, hi)
            got = R.summaries(table, flags, min_fnt, lo, hi)
            assert got.tobytes() == want.tobytes(), (flags, lo, hi, min_fnt)
    rec = R.summaries(table, flags)
    assert len(rec) == 3 * 2 * 3 - 1 and (rec["key"] < 0).any()                  # every block but the UNKNOWN one; negative coordinates
    assert by_key(rec, named["unknown"]) is None
    c = by_key(rec, named["corner"])
    assert (c["n_free"], c["n_occupied"], c["n_fnt"], c["fnt_voxel"], c["free_voxel"]) == (0, 1, 0, R.NONE, R.NONE)
    f = by_key(rec, named["all_fnt"])
    assert (f["n_free"], f["n_occupied"], f["n_fnt"], f["fnt_voxel"], f["free_voxel"]) == (0, 0, 512, 0, 0)
    want_d = {"none_valid": R.EMPTY_VALUE, "edge_valid": 899999, "zero": 0, "occupied_near": 5, "corner": R.EMPTY_VALUE}
    for name, v in want_d.items():
        assert by_key(rec, named[name])["min_dist_sq"] == (v if flags else R.EMPTY_VALUE), name
    assert (rec["flags"] == flags).all() and (rec["reserved"] == 0).all()
    e = by_key(rec, named["edge_valid"])
    assert (e["fnt_voxel"], e["free_voxel"]) == (3 * 64 + 1 * 8 + 3, 0 * 64 + 0 * 8 + 1)


def test_arithmetic_shift_not_division(data):
    xyz, _, _, _, table = data
    keys = table[0]
    assert keys[:, 0].min() == -2 and (keys[:, 0] == -1).any()                   # voxel -1 lies in block -1, voxel -16 in block -2
    assert {tuple(k) for k in keys.tolist()} == {tuple(k) for k in (xyz >> 3).tolist()}
    assert int(np.int32(-1) >> 3) == -1 and int(-1 / 8) == 0


def test_min_fnt_thresholds(data):
    _, _, _, named, table = data
    n = int(by_key(R.summaries(table), named["zero"])["n_fnt"])
    assert n == 1
    for min_fnt, there in ((0, True), (1, True), (n, True), (n + 1, False)):
        assert (by_key(R.summaries(table, 0, min_fnt), named["zero"]) is not None) == there, min_fnt
    assert by_key(R.summaries(table, 0, 512), named["all_fnt"]) is not None
    assert by_key(R.summaries(table, 0, 1), named["corner"]) is None and by_key(R.summaries(table, 0, 0), named["corner"]) is not None


def test_the_full_fnt_block_stays_in_its_field(data):
    _, _, _, named, table = data
    lo = hi = named["all_fnt"]
    g = R.grid(table, lo, hi)
    assert g.shape == (1, 1, 1) and int(g[0, 0, 0]) == (1 << 31) | (512 << 20)
    assert (int(g[0, 0, 0]) >> 20) & 0x7ff == 512 and int(g[0, 0, 0]) & 0xfffff == 0


# ---------------------------------------------------------------------------------------------------------- the structs
def header_struct(name):
    """[(field, offset, size)] and the size of a struct of include/gie.h made of int32_t / uint16_t members, natural alignment"""
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size_of = {"int32_t": 4, "uint32_t": 4, "uint16_t": 2, "int16_t": 2}
    fields, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        s = size_of[ctype]
        align = max(align, s)
        for nm in names.split(","):
            nm = nm.strip()
            mt = re.fullmatch(r"(\w+)\[(\d+)\]", nm)
            count = int(mt.group(2)) if mt else 1
            off = (off + s - 1) // s * s
            fields.append((mt.group(1) if mt else nm, off, s * count))
            off += s * count
    return fields, (off + align - 1) // align * align


@pytest.mark.parametrize("name,ctype,dtype,size", [("gie_blocks_param", _capi.BlocksParam, None, 48),
                                                    ("gie_block_summary", _capi.BlockSummary, gie.BLOCK_SUMMARY_DTYPE, 32)])
def test_binding_structs_match_the_header(name, ctype, dtype, size):
    fields, total = header_struct(name)
    assert total == size == C.sizeof(ctype)
    assert [f[0] for f in fields] == [f[0] for f in ctype._fields_]
    for fname, off, nbytes in fields:
        desc = getattr(ctype, fname)
        assert (desc.offset, desc.size) == (off, nbytes), fname
    if dtype is not None:
        assert dtype.itemsize == size and dtype == R.BLOCK_SUMMARY_DTYPE
        for fname, off, nbytes in fields:
            assert dtype.fields[fname][1] == off and dtype.fields[fname][0].itemsize == nbytes, fname
    txt = open(os.path.join(ROOT, "include", "gie.h")).read()
    assert re.search(r"#define GIE_BLOCKS_DIST 1\b", txt) and _capi.BLOCKS_DIST == R.DIST == 1
    assert re.search(r"#define GIE_EMPTY_VALUE %d\b" % R.EMPTY_VALUE, txt)


# ---------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("lo,hi", [((-1, -1, 0), (-1, -1, 0)),         # one block
                                   ((-2, -1, -1), (0, 0, 1)),           # the data's box: 3 x 2 x 3
                                   ((-1, -1, 0), (3, 0, 0)),            # non-cubic, partly beside the data
                                   ((-4, -3, -2), (1, 2, 0)),           # around the data's low corner
                                   ((5, 5, 5), (6, 8, 5))])             # wholly beside the data
def test_grid_indexing(data, lo, hi):
    xyz, ty, d, _, table = data
    g = R.grid(table, lo, hi)
    nx, ny, nz = (hi[k] - lo[k] + 1 for k in range(3))
    assert g.shape == (nz, ny, nx) and g.dtype == np.uint32
    flat = np.zeros(nx * ny * nz, np.uint32)
    for r in literal(xyz, ty, d, 0, 0, lo, hi, for_grid=True):
        x, y, z = (int(v) for v in r["key"])
        flat[((z - lo[2]) * ny + (y - lo[1])) * nx + (x - lo[0])] = (1 << 31) | (int(r["n_fnt"]) << 20) | (int(r["n_occupied"]) << 10) | int(r["n_free"])
    assert np.array_equal(g.ravel(), flat)
    inside = all(lo[k] <= VHI[k] // 8 - 1 and hi[k] >= VLO[k] // 8 for k in range(3))
    assert (g != 0).any() == inside
    # the grid ignores min_fnt: a block without FNT voxels has its cell
    no_fnt = [r for r in literal(xyz, ty, d, 0, 0, lo, hi, for_grid=True) if r["n_fnt"] == 0]
    for r in no_fnt:
        x, y, z = (int(v) - lo[k] for k, v in enumerate(r["key"]))
        assert g[z, y, x] >> 31 == 1 and (int(g[z, y, x]) >> 20) & 0x3ff == 0


def test_goal_order_and_positions():
    rec = np.zeros(4, R.BLOCK_SUMMARY_DTYPE)
    rec["key"] = [(3, 0, 0), (0, 0, -3), (-1, 2, 0), (0, 3, 0)]
    rec["n_fnt"] = [4, 5, 6, 7]
    rec["fnt_voxel"] = [0, 511, 1 * 64 + 2 * 8 + 3, 7]
    rec["min_dist_sq"] = [1, 2, 3, 4]
    pos, n_fnt, dmin = R.goals(rec, (0.04, 0.0, -0.04), 0.1, 3)                  # the robot's voxel (0, 0, 0): block (0, 0, 0)
    assert n_fnt.tolist() == [6, 5, 4] and dmin.tolist() == [3, 2, 1]             # distance 5, then 9 three times: ties by key (z, y, x)
    w = np.float32(0.1)
    want = np.array([(-8 + 1, 16 + 2, 3), (7, 7, -24 + 7), (24, 0, 0)], np.float32) * w
    assert pos.dtype == np.float32 and pos.tobytes() == want.tobytes()

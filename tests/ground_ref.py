"""numpy / scipy statement of the ground costmap (include/gie.h "ground costmap").

Volumes are [Z][Y][X] like Mapper.read_local, cell planes [Y][X]; sizes are (X, Y, Z); z_lo / z_hi are GLOBAL voxel z, inclusive."""
import numpy as np
from scipy import ndimage

from gie import scenes

UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
UNKNOWN_BLOCKS = 1
EMPTY = 999999                                                  # GIE_EMPTY_VALUE
NO_TOP = -2 ** 31                                               # INT32_MIN
SEENDIST = np.dtype([("d", "<f4"), ("s", "u1"), ("o", "u1"), ("pad", "u1", (2,))])
CELL = np.dtype([("dist_sq", "<i4"), ("coc", "<i4", (2,)), ("type", "i1"), ("inside", "u1"), ("pad", "u1", (2,))])


def band(pvt_z, Z, z_lo, z_hi):
    """the LOCAL layers [z0, z1) of B = [max(z_lo, pvt_z), min(z_hi, pvt_z + Z - 1)]; z0 == z1 when it is empty"""
    z0, z1 = max(z_lo, pvt_z) - pvt_z, min(z_hi, pvt_z + Z - 1) - pvt_z + 1
    return (z0, z1) if z0 < z1 else (0, 0)


def columns(vtype, pvt_z, z_lo, z_hi, min_known=1):
    """(type int8 [Y][X], top int32 [Y][X] global z, counts int32 [4]) of the band's columns"""
    vtype = np.asarray(vtype)
    Z = vtype.shape[0]
    z0, z1 = band(pvt_z, Z, z_lo, z_hi)
    b = vtype[z0:z1]
    occ = (b == OCCUPIED).any(axis=0)
    known = ((b == FREE) | (b == FNT) | (b == OCCUPIED)).sum(axis=0)
    fnt = (b == FNT).any(axis=0)
    ctype = np.where(occ, OCCUPIED, np.where(known < min_known, UNKNOWN, np.where(fnt, FNT, FREE))).astype(np.int8)
    gz = np.arange(z0, z1, dtype=np.int64)[:, None, None] + pvt_z
    top = np.where(b == OCCUPIED, gz, NO_TOP).max(axis=0, initial=NO_TOP).astype(np.int32)
    return ctype, top, np.bincount(ctype.ravel(), minlength=4).astype(np.int32)


def obstacles(ctype, flags=0):
    return (ctype == OCCUPIED) | ((ctype == UNKNOWN) if flags & UNKNOWN_BLOCKS else False)


def dist_sq(obs):
    """int32 [Y][X]: the exact squared distance to the nearest obstacle cell, from scipy's indices; -1 everywhere without one"""
    obs = np.asarray(obs, bool)
    if not obs.any():
        return np.full(obs.shape, -1, np.int32)
    _, idx = ndimage.distance_transform_edt(~obs, return_indices=True)
    return ((idx - np.indices(obs.shape)).astype(np.int64) ** 2).sum(axis=0).astype(np.int32)


def field(vtype, pvt, z_lo, z_hi, min_known=1, flags=0):
    """{"type", "top", "counts", "obs", "dist_sq"} of the local types `vtype` at pivot `pvt`"""
    ctype, top, counts = columns(vtype, pvt[2], z_lo, z_hi, min_known)
    obs = obstacles(ctype, flags)
    return {"type": ctype, "top": top, "counts": counts, "obs": obs, "dist_sq": dist_sq(obs)}


def check_witness(coc, f, pvt):
    """coc [Y][X][2] (global x, y) against the field: in range, an obstacle column, at exactly dist_sq; EMPTY without an obstacle"""
    Y, X = f["obs"].shape
    if not f["obs"].any():
        assert (coc == EMPTY).all()
        return
    cx, cy = coc[..., 0].astype(np.int64) - pvt[0], coc[..., 1].astype(np.int64) - pvt[1]
    assert (cx >= 0).all() and (cx < X).all() and (cy >= 0).all() and (cy < Y).all()
    assert f["obs"][cy, cx].all()
    yy, xx = np.indices((Y, X))
    assert np.array_equal((cx - xx) ** 2 + (cy - yy) ** 2, f["dist_sq"])


def costmap(f, size, pvt, voxel_width, z_lo):
    """(payload [Y][X] SEENDIST, header fields) of gie_read_costmap_ground"""
    d = f["dist_sq"]
    pay = np.zeros(d.shape, SEENDIST)
    pay["d"] = np.where(d < 0, np.float32(size[0] ** 2 + size[1] ** 2 + size[2] ** 2), np.sqrt(np.maximum(d, 0).astype(np.float32)))
    pay["o"] = f["type"] != UNKNOWN
    w = np.float32(voxel_width)
    hdr = {"x_size": size[0], "y_size": size[1], "z_size": 1, "x_origin": np.float32(pvt[0]) * w, "y_origin": np.float32(pvt[1]) * w,
           "z_origin": np.float32(z_lo) * w, "width": w, "type": 1}
    return pay, hdr


def query(f, coc, pvt, voxel_width, xy):
    """the records (CELL) of world points xy (n x 2 metres); `coc` [Y][X][2] is the field's own (a witness, not recomputed)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    Y, X = f["type"].shape
    out = np.zeros(len(xy), CELL)
    out["dist_sq"], out["coc"], out["type"] = -1, EMPTY, UNKNOWN
    for i, p in enumerate(xy):
        if not np.isfinite(p).all():
            continue
        x, y = scenes.pos2coord(p[0], voxel_width) - pvt[0], scenes.pos2coord(p[1], voxel_width) - pvt[1]
        if 0 <= x < X and 0 <= y < Y:
            out[i] = (f["dist_sq"][y, x], coc[y, x], f["type"][y, x], 1, (0, 0))
    return out

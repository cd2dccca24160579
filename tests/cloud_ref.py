"""numpy reference of the display clouds (include/gie.h "display clouds"): the selected voxels of the local volume, or of a box of
global voxels with their gie_query_global records, as gie_cloud_point records — every value exact in float32, so a device cloud
and its reference are equal as sets of 16-byte records (`canon` sorts them by their bit patterns)."""
import numpy as np

CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
TYPE, DIST = 0, 1
UNKNOWN, FREE, OCCUPIED, FNT = 0, 1, 2, 3
KNOWN = (1 << FREE) | (1 << OCCUPIED) | (1 << FNT)
NO_BAND = (-2 ** 31, 2 ** 31 - 1)
DIST_END = 900000                       # the reference's invalid_dist_glb: dist_sq < 0 or >= 900000


def param(type_mask, intensity=TYPE, z_lo=None, z_hi=None):
    return dict(type_mask=int(type_mask), intensity=int(intensity), z_lo=NO_BAND[0] if z_lo is None else int(z_lo),
                z_hi=NO_BAND[1] if z_hi is None else int(z_hi))


def reference_params(slice_z):
    """the reference's four clouds (volumetric_mapper.h:181-357): name -> (form, param)"""
    return {"loc_ogm": ("local", param(1 << OCCUPIED, TYPE)), "loc_edt": ("local", param(KNOWN, DIST)),
            "glb_ogm": ("global", param(1 << OCCUPIED, TYPE)), "glb_edt": ("global", param(KNOWN, DIST, slice_z, slice_z))}


def _records(g, inten, w):
    out = np.zeros(len(g), CLOUD_DTYPE)
    w = np.float32(w)
    out["x"], out["y"], out["z"] = (g[:, k].astype(np.float32) * w for k in range(3))
    out["intensity"] = inten
    return out


def _mask_on(types, type_mask):
    t = types.astype(np.int64)
    return (t >= 0) & (t < 32) & (((np.int64(type_mask) >> np.clip(t, 0, 31)) & 1) != 0)


def local_cloud(types, edt, pvt, w, p):
    """types int8 / edt float32 [Z][Y][X] as Mapper.read_local returns them, pvt = Mapper.pivot()"""
    Z, Y, X = types.shape
    gz, gy, gx = np.meshgrid(np.arange(Z, dtype=np.int64) + pvt[2], np.arange(Y, dtype=np.int64) + pvt[1], np.arange(X, dtype=np.int64) + pvt[0],
                             indexing="ij")
    sel = _mask_on(types, p["type_mask"]) & (gz >= p["z_lo"]) & (gz <= p["z_hi"])
    g = np.stack([gx[sel], gy[sel], gz[sel]], -1)
    if p["intensity"] == TYPE:
        inten = types[sel].astype(np.float32)
    else:
        inten = edt[sel].astype(np.float32) * np.float32(w)
    return _records(g, inten, w)


def global_cloud(records, xyz, w, p):
    """records = Mapper.query_global(xyz) (VOXEL_DTYPE [n]) of the global voxels xyz (n x 3), each voxel once"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    d = records["dist_sq"].astype(np.int64)
    sel = _mask_on(records["vox_type"], p["type_mask"]) & (xyz[:, 2] >= p["z_lo"]) & (xyz[:, 2] <= p["z_hi"])
    if p["intensity"] == DIST:
        sel &= (d >= 0) & (d < DIST_END)
        inten = np.sqrt(d[sel].astype(np.float32)) * np.float32(w)
    else:
        inten = records["vox_type"][sel].astype(np.float32)
    return _records(xyz[sel], inten, w)


def canon(cloud):
    """the cloud as an (n, 4) uint32 array of bit patterns, rows sorted: two clouds are the same set iff these are equal"""
    a = np.ascontiguousarray(cloud).view(np.uint32).reshape(-1, 4)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def same(a, b):
    ca, cb = canon(a), canon(b)
    return ca.shape == cb.shape and np.array_equal(ca, cb)


def box_coords(lo, hi):
    """every global voxel of the box [lo, hi) (int32, n x 3)"""
    gz, gy, gx = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], -1).astype(np.int32)

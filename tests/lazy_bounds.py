"""The lazy tiles' distance bounds, checked at the map update that writes them (gie_ops.h "lazy pairs", "deferred records").

Mark + commit records per 8^3 tile `tmax` = 1 + the largest distance it committed there; the next update's gie_tile_oldskip trusts
it, and a tile whose bound is too small silently skips the stored-record test.  The oracle has no tiles, so comparing maps after
every update only shows a wrong bound on a later drive that happens to expose it.  `check_update` holds the per-tile state of the
last update (gie_debug_tile_state) against data that does not come from tmax / tbmax:

  (a) stored records: every voxel of a tile with a finite bound has a stored distance <= tmax - 1, at exactly the distance of its
      stored closest obstacle (query_global);
  (b) lazy tiles: tlazy => tknown and tskip == 2, and tmax - 1 >= the largest TRUE batch distance of the tile (a host EDT of the
      update's occupied voxels);
  (c) pass Z's streaming form (zstream): tbmax <= 80 is the tile's true largest batch distance, and a true largest distance <= 80 is
      never above tbmax; the columns it gave up (zredo) hold tiles with "81 or more".

`check_definition` is the oracle-free check of the committed field (test_oracle_edt.py), for chosen updates.  `Drive` generates
the drives of test_lazy_bounds.py (GPU) and test_lazy_bounds_emu.py (CPU emulation); `run_checked_drive` runs one against the
oracle with every check."""
import numpy as np

from gie import scenes

TMAX_INF = 0x7fffffff
ZS_EXACT = 80                       # pass Z's streaming form records a tile's largest distance exactly below (GIE_ZS_R + 1)^2 = 81


def host_batch_edt(types):
    """True batch distance^2 of every voxel to the nearest voxel of type OCCUPIED (2), int64, squared from scipy's indices (no float
    rounding); None when there is no occupied voxel"""
    from scipy import ndimage
    occ = types == 2
    if not occ.any():
        return None
    _, idx = ndimage.distance_transform_edt(~occ, return_indices=True)
    d2 = np.zeros(types.shape, np.int64)
    for ax in range(3):
        g = np.arange(types.shape[ax], dtype=np.int64).reshape([-1 if a == ax else 1 for a in range(3)])
        d2 += (idx[ax].astype(np.int64) - g) ** 2
    return d2


def tile_max(vol, fill=-1):
    """[Z][Y][X] -> the largest value of every 8^3 tile, [tz][ty][tx] (partial tiles at the upper faces: their voxels only)"""
    Z, Y, X = vol.shape
    tz, ty, tx = (Z + 7) // 8, (Y + 7) // 8, (X + 7) // 8
    p = np.full((tz * 8, ty * 8, tx * 8), fill, vol.dtype)
    p[:Z, :Y, :X] = vol
    return p.reshape(tz, 8, ty, 8, tx, 8).max(axis=(1, 3, 5))


def _tile_of_voxels(shape):
    Z, Y, X = shape
    zz, yy, xx = np.meshgrid(np.arange(Z) >> 3, np.arange(Y) >> 3, np.arange(X) >> 3, indexing="ij")
    return zz, yy, xx


class Tally:
    """what the checked drive went through, for the test's "the paths ran" assertions"""

    def __init__(self):
        self.updates = []

    def add(self, k, st, n_exact, n_sampled, n_skip2, n_redo81):
        self.updates.append(dict(k=k, zstream=st["zstream"], zwide=st["zwide"], zfail=st["zfail"], caught_up=st["caught_up"],
                                 lazy_exact=n_exact, lazy_sampled=n_sampled, skip2=n_skip2, redo81=n_redo81))

    def total(self, key, after=-1):
        return sum(u[key] for u in self.updates if u["k"] > after)


def check_update(tag, m, st, types, true_d2, tally=None, k=None):
    """(a), (b), (c) on the state `st` = m.debug_tile_state() of the update just merged; `types` = m.read_local()["type"], `true_d2` =
    host_batch_edt(types).  Raises AssertionError naming the first tile that breaks an invariant."""
    X, Y, Z = m.size
    pv = np.array(m.pivot(), np.int64)
    tmax, tbmax, tlazy, tskip, tknown = st["tmax"], st["tbmax"], st["tlazy"] != 0, st["tskip"], st["tknown"] != 0
    # (a) every voxel of a tile with a finite bound: stored distance <= bound - 1, witness at exactly that distance
    fin = (tmax > 0) & (tmax < TMAX_INF)
    if fin.any():
        tz, ty, tx = _tile_of_voxels(types.shape)
        sel = fin[tz, ty, tx]
        zz, yy, xx = np.nonzero(sel)
        g = np.stack([xx, yy, zz], -1).astype(np.int64) + pv
        r = m.query_global(g.astype(np.int32))
        d = r["dist_sq"].astype(np.int64)
        bound = tmax[zz >> 3, yy >> 3, xx >> 3].astype(np.int64) - 1
        bad = d > bound
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError("%s (a): %d voxels store a distance above their tile's bound; first: local (%d, %d, %d), stored %d, "
                                 "tmax %d, tlazy %d, tskip %d" % (tag, int(bad.sum()), xx[i], yy[i], zz[i], d[i], bound[i] + 1,
                                                                  tlazy[zz[i] >> 3, yy[i] >> 3, xx[i] >> 3], tskip[zz[i] >> 3, yy[i] >> 3, xx[i] >> 3]))
        wit = ((r["coc"].astype(np.int64) - g) ** 2).sum(-1)
        badw = wit != d
        assert not badw.any(), "%s (a): %d stored records are not at the distance of their closest obstacle; first: local (%d, %d, %d), stored %d, " \
            "witness %d" % (tag, int(badw.sum()), xx[np.argmax(badw)], yy[np.argmax(badw)], zz[np.argmax(badw)], d[np.argmax(badw)], wit[np.argmax(badw)])
    # (b) lazy tiles: flagged only where the sweep's short way applies, bounded above the true batch distances
    bad = tlazy & ~(tknown & (tskip == 2))
    assert not bad.any(), "%s (b): %d lazy tiles are not known tiles flagged 2; first tile (tz, ty, tx) %s" % (tag, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    tm = tile_max(true_d2) if true_d2 is not None else None
    n_exact = n_sampled = n_redo81 = 0
    if tlazy.any():
        assert tm is not None, "%s (b): lazy tiles in an update without obstacles" % tag
        under = tlazy & (tmax.astype(np.int64) - 1 < tm)
        if under.any():
            t = tuple(np.argwhere(under)[0])
            raise AssertionError("%s (b): %d lazy tiles' bound below their largest batch distance; first tile (tz, ty, tx) %s: tmax %d, true %d, "
                                 "tbmax %d, zstream %d" % (tag, int(under.sum()), t, tmax[t], tm[t], tbmax[t], st["zstream"]))
        exact = tlazy & (tbmax <= ZS_EXACT) if st["zstream"] else np.zeros_like(tlazy)
        n_exact, n_sampled = int(exact.sum()), int((tlazy & ~exact).sum())
    # (c) pass Z's streaming form's record of every tile's largest batch distance
    if st["zstream"] and tm is not None:
        wrong = (tbmax <= ZS_EXACT) & (tbmax != tm)
        if wrong.any():
            t = tuple(np.argwhere(wrong)[0])
            raise AssertionError("%s (c): %d tiles' tbmax <= 80 is not their largest batch distance; first tile (tz, ty, tx) %s: tbmax %d, true %d"
                                 % (tag, int(wrong.sum()), t, tbmax[t], tm[t]))
        low = (tm <= ZS_EXACT) & (tbmax < tm)
        assert not low.any(), "%s (c): %d tiles' tbmax below a largest batch distance <= 80" % (tag, int(low.sum()))
        ys, x16 = np.nonzero(st["zredo"])
        if len(ys):
            cols = np.zeros(tbmax.shape[1:], bool)                    # [ty][tx] columns of tiles that a given-up slab crosses
            for a in (0, 1):
                tx = 2 * x16 + a
                ok = tx < cols.shape[1]
                cols[ys[ok] >> 3, tx[ok]] = True
            n_redo81 = int(((tbmax > ZS_EXACT) & cols[None]).sum())
            assert n_redo81 > 0, "%s (c): slabs given up, but no tile of their columns holds 81 or more" % tag
    if tally is not None:
        tally.add(k, st, n_exact, n_sampled, int((tskip == 2).sum()), n_redo81)


def pin_host_edt(tag, true_d2, batch_dist_sq, brute=None):
    """the host EDT against the library's batch EDT of the same update (read after the tile state) and, on small grids, the brute force"""
    assert true_d2 is not None, tag
    assert np.array_equal(true_d2, batch_dist_sq.astype(np.int64)), "%s: host EDT differs from the batch EDT in %d voxels" % (
        tag, int((true_d2 != batch_dist_sq).sum()))
    if brute is not None:
        assert np.array_equal(true_d2, brute.astype(np.int64)), "%s: host EDT differs from the brute force" % tag


def check_definition(tag, m, mg=20):
    """test_oracle_edt.py::test_incremental_field_against_the_definition on the committed field of `m`: every known voxel's closest
    obstacle is believed occupied, at exactly the stored distance; the distance is never below the cKDTree truth over the believed
    occupied voxels around the volume, and equals it for > 99.5 % of the voxels whose nearest obstacle certainly lies in that region"""
    from scipy.spatial import cKDTree
    X, Y, Z = m.size
    r = m.read_local(edt=False)
    pv = np.array(m.pivot(), np.int64)
    gx, gy, gz = np.meshgrid(np.arange(-mg, X + mg), np.arange(-mg, Y + mg), np.arange(-mg, Z + mg), indexing="ij")
    reg = (np.stack([gx, gy, gz], -1).reshape(-1, 3) + pv).astype(np.int32)
    occ = reg[m.query_global(reg)["vox_type"] == 2]
    del reg, gx, gy, gz
    assert len(occ) > 50, tag
    known = (r["type"] != 0) & (r["dist_sq"] < 900000)
    zz, yy, xx = np.nonzero(known)
    vox = np.stack([xx, yy, zz], -1).astype(np.int64) + pv
    d = r["dist_sq"][known].astype(np.int64)
    coc = r["coc"][known].astype(np.int64)
    assert np.array_equal(((coc - vox) ** 2).sum(-1), d), "%s: a witness is not at the stored distance" % tag
    assert (m.query_global(coc.astype(np.int32))["vox_type"] == 2).all(), "%s: a witness is not believed occupied" % tag
    true_d, _ = cKDTree(occ).query(vox, workers=8)
    true_sq = np.rint(true_d ** 2).astype(np.int64)
    inside = true_sq <= (mg - 1) ** 2
    assert (d[inside] >= true_sq[inside]).all(), "%s: %d stored distances below the truth" % (tag, int((d[inside] < true_sq[inside]).sum()))
    frac = float((d[inside] == true_sq[inside]).mean())
    assert frac > 0.995, "%s: only %.4f of the stored distances equal the truth" % (tag, frac)
    return frac


def run_checked_drive(dr, make_a, make_b, brute_pin=False, definition=()):
    """every update: the oracle's and the mapper's local planes, stats and global probes (in and around the volume, and the slabs just
    left) bit for bit, then checks (a)-(c) on the mapper's tile state; the host EDT pinned at update dr.pin_at.  Returns the Tally."""
    import parity
    from oracle_py import brute_force_edt
    cfg = dr.config()
    a, b = make_a(cfg), make_b(cfg)
    rng = np.random.default_rng(dr.seed + 99)
    tally = Tally()
    prev = None
    try:
        for k, pos, q, kind, data, stream in dr.frames():
            tag = "%s update %d" % (dr.name, k)
            for m in (a, b):
                m.stream_enable(stream)
                m.update(pos, q, kind, data)
                if stream:
                    m.stream_changed()
            st = b.debug_tile_state()                  # (before anything reads the batch EDT: its completion reruns pass Z)
            ra, rb = a.read_local(), b.read_local()
            for key in ("type", "dist_sq", "coc"):
                assert np.array_equal(ra[key], rb[key]), "%s: %s differs in %d voxels" % (
                    tag, key, int((ra[key] != rb[key]).reshape(ra["type"].shape + (-1,)).any(-1).sum()))
            assert np.allclose(ra["edt"], rb["edt"], rtol=1e-6, atol=0.0), "%s: edt differs" % tag
            sa, sb = a.stats(), b.stats()
            for key in ("seeds_a", "seeds_b", "seeds_c", "levels_a", "levels_b", "levels_c", "visits_a", "visits_b", "visits_c", "blocks_total"):
                assert sa[key] == sb[key], "%s: stat %s %d != %d" % (tag, key, sa[key], sb[key])
            pvt = a.pivot()
            assert pvt == b.pivot()
            parity.compare_global(tag, a, b, parity.probe_coords(pvt, dr.size, rng, n=20000, margin=12))
            if prev is not None:
                parity.compare_global(tag + " (left behind)", a, b, parity.probe_left_behind(prev, pvt, dr.size, rng))
            prev = pvt
            true_d2 = host_batch_edt(rb["type"])
            check_update(tag, b, st, rb["type"], true_d2, tally, k)
            if k == dr.pin_at:
                pin_host_edt(tag, true_d2, b.read_batch_edt()["dist_sq"], brute_force_edt(rb["type"] == 2) if brute_pin else None)
            if k in definition:
                check_definition(tag, b)
    finally:
        a.close()
        b.close()
    return tally


# ---------------------------------------------------------------------------------------------------------- drives
class Drive:
    """A seeded map-update sequence of the hash world (bench.C5's parameters by default) with events:
    path:         "turn" (the bench's out-and-back: +step voxels in x per update, back after `turn` updates) or a list of per-update
                  displacements in voxels (any axis, any sign);
    jump:         {update: (dx, dy, dz)}: the robot jumps (off the block grid) before that update, and stays displaced;
    pocket:       (global voxel corner, side or (sx, sy, sz)): an obstacle-free box of the world;
    unobserved:   {update: (x0, x1)}: local x slab not observed in that update (its labels UNKNOWN);
    stream_on:    updates with the changed-block flags on (the reference's order of kernels instead of the fused sweep);
    lidar:        updates that take a ray-cast point cloud (occupied voxels of the world near the sensor) instead of labels;
    field:        None (the hash world) or a function (global x, y, z index grids) -> bool occupied."""

    def __init__(self, name, size, updates, voxel=0.05, path="turn", step=8, turn=24, jump=None, pocket=None, unobserved=None,
                 stream_on=(), lidar=(), field=None, seed=5, p_occ=0.01, toggle=0.25, cutoff_dist=2.0, definition_at=(), pin_at=1):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.jump, self.unobserved = jump or {}, unobserved or {}

    def config(self):
        import gie
        return gie.make_config(self.voxel, self.size, cutoff_dist=self.cutoff_dist)

    def position(self, k):
        """sensor voxel of update k"""
        if self.path == "turn":
            import bench
            at = np.array([bench.turn_index(k, self.turn) * self.step, 0, 0], np.int64)
        else:
            at = np.sum(np.asarray(self.path[:k], np.int64).reshape(-1, 3), axis=0)
        for j, d in self.jump.items():
            if k >= j:
                at = at + np.asarray(d, np.int64)
        return at

    def labels(self, k, pvt):
        X, Y, Z = self.size
        if self.field is None:
            lab = scenes.hash_world_labels(pvt, self.size, k, seed=self.seed, p_occ=self.p_occ, toggle_frac=self.toggle).astype(np.int8)
        else:
            gz, gy, gx = np.meshgrid(np.arange(Z) + pvt[2], np.arange(Y) + pvt[1], np.arange(X) + pvt[0], indexing="ij")
            lab = np.where(self.field(gx, gy, gz), 2, 1).astype(np.int8)
        if self.pocket is not None:
            c0, s = np.asarray(self.pocket[0]), np.broadcast_to(np.asarray(self.pocket[1]), (3,))
            lo = np.maximum(c0 - np.array(pvt), 0)
            hi = np.minimum(c0 + s - np.array(pvt), np.array([X, Y, Z]))
            if np.all(hi > lo):
                lab[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = 1
        if k in self.unobserved:
            x0, x1 = self.unobserved[k]
            lab[:, :, x0:x1] = 0
        return lab

    def frames(self):
        """per update: (k, pos, quat, kind, data, stream)"""
        w = np.float32(self.voxel)
        for k in range(self.updates):
            at = self.position(k)
            pos = tuple(np.float32(int(at[i]) * w) for i in range(3))
            q = (1.0, 0.0, 0.0, 0.0)
            pvt = scenes.local_pivot(pos, self.voxel, self.size)
            lab = self.labels(k, pvt)
            if k in self.lidar:
                # a ray-cast scan: the world's occupied voxels within 24 voxels of the sensor, as points at their centres
                zz, yy, xx = np.nonzero(lab == 2)
                loc = np.stack([xx, yy, zz], -1)
                near = np.abs(loc - np.array(self.size) // 2).max(-1) <= 24
                pts = ((loc[near] + np.array(pvt)) * w).astype(np.float32)
                yield k, pos, q, "pointcloud", np.ascontiguousarray(pts), k in self.stream_on
            else:
                yield k, pos, q, "labels", lab, k in self.stream_on


def edge_field(y0=0):
    """Bands in y (global y - y0, mod 96) of z-lines — every plane holds obstacles — whose tiles reach a largest batch distance^2 of
         82: lines at x = 0 mod 18, y even (in-plane |dx| = 9, |dy| = 1)          [0, 48)
         64: planes x = 0 mod 16 (|dx| = 8)                                     [48, 64)
         80: lines at x = 0 mod 16, y = 0 mod 8 (|dx| = 8, |dy| = 4)             [64, 80)
         81: planes x = 0 mod 18 (|dx| = 9)                                     [80, 96)
    the window edges of the fused form's key (|dx| <= 8) and both sides of GIE_ZS_LIMIT (81)."""
    def f(gx, gy, gz):
        yb = np.mod(gy - y0, 96)
        b82 = (yb < 48) & (np.mod(gx, 18) == 0) & (np.mod(yb, 2) == 0)
        b64 = (yb >= 48) & (yb < 64) & (np.mod(gx, 16) == 0)
        b80 = (yb >= 64) & (yb < 80) & (np.mod(gx, 16) == 0) & (np.mod(yb, 8) == 0)
        b81 = (yb >= 80) & (np.mod(gx, 18) == 0)
        return b82 | b64 | b80 | b81
    return f

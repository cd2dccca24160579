"""The batch EDT's selection rules, stated on the host, and the table of cases that pins every form they can select.

Plain Python and numpy, no GPU.  Written from the dispatch code, constant by constant:

  gie_edt_plan_for (executed by be_edt / be_edt_z, gie_hip.hip)                gie_edt_plan.h         what the host launches
  gie_zs_takes, gie_edt_x_row, gie_row_window, k_edt_z, k_edt_z_stream        gie_kernels.hip.h      what the device picks
  gie_z_use_lists                                                              gie_types.h
  gie_batch_edt (full = 0 where the volume is at most 64 tiles high)           gie_api.inc.h

Two kinds of statement:

* host_forms: the kernel names an update announces (GIE_TRACE_LAUNCHES).  The GPU test compares them with the trace.
* row_forms_x / column_forms_z / stream_outcome: which form the DEVICE takes for a row, a column, a volume.  No trace shows
  these, so the cases are built for the form to follow by construction, and the functions say how far from a border each
  decision is (`clear`): a case may only claim a form for rows / columns whose decision is clear, and stream_outcome refuses
  a volume whose outcome is not.

The windowed form (gie_row_window) is not restated trip by trip.  Its loop widens a window by four sites a trip and lets a
band of 64 positions go once every position of it holds a value below (W + 1)^2; the values only fall and the bound only
rises, so the band is let go by W = GIE_WIN_MAX at the latest if and only if
        v(u) = min over |i - u| <= 48 of (a_i + (u - i)^2)  <  49^2 = 2401        for every position u of the band,
and the row gives up otherwise.  A decision counts as clear when the worst v(u) is below 47^2 or at least 51^2.
"""
import functools

import numpy as np

BAND_MAXK = 160                     # GIE_BAND_MAXK, gie_kernels.hip.h: banded form up to this many sites
WIN_MAX = 48                        # GIE_WIN_MAX, gie_kernels.hip.h
WIN_OK = (WIN_MAX + 1) ** 2         # a band is let go below this value at W = GIE_WIN_MAX
WIN_CLEAR_LO = (WIN_MAX - 1) ** 2
WIN_CLEAR_HI = (WIN_MAX + 3) ** 2
ZS_R, ZS_C, ZS_R2 = 8, 16, 24       # GIE_ZS_R, GIE_ZS_C, GIE_ZS_R2: narrow window, planes per trip, wide window
ZS_LIMIT = (ZS_R + 1) ** 2          # the narrow trip is exact below 81 ...
ZS_LIMIT2 = (ZS_R2 + 1) ** 2        # ... the wide trip below 625
ZS_WAVES = 8                        # GIE_ZSTREAM_WAVES, gie_types.h
Z_LIST_DIV = 8                      # GIE_Z_LIST_DIV, gie_types.h
Z_SHORT_TILES = 8                   # GIE_Z_SHORT_LISTS: volumes at most this many tiles high always take the list form
PARTIAL_MAX_TILES = 64              # gie_batch_edt: full = 0 up to this many z tiles
CPS = (1, 2, 4, 8, 16)
NONE, LEFT, TOOK = 0, 1, 2          # GIE_EDT_HINT_*, gie_types.h: what an update is launched for
CU_TOTAL = 256                      # compute units of the device the suite runs on; stream_segments checks that it does not matter

Y_KERNELS = ("k_edt_y4<16>", "k_edt_y4<32>", "k_edt_y<8,8>", "k_edt_y<16,16>", "k_edt_y<32,16>")


def cp_of(L):
    """gie_edt_cp: the CP instantiation of a line of L voxels"""
    return 1 if L <= 64 else 2 if L <= 128 else 4 if L <= 256 else 8 if L <= 512 else 16


def pass_y_kernel(X, Y):
    """gie_edt_plan_for, pass Y: (kernel name, rows of a thread's share)"""
    if X % 4 == 0:
        return ("k_edt_y4<32>", 32) if Y > 512 else ("k_edt_y4<16>", 16)
    if Y <= 256:
        return "k_edt_y<8,8>", 32            # QW = YW / TPC = 1 mask word
    if Y <= 512:
        return "k_edt_y<16,16>", 32
    return "k_edt_y<32,16>", 64              # QW = 2


def zs_mode(X, Z, fused_switch=True):
    """gie_edt_zs_host: 0 = no streaming form, 1 = from pass X's planes (odd X, or GIE_ZS_FUSED=0), 2 = fused (even X)"""
    if Z < 64 or Z > 1024:
        return 0
    return 2 if fused_switch and X % 2 == 0 else 1


def tiles(size):
    X, Y, Z = size
    return (X + 7) // 8, (Y + 7) // 8, (Z + 7) // 8


def update_is_partial(size):
    """gie_batch_edt: full = 0"""
    return tiles(size)[2] <= PARTIAL_MAX_TILES


def z_use_lists(size, known_tiles, force=None):
    """gie_z_use_lists; force = GIE_TILE_LIST of the test build (None: unset)"""
    if force is not None:
        return bool(force)
    nx, ny, nz = tiles(size)
    if nz <= Z_SHORT_TILES:
        return True
    return known_tiles * Z_LIST_DIV <= nx * ny * nz


def zs_takes(size, planes_with_obstacles, known_tiles, full, force=None):
    """gie_zs_takes"""
    X, Y, Z = size
    return bool(zs_mode(X, Z)) and not (not full and z_use_lists(size, known_tiles, force)) and planes_with_obstacles > BAND_MAXK


def host_forms(size, planes_with_obstacles, known_tiles, full, completion=False, guess=NONE, fused_switch=True):
    """The kernel names of the batch EDT that gie_batch_edt (or, completion=True, the pass Z gie_read_batch_edt runs again with
    full = 1: be_edt_z) must announce, blanks removed.  The guess of a fresh mapper is NONE (be_edt_hint_take: the hint word is
    0), so pass X and k_edt_x_redo are both launched wherever the fused form may take the volume, and neither the planes with
    obstacles nor the known tiles change a launch: those two decide on the device (z_worker) which of the launched kernels
    does the pass.  They are arguments so that a call states the whole situation.
    guess: what the update is launched for ("the hint"); it counts only for an update of a volume the fused form may
    take.  TOOK: no pass X.  LEFT: the streaming form that reads pass X's planes, no k_edt_x_redo."""
    X, Y, Z = size
    zs = zs_mode(X, Z, fused_switch)
    if completion or zs != 2:
        guess = NONE
    if guess == LEFT:
        zs = 1
    out = set()
    if not completion:
        out.add(pass_y_kernel(X, Y)[0])
        if guess != TOOK:
            out.add("k_edt_x<%d>" % cp_of(X))
    if zs:
        out.add("k_edt_z_stream<true>" if zs == 2 else "k_edt_z_stream<false>")
        if zs == 2:
            out.add("k_edt_x_redo<%d>" % cp_of(X))
    elif not full and not completion:
        out.add("k_edt_z_direct")
    out.add("k_edt_z<%d,16,8>" % cp_of(Z))
    return out


def z_worker(size, planes_with_obstacles, known_tiles, full, force=None):
    """which launched kernel does pass Z: 'list' (gie_edt_z_direct_body, in its own kernel or in the streaming kernel's launch),
    'stream' (the column kernel behind it repairs the slabs given up) or 'column'"""
    if not full and z_use_lists(size, known_tiles, force):
        return "list"
    return "stream" if zs_takes(size, planes_with_obstacles, known_tiles, full, force) else "column"


# ---------------------------------------------------------------------------------------------------------- device forms
def _sq_along(occ, axis):
    """squared distance to the nearest True along `axis` (int64), and whether there is one"""
    o = np.moveaxis(occ, axis, 0)
    L = o.shape[0]
    far = 1 << 20
    d = np.empty(o.shape, np.int64)
    run = np.full(o.shape[1:], far, np.int64)
    for i in range(L):
        run = np.where(o[i], 0, run + 1)
        d[i] = run
    run = np.full(o.shape[1:], far, np.int64)
    for i in range(L - 1, -1, -1):
        run = np.where(o[i], 0, run + 1)
        d[i] = np.minimum(d[i], run)
    has = d < far
    return np.moveaxis(np.where(has, d * d, 0), 0, axis), np.moveaxis(has, 0, axis)


def _window_worst(a, has, need=None):
    """a, has: [..., L] values of the sites along the last axis.  The largest v(u) (module docstring) over the positions u that
    `need` marks (default: all); positions without a site inside the window count as 1 << 40."""
    L = a.shape[-1]
    none = np.int64(1) << 40
    val = np.where(has, a, none)
    pad = np.full(a.shape[:-1] + (WIN_MAX,), none, np.int64)
    ext = np.concatenate([pad, val, pad], axis=-1)
    v = np.full(a.shape, none, np.int64)
    for k in range(-WIN_MAX, WIN_MAX + 1):
        v = np.minimum(v, ext[..., WIN_MAX + k:WIN_MAX + k + L] + k * k)
    if need is not None:
        v = np.where(need, v, 0)
    return v.max(axis=-1)


def _window_verdict(worst):
    ok = worst < WIN_OK
    clear = (worst < WIN_CLEAR_LO) | (worst >= WIN_CLEAR_HI)
    return ok, clear


def row_forms_x(occ):
    """Pass X, gie_edt_x_row: per row (z, y) the form that takes it and whether that decision is clear.
    form[z][y] in 'skipped' (plane without obstacle: the row is left at the plane flag), 'banded', 'windowed', 'gives_up'
    (windowed, no bound inside GIE_WIN_MAX: the envelope takes it, which is divide & conquer since K > 160) and 'dnc'.
    The sites of a row are the columns of its plane that hold an obstacle, whatever y: the count decides per plane, the
    values (y - cy)^2 per row."""
    Z, Y, X = occ.shape
    cp = cp_of(X)
    a, has = _sq_along(occ, 1)
    form = np.empty((Z, Y), object)
    clear = np.ones((Z, Y), bool)
    for z in range(Z):
        kall = int(occ[z].any(axis=0).sum())
        if kall == 0:
            form[z, :] = "skipped"
        elif kall <= BAND_MAXK:
            form[z, :] = "banded"
        elif cp >= 4 and kall * 8 >= X * 7:
            ok, cl = _window_verdict(_window_worst(a[z], has[z]))
            form[z, :] = np.where(ok, "windowed", "gives_up")
            clear[z, :] = cl
        else:
            assert cp >= 4, "more than 160 sites need X > 160"
            form[z, :] = "dnc"
    return form, clear


def x_store_path(X):
    """gie_edt_x_row: how the envelope's results leave ('vec': 16-byte vectors, 'dword'); the banded and the windowed form
    store dwords themselves"""
    return "vec" if cp_of(X) >= 4 and X % 4 == 0 else "dword"


def _inplane_sq(occ):
    """per plane with obstacles the in-plane squared distance [Z][Y][X] (what pass X leaves), and the planes' flags"""
    from scipy import ndimage
    Z, Y, X = occ.shape
    has = occ.reshape(Z, -1).any(axis=1)
    a = np.zeros((Z, Y, X), np.int64)
    for z in np.nonzero(has)[0]:
        a[z] = np.rint(ndimage.distance_transform_edt(~occ[z]) ** 2).astype(np.int64)
    return a, has


def column_forms_z(occ, full=True, need=None):
    """The column kernel k_edt_z: per column (y, x) the form that takes it and whether that is clear.  'empty' (no obstacle
    in the volume), 'banded' (K <= 160 planes with obstacles), 'windowed', 'gives_up' (the envelope: divide & conquer), and
    'unread' (full = 0: no tile of the column has a reader).  need [tz][ty][tx]: the tiles with a reader (full = 0); the
    windowed form then only runs the 64-position bands with one."""
    Z, Y, X = occ.shape
    cp = cp_of(Z)
    a, has = _inplane_sq(occ)
    K = int(has.sum())
    form = np.empty((Y, X), object)
    clear = np.ones((Y, X), bool)
    if K == 0:
        form[:] = "empty"
    elif K <= BAND_MAXK:
        form[:] = "banded"
    else:
        assert cp >= 4, "more than 160 planes need Z > 160"
        av = np.moveaxis(a, 0, -1)                                       # [Y][X][Z]
        hv = np.broadcast_to(has, av.shape)
        needv = None
        if not full:
            assert Z <= 512
            vox = np.repeat(np.repeat(np.repeat(need, 8, 0), 8, 1), 8, 2)[:Z, :Y, :X]
            band = np.zeros((Z, Y, X), bool)
            for m in range(0, Z, 64):                                    # a band runs when any of its eight z tiles has a reader
                band[m:m + 64] = vox[m:m + 64].any(axis=0)
            needv = np.moveaxis(band, 0, -1)
        ok, cl = _window_verdict(_window_worst(av, hv, needv))
        form[:] = np.where(ok, "windowed", "gives_up")
        clear[:] = cl
    if not full:
        colneed = np.repeat(np.repeat(need.any(axis=0), 8, 0), 8, 1)[:Y, :X]
        form[~colneed] = "unread"
    return form, clear


def stream_segments(size, cu_total=CU_TOTAL):
    """gie_edt_plan_for, the streaming kernel: (number of z segments, their length).  The volumes of the table are small enough for the cap of one
    segment per 64 planes to bind on any device of 16 compute units or more, which is asserted."""
    X, Y, Z = size
    nxr = (X + 63) // 64

    def plan(cu):
        want = cu * 4 * ZS_WAVES
        nseg = (want + nxr * Y - 1) // (nxr * Y)
        nseg = max(1, min(nseg, max(Z // 64, 1)))
        seg_len = ((Z + nseg - 1) // nseg + 31) & ~31
        return (Z + seg_len - 1) // seg_len, seg_len
    assert plan(cu_total) == plan(16) == plan(1024), "the segments of this volume depend on the device"
    return plan(cu_total)


def edt_sq(occ):
    """exact squared distances of the whole volume (int64)"""
    from scipy import ndimage
    return np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.int64)


def stream_outcome(occ):
    """The streaming form k_edt_z_stream on a volume it takes (more than 160 planes with obstacles):
    dict(wide=trips that need the wide window > 0, given_up=set of the slabs (y, x // 64) given up).
    A narrow trip (16 planes of 64 columns) is exact where the distance is below 81 and needs the wide window otherwise; a
    slab (one z segment of the strip) is given up with a third such trip, or when a wide trip meets 625 or more.  Asserted
    margins: a trip's largest distance is at most 64 or at least 100; a slab is either given up for certain (three wide
    trips, or a trip with 729 or more: it fails as a wide trip or comes third) or kept for certain (at most two wide trips, none above 529)."""
    Z, Y, X = occ.shape
    assert int(occ.reshape(Z, -1).any(axis=1).sum()) > BAND_MAXK
    nseg, seg_len = stream_segments((X, Y, Z))
    d = edt_sq(occ)
    nxr = (X + 63) // 64
    wide_any = False
    given_up = set()
    for seg in range(nseg):
        z0, z1 = seg * seg_len, min(Z, (seg + 1) * seg_len)
        nwide = np.zeros((Y, nxr), int)
        sure_fail = np.zeros((Y, nxr), bool)
        sure_keep = np.ones((Y, nxr), bool)
        for zc in range(z0, z1, ZS_C):
            mx = np.stack([d[zc:min(zc + ZS_C, z1), :, 64 * r:64 * r + 64].max(axis=(0, 2)) for r in range(nxr)], axis=1)
            assert ((mx <= 64) | (mx >= 100)).all(), "a trip next to the narrow window's limit"
            nwide += mx >= ZS_LIMIT
            sure_fail |= mx >= 729
            sure_keep &= mx <= 529
        sure_keep &= nwide <= 2
        sure_fail |= nwide >= 3                            # (every wide trip counted is a clear one: asserted above)
        assert (sure_fail | sure_keep).all(), "a slab whose fate is not clear"
        wide_any |= bool((nwide > 0).any())
        given_up |= {(int(y), int(r)) for y, r in zip(*np.nonzero(sure_fail))}
    return dict(wide=wide_any, given_up=given_up)


# ---------------------------------------------------------------------------------------------------------- partial pass Z
def need_of_labels(labels):
    """the tiles [tz][ty][tx] that hold a known voxel (label 0 = not observed): the readers of a partial pass Z"""
    Z, Y, X = labels.shape
    nx, ny, nz = tiles((X, Y, Z))
    pad = np.zeros((nz * 8, ny * 8, nx * 8), bool)
    pad[:Z, :Y, :X] = labels != 0
    return pad.reshape(nz, 8, ny, 8, nx, 8).any(axis=(1, 3, 5))


def partial_conditions(size, need):
    """what keeps a partial case from passing vacuously, from the reader tiles alone (k_edt_z's nd0 / nd1 are the masks of the
    two 8-wide halves of a 16-column workgroup tile)"""
    nz, ny, nx = need.shape
    col = need.any(axis=0)
    out = {}
    out["needed and not needed in one tile column"] = bool((col & ~need.all(axis=0)).any())
    differ = second_only = False
    for tx in range(0, nx - 1, 2):
        a, b = need[:, :, tx], need[:, :, tx + 1]
        differ |= bool(((a != b).any(axis=0) & a.any(axis=0) & b.any(axis=0)).any() or (a.any(axis=0) != b.any(axis=0)).any())
        second_only |= bool((~a.any(axis=0) & b.any(axis=0)).any())
    out["halves of a workgroup tile differ"] = differ
    out["only the second half has readers"] = second_only
    out["first and last z tile needed"] = bool(need[0].any() and need[-1].any())
    if cp_of(size[2]) >= 4:
        nb = (nz + 7) // 8
        bands = np.stack([need[8 * m:8 * m + 8].any(axis=0) for m in range(nb)])      # [band][ty][tx]
        hole = False
        for m in range(1, nb - 1):
            hole |= bool((~bands[m] & bands[:m].any(axis=0) & bands[m + 1:].any(axis=0)).any())
        out["a band without a reader between two with one"] = hole
    return out


# ---------------------------------------------------------------------------------------------------------- pass Y patterns
Y_PATTERNS = ("full", "empty", "full_again", "y0", "ylast", "word_borders", "share_borders", "even_pairs", "long_gap")


def y_pattern(name, Y, share):
    """one column of pass Y [Y] bool.  share: the rows of a thread's share (pass_y_kernel)"""
    c = np.zeros(Y, bool)
    if name in ("full", "full_again"):
        c[:] = True
    elif name == "y0":
        c[0] = True
    elif name == "ylast":
        c[Y - 1] = True
    elif name == "word_borders":                       # both sides of every border of a 32-row mask word
        for k in range(32, Y, 32):
            c[k - 1] = c[k] = True
        if Y <= 32:
            c[Y // 2 - 1] = c[Y // 2] = True
    elif name == "share_borders":                      # both sides of every second border of a thread's share, and one row off it
        for k in range(share, Y, 2 * share):
            c[k - 1] = c[k] = True
            if k + share + 1 < Y:
                c[k + share + 1] = True
        if Y <= share:
            c[0] = c[Y - 1] = True
    elif name == "even_pairs":                         # even gaps: the midpoint ties and the larger y wins; gaps cross words and shares
        y, k, gaps = 1, 0, (2, 4, 6, 32, 64, 10, 30)
        while y < Y:
            c[y] = True
            y += gaps[k % len(gaps)]
            k += 1
    elif name == "long_gap":                           # the longest gap the column has room for (more than 512 where Y allows)
        c[min(2, Y - 1)] = True
        c[max(Y - 3, 0)] = True
    else:
        assert name == "empty"
    return c


def y_pattern_volume(X, Y):
    """One pattern per column, in the order of Y_PATTERNS over x then z (an empty column stands between two full ones), as
    many planes as that takes, and a last plane without any obstacle (its cy1 is never read)."""
    share = pass_y_kernel(X, Y)[1]
    npl = (len(Y_PATTERNS) + X - 1) // X
    occ = np.zeros((npl + 1, Y, X), bool)
    for z in range(npl):
        for x in range(X):
            occ[z, :, x] = y_pattern(Y_PATTERNS[(z * X + x) % len(Y_PATTERNS)], Y, share)
    return occ


def y_patterns_present(occ):
    """the patterns that stand in some column of the volume"""
    Z, Y, X = occ.shape
    share = pass_y_kernel(X, Y)[1]
    cols = {occ[z, :, x].tobytes() for z in range(Z) for x in range(X) if occ[z].any()}
    return {p for p in Y_PATTERNS if y_pattern(p, Y, share).tobytes() in cols}


# ---------------------------------------------------------------------------------------------------------- builders
def spread(X, k):
    """k columns of X, evenly"""
    assert k <= X
    return np.unique((np.arange(k) * X) // k)


def _x_thin(X, Y=6):
    """Pass X, thin in y and z: one plane per site pattern, obstacles of a plane in one row (every site of a row then has the
    same dy^2: wherever two sites are equally far in x they tie, and the smaller x must win)."""
    planes = [("one", np.array([X - 1])), ("none", np.array([], int)), ("all", np.arange(X)), ("alternate", np.arange(0, X, 2))]
    if X >= 161:
        planes += [("k160", spread(X, 160)), ("k161", spread(X, 161))]
        k78 = (7 * X + 7) // 8                                       # the fewest sites with 8 kall >= 7 X
        if k78 - 1 > BAND_MAXK:
            planes += [("thr78", spread(X, k78)), ("thr78_less", spread(X, k78 - 1))]
    if X - 120 >= (7 * X + 7) // 8:                                  # room for a 120-wide stretch without a site at 7 of 8 columns
        for g0 in (3, X // 2 - 60, X - 123):                         # in the first, a middle and the last band
            planes.append(("gap%d" % g0, np.concatenate([np.arange(g0), np.arange(g0 + 120, X)])))
    occ = np.zeros((len(planes), Y, X), bool)
    for z, (_, cols) in enumerate(planes):
        occ[z, (2 * z + 1) % Y, cols] = True
    return occ


def _x_tall(X, Y=56):
    """Pass X with every column a site in row 0: the rows far from it hold values above the window's reach (dy^2 >= 51^2 from
    y = 51 on) and give up, the rows near it do not; a second plane with 7 of 8 columns."""
    occ = np.zeros((2, Y, X), bool)
    occ[0, 0, :] = True
    occ[1, 0, spread(X, (7 * X + 7) // 8)] = True
    return occ


def _z_planes(Z, K, lattice=False, size_xy=(12, 12)):
    """(12, 12, Z): K planes with obstacles spread evenly, one obstacle a plane (or a 4-lattice in the plane)"""
    X, Y = size_xy
    occ = np.zeros((Z, Y, X), bool)
    for z in spread(Z, K):
        if lattice:
            occ[z, (z % 4)::4, ((z // 4) % 4)::4] = True
        else:
            occ[z, (5 * z) % Y, z % X] = True
    return occ


def _z_pocket(Z, pockets, size_xy=(24, 12), y0=0, ny=None):
    """An obstacle in every plane, all at x <= 3 (far columns hold large in-plane values), but for the planes of the pockets
    [(first plane, depth)]: the streaming form gives every slab up (distances of 625 and more), the column kernel repairs"""
    X, Y = size_xy
    ny = Y if ny is None else ny
    occ = np.zeros((Z, Y, X), bool)
    for z in range(Z):
        occ[z, y0 + (5 * z) % ny, z % 4] = True
    for p, depth in pockets:
        occ[p:p + depth] = False
    return occ


def _stream_field(X, Y, Z, boxes):
    """a lattice with obstacles in every plane, four apart, and boxes [(x0, y0, z0, sx, sy, sz)] without any"""
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    occ = (xx % 4 == zz % 4) & (yy % 4 == (zz // 4) % 4)
    for x0, y0, z0, sx, sy, sz in boxes:
        occ[z0:z0 + sz, y0:y0 + sy, x0:x0 + sx] = False
    return occ


def _partial_need(size, whole_slab=True):
    """The known tiles of a partial case [tz][ty][tx]: in tile column (0, 0) the first and the last z tile and every tile but
    those of the second band of eight; column (1, 0) none (the halves of workgroup tile 0 differ); column (1, 1) every second
    tile with column (0, 1) none (only the second half has readers); the last y row of tiles completely (more than an eighth
    of the volume: the column kernel's share by gie_z_use_lists)."""
    nx, ny, nz = tiles(size)
    need = np.zeros((nz, ny, nx), bool)
    need[:, 0, 0] = True
    need[8:16, 0, 0] = False
    need[0, 0, 0] = need[nz - 1, 0, 0] = True
    if nz <= 16:
        need[1:nz - 1:2, 0, 0] = False
    need[::2, 1, 1] = True
    if whole_slab:
        need[:, ny - 1, :] = True
    return need


def _labels(size, occ, need):
    """label feed: 0 outside the known tiles, 2 on the obstacles inside them, 1 elsewhere"""
    X, Y, Z = size
    vox = np.repeat(np.repeat(np.repeat(need, 8, 0), 8, 1), 8, 2)[:Z, :Y, :X]
    return np.where(vox, np.where(occ, 2, 1), 0).astype(np.int8)


def _sparse_field(size, zstep):
    """a few obstacles in every zstep-th plane, in every tile column"""
    X, Y, Z = size
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return (zz % zstep == 0) & (xx % 8 == (zz // zstep) % 8) & (yy % 8 == (3 * (zz // zstep)) % 8)


class Case:
    """name; group (one child process each on the GPU); size (X, Y, Z); occ() -> bool [Z][Y][X]; labels() for a partial case
    (int8 [Z][Y][X], else None); covers: the combinations the case is in the table for (test_edt_forms.py checks each claim
    against the functions above)"""

    def __init__(self, name, group, size, occ, covers, labels=None, conditions=True):
        self.name, self.group, self.size, self._occ, self.covers, self._labels, self.conditions = name, group, size, occ, set(covers), labels, conditions

    @property
    def partial(self):
        return self._labels is not None

    def labels(self):
        return self._labels() if self._labels else None

    def occ(self):
        """the obstacles the EDT sees (a partial case: the ones inside the known tiles)"""
        if self._labels:
            return self._labels() == 2
        o = self._occ()
        X, Y, Z = self.size
        assert o.shape == (Z, Y, X) and o.dtype == bool
        return o


def _make_cases():
    cases = []

    # pass Y: every kernel, every pattern
    for X, Y in [(5, 256), (5, 257), (67, 300), (130, 512), (7, 513), (67, 1024), (3, 1024),
                 (4, 16), (60, 17), (64, 512), (68, 513), (8, 1024)]:
        occ = functools.partial(y_pattern_volume, X, Y)
        Z = (len(Y_PATTERNS) + X - 1) // X + 1
        kern = pass_y_kernel(X, Y)[0]
        cov = {("y", kern)} | {("y_pattern", kern, p) for p in Y_PATTERNS}
        cases.append(Case("y_%dx%d" % (X, Y), "y", (X, Y, Z), occ, cov))

    # pass X: Z < 64, so no streaming form takes the rows
    for X in (64, 65, 128, 130, 254, 256, 258, 512, 514, 1024):
        cp, st = cp_of(X), x_store_path(X)
        cov = {("x", cp, "banded")}
        if X >= 254:
            cov |= {("x", cp, "windowed"), ("x", cp, "dnc", st)}
        if X == 1024:
            cov |= {("x", cp, "gives_up", st)}
        Z = _x_thin(X).shape[0]
        cases.append(Case("x_thin_%d" % X, "x", (X, 6, Z), functools.partial(_x_thin, X), cov))
    for X in (254, 256, 258, 512, 514, 1024):
        cp, st = cp_of(X), x_store_path(X)
        cases.append(Case("x_tall_%d" % X, "x", (X, 56, 2), functools.partial(_x_tall, X), {("x", cp, "windowed"), ("x", cp, "gives_up", st)}))

    # the column kernel under full = 1 (at most 160 planes with obstacles, or Z < 64)
    for Z in (63, 64, 65, 128, 129, 256, 257, 512, 513, 1024):
        K = min(Z, BAND_MAXK)
        cases.append(Case("z_%d_k%d" % (Z, K), "z", (12, 12, Z), functools.partial(_z_planes, Z, K), {("z", cp_of(Z), "banded")}))
    for Z in (64, 1024):
        cases.append(Case("z_%d_k1" % Z, "z", (12, 12, Z), functools.partial(_z_planes, Z, 1), {("z", cp_of(Z), "banded")}))
    cases.append(Case("z_256_k161", "z", (12, 12, 256), functools.partial(_z_planes, 256, 161, True), {("stream", True, "narrow")}))
    # ... and as the repair of the slabs the streaming form gives up: windowed (a pocket 70 planes deep) and the envelope
    # behind a window that gives up (95 planes at Z = 256, which keeps 161 planes with obstacles; 130 otherwise)
    for Z, deep in ((256, 95), (512, 130), (1024, 130)):
        cp = cp_of(Z)
        cases.append(Case("z_repair_%d_windowed" % Z, "zr", (24, 12, Z), functools.partial(_z_pocket, Z, [(Z // 2 - 20, 70)]),
                          {("z", cp, "windowed"), ("stream", True, "given_up")}))
        cases.append(Case("z_repair_%d_envelope" % Z, "zr", (24, 12, Z), functools.partial(_z_pocket, Z, [(Z // 2 - 20, deep)]),
                          {("z", cp, "gives_up"), ("stream", True, "given_up")}))

    # the streaming forms: even X (fused) and odd X, a partial 64-column strip, Z = 176 (no multiple of 32; two z segments, 96
    # and 80 planes); boxes without obstacles at the low z face and across the border of the segments
    for X in (130, 129):
        fused = X % 2 == 0
        for kind, boxes in (("narrow", [(20, 2, 0, 10, 10, 10), (90, 4, 91, 10, 10, 10)]),
                            ("wide", [(10, 0, 0, 20, 16, 20), (84, 0, 86, 20, 16, 20)]),
                            ("given_up", [(2, 0, 0, 60, 16, 60), (66, 0, 66, 60, 16, 60)])):
            cases.append(Case("stream_%d_%s" % (X, kind), "s", (X, 16, 176), functools.partial(_stream_field, X, 16, 176, boxes),
                              {("stream", fused, kind)}))

    # partial pass Z (full = 0) under a label feed
    def partial(name, size, field, covers, need=None, conditions=True):
        nd = functools.partial(_partial_need, size) if need is None else need
        lab = lambda: _labels(size, field(), nd())                    # noqa: E731
        cases.append(Case(name, "p", size, None, covers, labels=lab, conditions=conditions))
    partial("partial_40", (40, 24, 40), functools.partial(_sparse_field, (40, 24, 40), 2), {("partial", "list"), ("partial", "column", 1, "banded")})
    partial("partial_72", (40, 24, 72), functools.partial(_sparse_field, (40, 24, 72), 2), {("partial", "list"), ("partial", "column", 2, "banded")})
    partial("partial_200", (40, 24, 200), functools.partial(_sparse_field, (40, 24, 200), 2), {("partial", "list"), ("partial", "column", 4, "banded")})
    partial("partial_512", (24, 24, 512), functools.partial(_sparse_field, (24, 24, 512), 4), {("partial", "list"), ("partial", "column", 8, "banded")})

    def corner():
        need = np.zeros(tiles((40, 24, 72))[::-1], bool)
        need[-1, -1, -1] = True
        return need

    def corner_labels():
        lab = np.zeros((72, 24, 40), np.int8)
        lab[71, 23, 39] = 2
        return lab
    cases.append(Case("partial_corner_voxel", "p", (40, 24, 72), None, {("partial", "list")}, labels=corner_labels, conditions=False))
    # tall, more than 160 planes with obstacles inside the known tiles (the last y row of tiles): the streaming form runs under
    # full = 0, gives slabs up, and the column kernel repairs them under the reader masks
    for Z, deep in ((256, 95), (512, 130)):
        cp = cp_of(Z)
        size = (24, 24, Z)
        partial("partial_tall_%d_windowed" % Z, size, functools.partial(_z_pocket, Z, [(Z // 2 - 20, 70)], (24, 24), 16, 8),
                {("partial", "list"), ("partial", "repair", cp, "windowed")})
        partial("partial_tall_%d_envelope" % Z, size, functools.partial(_z_pocket, Z, [(Z // 2 - 20, deep)], (24, 24), 16, 8),
                {("partial", "list"), ("partial", "repair", cp, "gives_up")})
    return cases


CASES = _make_cases()
PARTIAL_MODES = (None, 0, 1)            # GIE_TILE_LIST unset, 0, 1

# The plan of the table, shape by shape: what each group is there to vary (a combination is often reached by several shapes —
# Y at both ends of a kernel's range, one strip and two, X a multiple of 4 and not — so the combinations alone would not miss a
# shape that left the table; this list does).
PLAN = (
    # pass Y, X % 4 != 0: a partial strip, two strips, lanes beyond X, Y at both ends of each kernel's range
    "y_5x256", "y_5x257", "y_67x300", "y_130x512", "y_7x513", "y_67x1024", "y_3x1024",
    # pass Y, X % 4 == 0
    "y_4x16", "y_60x17", "y_64x512", "y_68x513", "y_8x1024",
    # pass X: both ends of every CP's range, both store paths; rows that give up by their values at every CP >= 4
    "x_thin_64", "x_thin_65", "x_thin_128", "x_thin_130", "x_thin_254", "x_thin_256", "x_thin_258", "x_thin_512", "x_thin_514", "x_thin_1024",
    "x_tall_254", "x_tall_256", "x_tall_258", "x_tall_512", "x_tall_514", "x_tall_1024",
    # the column kernel under full = 1: both ends of every CP's range, 1 / 160 / 161 planes with obstacles, repair
    "z_63_k63", "z_64_k64", "z_65_k65", "z_128_k128", "z_129_k129", "z_256_k160", "z_257_k160", "z_512_k160", "z_513_k160", "z_1024_k160",
    "z_64_k1", "z_1024_k1", "z_256_k161",
    "z_repair_256_windowed", "z_repair_256_envelope", "z_repair_512_windowed", "z_repair_512_envelope", "z_repair_1024_windowed", "z_repair_1024_envelope",
    # the streaming forms
    "stream_130_narrow", "stream_130_wide", "stream_130_given_up", "stream_129_narrow", "stream_129_wide", "stream_129_given_up",
    # partial
    "partial_40", "partial_72", "partial_200", "partial_512", "partial_corner_voxel",
    "partial_tall_256_windowed", "partial_tall_256_envelope", "partial_tall_512_windowed", "partial_tall_512_envelope",
)


def case(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(dist_sq, coc) of a case's obstacles by the CPU oracle's EDT alone, computed once per process and shared (read only);
    test_edt_forms.py holds it against the closed form and the brute force before the GPU test compares a kernel with it"""
    import gie
    from oracle_py import OracleMapper
    c = case(name)
    m = OracleMapper(gie.make_config(0.1, c.size, cutoff_dist=1.0))
    try:
        d, coc = m.edt_only(np.where(c.occ(), 2, 1).astype(np.int8))
    finally:
        m.close()
    d.setflags(write=False)
    coc.setflags(write=False)
    return d, coc


# ---------------------------------------------------------------------------------------------------------- coverage
def required_and_impossible():
    """(required combinations, {impossible combination: the one-line reason})"""
    req, imp = set(), {}
    for k in Y_KERNELS:
        req.add(("y", k))
        for p in Y_PATTERNS:
            req.add(("y_pattern", k, p))
    for cp in CPS:
        req.add(("x", cp, "banded"))
        imp[("x", cp, "empty")] = "a row's sites are the columns of its plane that hold an obstacle, the same for every y: a plane without any is left at its plane flag before a row is read"
        for form in ("windowed", "dnc", "gives_up"):
            for st in ("vec", "dword"):
                key = ("x", cp, form) if form == "windowed" else ("x", cp, form, st)
                if cp <= 2:
                    imp[key] = ("the windowed form at CP < 4" if form != "dnc" else
                                "divide & conquer in pass X at CP <= 2, since more than 160 sites need X > 160")
                else:
                    req.add(key)
        req.add(("z", cp, "banded"))
        for form in ("windowed", "gives_up"):
            if cp <= 2:
                imp[("z", cp, form)] = "more than 160 planes with obstacles need Z > 160: at CP <= 2 the column kernel is always banded"
            else:
                req.add(("z", cp, form))
        imp[("z", cp, "dnc_direct")] = ("divide & conquer in the column kernel only behind a window that gave up: above 160 planes CP >= 4 always tries the window"
                                        if cp >= 4 else "more than 160 planes with obstacles need Z > 160")
    for fused in (True, False):
        for kind in ("narrow", "wide", "given_up"):
            req.add(("stream", fused, kind))
    req.add(("partial", "list"))
    for cp in CPS:
        if cp == 16:
            imp[("partial", "column", cp, "banded")] = "a volume more than 64 tiles high is never partial (gie_batch_edt)"
        else:
            req.add(("partial", "column", cp, "banded"))
        for form in ("windowed", "gives_up"):
            imp[("partial", "column", cp, form)] = ("above 160 planes with obstacles the column kernel runs on its own only where Z < 64, which has no 160 planes: "
                                                    "with full = 0 these forms run as repair alone")
            if cp in (4, 8):
                req.add(("partial", "repair", cp, form))
            else:
                imp[("partial", "repair", cp, form)] = ("more than 160 planes need Z > 160" if cp <= 2 else
                                                        "a volume more than 64 tiles high is never partial (gie_batch_edt)")
        imp[("partial", "repair", cp, "banded")] = "the streaming form takes a volume only above 160 planes with obstacles, where the column kernel is not banded"
    return req, imp


def derived_coverage(c, occ=None):
    """What a case provably reaches, from its occupancy through the functions above: only clear decisions count."""
    X, Y, Z = c.size
    occ = c.occ() if occ is None else occ
    K = int(occ.reshape(Z, -1).any(axis=1).sum())
    out = set()
    if c.partial:
        need = need_of_labels(c.labels())
        known = int(need.sum())
        for mode in PARTIAL_MODES:
            w = z_worker(c.size, K, known, 0, mode)
            if w == "list":
                out.add(("partial", "list"))
                continue
            if w == "column":
                form, clear = column_forms_z(occ, False, need)
                for f in set(form[clear].tolist()) - {"unread", "empty"}:
                    out.add(("partial", "column", cp_of(Z), f))
            else:
                so = stream_outcome(occ)
                form, clear = column_forms_z(occ, False, need)
                for y, r in so["given_up"]:
                    sl = (slice(y, y + 1), slice(64 * r, 64 * r + 64))
                    for f in set(form[sl][clear[sl]].tolist()) - {"unread", "empty"}:
                        out.add(("partial", "repair", cp_of(Z), f))
        return out
    kern = pass_y_kernel(X, Y)[0]
    out.add(("y", kern))
    for p in y_patterns_present(occ):
        out.add(("y_pattern", kern, p))
    if c.group in ("x",):
        assert Z < 64
        form, clear = row_forms_x(occ)
        for f in set(form[clear].tolist()) - {"skipped"}:
            out.add(("x", cp_of(X), f) if f in ("banded", "windowed") else ("x", cp_of(X), f, x_store_path(X)))
    if c.group in ("z", "zr", "s"):
        if z_worker(c.size, K, 0, 1) == "column":
            form, clear = column_forms_z(occ)
            for f in set(form[clear].tolist()):
                out.add(("z", cp_of(Z), f))
        else:
            so = stream_outcome(occ)
            fused = zs_mode(X, Z) == 2
            out.add(("stream", fused, "given_up" if so["given_up"] else "wide" if so["wide"] else "narrow"))
            if so["given_up"]:
                form, clear = column_forms_z(occ)
                for y, r in so["given_up"]:
                    sl = (slice(y, y + 1), slice(64 * r, 64 * r + 64))
                    for f in set(form[sl][clear[sl]].tolist()):
                        out.add(("z", cp_of(Z), f))
    return out

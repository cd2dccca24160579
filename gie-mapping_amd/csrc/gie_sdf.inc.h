/*
 * gie_sdf.inc.h — the signed distance field of the local volume and its interpolated queries (include/gie.h "signed distance").
 * HIP backend only: included by gie_hip.hip after gie_api.inc.h; nothing of the map update reads what is computed here.
 *
 * inside_dist_sq is cached per generation of the committed types (gie_mapper::type_gen) in three planes:
 *   occ    one bit per voxel, OCCUPIED or not: rows of ceil(X/64) 64-bit words, bit x & 63 of word x >> 6 (k_sdf_occ);
 *   inner  same layout: occupied voxels without an in-volume non-occupied face neighbour, the "interior" (k_sdf_inner);
 *   ids    int32 per voxel, read at interior voxels only: the exact squared distance, or -1 (k_sdf_line).
 * Everywhere else inside_dist_sq is settled by the bits: 0 off the obstacles, 1 on their surface.  The exact pass is a separable
 * EDT of the complement — pass X from the bit rows, lower envelopes along y and z (gie_row_argmin, the batch EDT's) — and runs
 * only when the device-side count of interior voxels is non-zero: the line kernels read the count and return at once otherwise,
 * so that no call has to wait for the host.
 */

/* bits of word k of a row that lie beyond the volume (k = W - 1 when X is not a multiple of 64) */
GIE_DEV uint64_t gie_sdf_pad(const int X, const int k, const int W)
{
    return (k == W - 1 && (X & 63)) ? (~0ull << (X & 63)) : 0ull;
}
struct gie_sdf_dev {
    uint64_t *occ, *inner;  /* W words per row (row = z * Y + y) */
    int32_t *ids;           /* N */
    int32_t *count;         /* interior voxels of the current generation */
    int W;
};

/* (a) the bit plane of OCCUPIED: one lane per voxel, a wave per 64-voxel word; the first lane of the grid zeroes the count (b) adds to */
__global__ __launch_bounds__(256) void k_sdf_occ(const gie_ctx c, const gie_sdf_dev s, const int nwords)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *s.count = 0;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane;
    const bool occ = x < c.X && c.glb_type[(size_t)row * c.X + x] == GIE_VOX_OCCUPIED;
    const unsigned long long b = __ballot(occ);
    if (lane == 0) s.occ[wd] = b;
}

/* (a) for X % 16 == 0: sixteen voxels per lane (one 16-byte load), four lanes per word — the byte-per-lane form above moves 64 bytes per
 * load instruction of a wave and ran at half the speed of the type plane's stream */
__global__ __launch_bounds__(256) void k_sdf_occ16(const gie_ctx c, const gie_sdf_dev s, const int nwords)
{
    const int g = blockIdx.x * 256 + threadIdx.x, wd = g >> 2, q = g & 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) *s.count = 0;
    uint64_t v = 0;
    if (wd < nwords) {
        const int row = wd / s.W, x = (wd - row * s.W) * 64 + q * 16;
        if (x < c.X) {
            const uint4 t = *reinterpret_cast<const uint4 *>(c.glb_type + (size_t)row * c.X + x);
            const uint32_t w4[4] = { t.x, t.y, t.z, t.w };
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) m |= (uint32_t)(((w4[k >> 2] >> (8 * (k & 3))) & 0xffu) == GIE_VOX_OCCUPIED) << k;
            v = (uint64_t)m << (16 * q);
        }
    }
    v |= (uint64_t)__shfl_xor((unsigned long long)v, 1);
    v |= (uint64_t)__shfl_xor((unsigned long long)v, 2);
    if (q == 0 && wd < nwords) s.occ[wd] = v;
}

/* (b) one lane per word: the interior bits (an out-of-volume neighbour counts as occupied), counted into *s.count */
__global__ __launch_bounds__(256) void k_sdf_inner(const gie_ctx c, const gie_sdf_dev s, const int nwords)
{
    const int wd = blockIdx.x * 256 + threadIdx.x, W = s.W;
    int n = 0;
    if (wd < nwords) {
        const int row = wd / W, wx = wd - row * W, y = row % c.Y, z = row / c.Y;
        const uint64_t o = s.occ[wd];
        uint64_t in = 0;
        if (o) {
            auto on = [&](int r, int k) { return s.occ[(size_t)r * W + k] | gie_sdf_pad(c.X, k, W); };
            const uint64_t o1 = o | gie_sdf_pad(c.X, wx, W);
            const uint64_t xm = (o1 << 1) | (wx > 0 ? on(row, wx - 1) >> 63 : 1ull);
            const uint64_t xp = (o1 >> 1) | (wx < W - 1 ? on(row, wx + 1) << 63 : 1ull << 63);
            const uint64_t ym = y > 0 ? on(row - 1, wx) : ~0ull, yp = y < c.Y - 1 ? on(row + 1, wx) : ~0ull;
            const uint64_t zm = z > 0 ? on(row - c.Y, wx) : ~0ull, zp = z < c.Z - 1 ? on(row + c.Y, wx) : ~0ull;
            in = o & xm & xp & ym & yp & zm & zp;
        }
        s.inner[wd] = in;
        n = __popcll(in);
    }
    for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(s.count, n);
}

/* pass X of the exact pass: squared distance from voxel x of a bit row to the nearest non-occupied voxel of that row, -1 if none */
GIE_DEV int gie_sdf_g1(const uint64_t *row, const int W, const int X, const int x)
{
    const int wx = x >> 6, b = x & 63;
    int best = 0x7fffffff;
    uint64_t f = ~row[wx] & ~gie_sdf_pad(X, wx, W) & (~0ull << b);          /* at or right of x (x itself is occupied) */
    if (f) best = wx * 64 + __builtin_ctzll(f) - x;
    else for (int k = wx + 1; k < W; k++) { f = ~row[k] & ~gie_sdf_pad(X, k, W); if (f) { best = k * 64 + __builtin_ctzll(f) - x; break; } }
    f = ~row[wx] & ~gie_sdf_pad(X, wx, W) & ((2ull << b) - 1ull);           /* at or left of x (b = 63: 2 << 63 wraps to 0, all bits) */
    if (f) best = min(best, x - (wx * 64 + 63 - __builtin_clzll(f)));
    else for (int k = wx - 1; k >= 0 && x - (k * 64 + 63) < best; k--) { f = ~row[k]; if (f) { best = min(best, x - (k * 64 + 63 - __builtin_clzll(f))); break; } }
    return best == 0x7fffffff ? -1 : best * best;
}

/* (c) one wave per line of the volume, lines with nothing to do skipped.
 *   AXIS 1 (lines along y at (x, z)): sites = pass X of every voxel of the line (0 off the obstacles), computed from the bit rows;
 *          the envelope is stored at the line's OCCUPIED voxels (-1: no site).  Lines without an occupied voxel are skipped.
 *   AXIS 2 (lines along z at (x, y)): sites = 0 off the obstacles, the AXIS 1 result on them; the envelope is stored at the line's
 *          INTERIOR voxels (-1: the volume holds no non-occupied voxel).  Lines without an interior voxel are skipped.
 * Keys of the envelope are ((u - i)² + a) << 10 | rank: a + L² < 2^22 holds for every side gie_create accepts. */
#define GIE_SDF_WAVES 4
template <int CP, int AXIS>
__global__ __launch_bounds__(64 * GIE_SDF_WAVES) void k_sdf_line(const gie_ctx c, const gie_sdf_dev s)
{
    if (*(const volatile int32_t *)s.count == 0) return;        /* no interior voxel: the bits have settled everything */
    constexpr int LP = 64 * CP;
    __shared__ __attribute__((aligned(16))) uint2 s_ce[GIE_SDF_WAVES][LP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, W = s.W, X = c.X, Y = c.Y;
    const int L = AXIS == 1 ? c.Y : c.Z;
    const int nlines = AXIS == 1 ? c.X * c.Z : c.X * c.Y;
    uint2 *ce = s_ce[wave];
    const int u0 = lane * CP;
#pragma unroll 1
    for (int line = blockIdx.x * GIE_SDF_WAVES + wave; line < nlines; line += gridDim.x * GIE_SDF_WAVES) {
        const int x = line % X, o = line / X, wx = x >> 6, b = x & 63;
        /* word of position i of the line (AXIS 1: row (o, i); AXIS 2: row (i, o)) and its voxel */
        auto wrow = [&](int i) { return AXIS == 1 ? (size_t)o * Y + i : (size_t)i * Y + o; };
        bool any = false;
        bool occ[CP];
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int i = 64 * m + lane;
            occ[m] = false;
            if (i < L) {
                const size_t wd = wrow(i) * W + wx;
                occ[m] = (s.occ[wd] >> b) & 1ull;
                any |= AXIS == 1 ? occ[m] : (bool)((s.inner[wd] >> b) & 1ull);
            }
        }
        if (!__any(any)) continue;                              /* wave-uniform */
        gie_wave_sync();                                        /* (the wave's site list is reused line after line) */
        int K = 0;
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int i = 64 * m + lane;
            int a = 0;
            if (i < L && occ[m]) a = AXIS == 1 ? gie_sdf_g1(s.occ + wrow(i) * W, W, X, x) : s.ids[wrow(i) * X + x];
            if (64 * m < L) K = gie_row_compact_push(ce, K, i < L && a >= 0, (uint32_t)a, i, 0u, lane);
        }
        gie_wave_sync();
        int sj[CP];
        if (K > 0) gie_row_argmin<CP>(ce, K, L, lane, sj);
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int u = u0 + m;
            if (u >= L) break;
            const size_t wd = wrow(u) * W + wx;
            const bool keep = AXIS == 1 ? (bool)((s.occ[wd] >> b) & 1ull) : (bool)((s.inner[wd] >> b) & 1ull);
            if (!keep) continue;
            int d = -1;
            if (K > 0) {
                const uint2 e = ce[sj[m]];
                const int i = (int)((e.y & 0xffffu) >> 5), du = u - i;
                d = du * du + (int)(e.x >> 10);
            }
            s.ids[wrow(u) * X + x] = d;
        }
    }
}

/* inside_dist_sq of voxel (x, y, z) = id, from the cache */
GIE_DEV int gie_sdf_ids(const gie_ctx &c, const gie_sdf_dev &s, const int x, const int y, const int z, const int id)
{
    const size_t wd = ((size_t)z * c.Y + y) * s.W + (x >> 6);
    const uint64_t bit = 1ull << (x & 63);
    if (!(s.occ[wd] & bit)) return 0;
    if (!(s.inner[wd] & bit)) return 1;
    return s.ids[id];
}
/* sdf(v) (include/gie.h): the positive EDT where inside_dist_sq <= 1, one voxel minus the inside distance deeper in */
GIE_DEV float gie_sdf_of(const gie_ctx &c, const int d, const int id)
{
    if (d < 0) return -(float)c.max_loc_dist_sq;
    if (d <= 1) return gie_edt_value(c, id);
    return 1.0f - sqrtf((float)d);
}

/* gie_read_sdf: one lane per voxel */
struct op_sdf_export {
    gie_sdf_dev s; float *sdf; int32_t *ids;
    GIE_DEV void operator()(const gie_ctx &c, int i) const {
        const int plane = c.X * c.Y, z = i / plane, r = i - z * plane, y = r / c.X, x = r - y * c.X;
        const int d = gie_sdf_ids(c, s, x, y, z, i);
        if (ids) ids[i] = d;
        if (sdf) sdf[i] = gie_sdf_of(c, d, i);
    }
};

/* gie_query_sdf: one lane per point; the eight corners are gathered unrolled (independent loads, in flight together) */
__global__ __launch_bounds__(256) void k_sdf_query(const gie_ctx c, const gie_sdf_dev s, const float *xyz, const int n, float *dist, float *grad, uint8_t *flags)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int S[3] = { c.X, c.Y, c.Z };
    int i0[3], i1[3];
    float t[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float u = xyz[3 * (size_t)p + k] / c.voxel_width - (float)c.pvt[k];
        i0[k] = i1[k] = 0; t[k] = 0.f;
        if (S[k] >= 2) {
            if (u >= 0.f && u <= (float)(S[k] - 1)) { i0[k] = min((int)floorf(u), S[k] - 2); i1[k] = i0[k] + 1; t[k] = u - (float)i0[k]; }
            else in = false;
        } else if (!(u >= -0.5f && u < 0.5f)) in = false;
    }
    if (!in) {
        if (dist) dist[p] = __builtin_nanf("");
        if (grad) { grad[3 * (size_t)p] = 0.f; grad[3 * (size_t)p + 1] = 0.f; grad[3 * (size_t)p + 2] = 0.f; }
        if (flags) flags[p] = 0;
        return;
    }
    float v[8];
    bool known = true, occ = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {                               /* corner k: x1 if bit 0, y1 if bit 1, z1 if bit 2 */
        const int x = (k & 1) ? i1[0] : i0[0], y = (k & 2) ? i1[1] : i0[1], z = (k & 4) ? i1[2] : i0[2];
        const int id = gie_lid(c, x, y, z);
        const int8_t ty = c.glb_type[id];
        known &= ty != GIE_VOX_UNKNOWN;
        occ |= ty == GIE_VOX_OCCUPIED;
        v[k] = gie_sdf_of(c, gie_sdf_ids(c, s, x, y, z, id), id);
    }
    const float tx = t[0], ty = t[1], tz = t[2], sx = 1.f - tx, sy = 1.f - ty, sz = 1.f - tz;
    const float c00 = v[0] * sx + v[1] * tx, c10 = v[2] * sx + v[3] * tx, c01 = v[4] * sx + v[5] * tx, c11 = v[6] * sx + v[7] * tx;
    const float c0 = c00 * sy + c10 * ty, c1 = c01 * sy + c11 * ty;
    if (dist) dist[p] = (c0 * sz + c1 * tz) * c.voxel_width;
    if (grad) {
        const float e0 = (v[1] - v[0]) * sy + (v[3] - v[2]) * ty, e1 = (v[5] - v[4]) * sy + (v[7] - v[6]) * ty;
        grad[3 * (size_t)p] = S[0] >= 2 ? e0 * sz + e1 * tz : 0.f;
        grad[3 * (size_t)p + 1] = S[1] >= 2 ? (c10 - c00) * sz + (c11 - c01) * tz : 0.f;
        grad[3 * (size_t)p + 2] = S[2] >= 2 ? c1 - c0 : 0.f;
    }
    if (flags) flags[p] = (uint8_t)(1u | (known ? 2u : 0u) | (occ ? 4u : 0u));
}

/* ---- host side */
/* a mapper that is (or will be, at its next pose) one tile of a larger volume: gie_set_tile with a non-zero offset or whole != local_size */
static bool gie_tiled(const gie_mapper *m)
{
    const gie_ctx &c = m->c;
    const int size[3] = { c.X, c.Y, c.Z };
    for (int i = 0; i < 3; i++)
        if ((m->has_pose && (c.tile_off[i] != 0 || c.whole_lo[i] != 0 || c.whole_hi[i] != size[i])) || m->next_off[i] != 0 || m->next_whole[i] != size[i]) return true;
    return false;
}
static int gie_sdf_check(gie_mapper *m, const char *who)
{
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) {
        gie_set_err(std::string(who) + ": not for a tiled mapper (its inside distances would stop at the tile's faces)");
        return GIE_ERR_INVALID;
    }
    return GIE_OK;
}
static gie_sdf_dev gie_sdf_view(const gie_mapper *m)
{
    gie_sdf_dev s;
    s.occ = m->sdf.occ; s.inner = m->sdf.inner; s.ids = m->sdf.ids; s.count = m->sdf.count; s.W = (m->c.X + 63) / 64;
    return s;
}
template <int CP> static void be_sdf_lines(be_state *b, const gie_ctx &c, const gie_sdf_dev &s)
{
    const int ny = c.X * c.Z, nz = c.X * c.Y, cap = b->cu_total * 16;
    GIE_LAUNCH(b, (k_sdf_line<CP, 1>), dim3(std::min((ny + GIE_SDF_WAVES - 1) / GIE_SDF_WAVES, cap)), dim3(64 * GIE_SDF_WAVES), 0, c, s);
    GIE_LAUNCH(b, (k_sdf_line<CP, 2>), dim3(std::min((nz + GIE_SDF_WAVES - 1) / GIE_SDF_WAVES, cap)), dim3(64 * GIE_SDF_WAVES), 0, c, s);
}
/* the inside distances of the current generation of types: allocated at the first call, recomputed after a type change */
static int gie_sdf_ready(gie_mapper *m, const char *who)
{
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of the readers) */
    const int W = (c.X + 63) / 64, nwords = W * c.Y * c.Z;
    if (!m->sdf.occ) {
        uint64_t *bits = gie_dalloc<uint64_t>(m, 2 * (size_t)nwords, false);
        int32_t *ids = bits ? gie_dalloc<int32_t>(m, (size_t)c.N, false) : nullptr;
        int32_t *cnt = ids ? gie_dalloc<int32_t>(m, 1, false) : nullptr;
        if (!cnt) { gie_set_err(std::string(who) + ": device allocation of the signed distance planes failed"); return GIE_ERR_DEVICE; }
        m->sdf.occ = bits; m->sdf.inner = bits + nwords; m->sdf.ids = ids; m->sdf.count = cnt;
        m->sdf.gen = m->type_gen - 1;
    }
    if (m->sdf.gen == m->type_gen) return GIE_OK;
    const gie_sdf_dev s = gie_sdf_view(m);
    be_prof(&m->be, GIE_K_SDF, 0);
    if ((c.X & 15) == 0) GIE_LAUNCH(&m->be, k_sdf_occ16, dim3((nwords + 63) / 64), dim3(256), 0, c, s, nwords);
    else GIE_LAUNCH(&m->be, k_sdf_occ, dim3((nwords + 3) / 4), dim3(256), 0, c, s, nwords);
    GIE_LAUNCH(&m->be, k_sdf_inner, dim3((nwords + 255) / 256), dim3(256), 0, c, s, nwords);
    const int L = std::max(c.Y, c.Z);
    if (L <= 64) be_sdf_lines<1>(&m->be, c, s);
    else if (L <= 128) be_sdf_lines<2>(&m->be, c, s);
    else if (L <= 256) be_sdf_lines<4>(&m->be, c, s);
    else if (L <= 512) be_sdf_lines<8>(&m->be, c, s);
    else be_sdf_lines<16>(&m->be, c, s);
    be_prof(&m->be, GIE_K_SDF, 1);
    m->sdf.gen = m->type_gen;
    return GIE_OK;
}

extern "C" int gie_read_sdf_dev(gie_mapper *m, float *d_sdf, int32_t *d_inside_dist_sq)
{
    int rc = gie_sdf_check(m, "gie_read_sdf_dev"); if (rc) return rc;
    if (!d_sdf && !d_inside_dist_sq) { gie_set_err("gie_read_sdf_dev: both outputs are null"); return GIE_ERR_INVALID; }
    rc = gie_sdf_ready(m, "gie_read_sdf_dev"); if (rc) return rc;
    gie_ctx c = m->c;
    c.gate = nullptr;
    op_sdf_export op; op.s = gie_sdf_view(m); op.sdf = d_sdf; op.ids = d_inside_dist_sq;
    be_prof(&m->be, GIE_K_SDF, 0);
    be_lin(&m->be, c, op, c.N);
    be_prof(&m->be, GIE_K_SDF, 1);
    return GIE_OK;
}
extern "C" int gie_read_sdf(gie_mapper *m, float *sdf, int32_t *inside_dist_sq)
{
    int rc = gie_sdf_check(m, "gie_read_sdf"); if (rc) return rc;
    if (!sdf && !inside_dist_sq) return gie_sync(m);
    const size_t N = (size_t)m->c.N;
    float *ds = sdf ? (float *)gie_scratch(m, 0, N * 4, "gie_read_sdf") : nullptr;
    int32_t *di = inside_dist_sq ? (int32_t *)gie_scratch(m, 1, N * 4, "gie_read_sdf") : nullptr;
    if ((sdf && !ds) || (inside_dist_sq && !di)) return GIE_ERR_DEVICE;
    rc = gie_read_sdf_dev(m, ds, di); if (rc) return rc;
    if (ds) be_d2h(&m->be, sdf, ds, N * 4);
    if (di) be_d2h(&m->be, inside_dist_sq, di, N * 4);
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_query_sdf_dev(gie_mapper *m, const float *d_xyz, int n, float *d_dist, float *d_grad, uint8_t *d_flags)
{
    int rc = gie_sdf_check(m, "gie_query_sdf_dev"); if (rc) return rc;
    if (n < 0 || (n > 0 && !d_xyz) || (!d_dist && !d_grad && !d_flags)) { gie_set_err("gie_query_sdf_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    rc = gie_sdf_ready(m, "gie_query_sdf_dev"); if (rc) return rc;
    gie_ctx c = m->c;
    c.gate = nullptr;
    be_prof(&m->be, GIE_K_SDF_QUERY, 0);
    GIE_LAUNCH(&m->be, k_sdf_query, dim3((n + 255) / 256), dim3(256), 0, c, gie_sdf_view(m), d_xyz, n, d_dist, d_grad, d_flags);
    be_prof(&m->be, GIE_K_SDF_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_query_sdf(gie_mapper *m, const float *xyz, int n, float *dist, float *grad, uint8_t *flags)
{
    int rc = gie_sdf_check(m, "gie_query_sdf"); if (rc) return rc;
    if (n < 0 || (n > 0 && !xyz) || (!dist && !grad && !flags)) { gie_set_err("gie_query_sdf: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    /* one export buffer: points (12 B) in the first, results (dist 4 + grad 12 + flags 1 B per point) in the second */
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 12, "gie_query_sdf");
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 17, "gie_query_sdf");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    float *dd = (float *)dr, *dg = (float *)(dr + (size_t)n * 4);
    uint8_t *df = (uint8_t *)(dr + (size_t)n * 16);
    be_h2d(&m->be, dx, xyz, (size_t)n * 12);
    rc = gie_query_sdf_dev(m, dx, n, dist ? dd : nullptr, grad ? dg : nullptr, flags ? df : nullptr); if (rc) return rc;
    if (dist) be_d2h(&m->be, dist, dd, (size_t)n * 4);
    if (grad) be_d2h(&m->be, grad, dg, (size_t)n * 12);
    if (flags) be_d2h(&m->be, flags, df, (size_t)n);
    gie_scratch_trim(m);
    return gie_sync(m);
}

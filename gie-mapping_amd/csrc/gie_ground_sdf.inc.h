/*
 * gie_ground_sdf.inc.h — the ground signed distance field: inside distances on the obstacle columns of the ground field, bilinear
 * distance / gradient queries and the clearance of whole trajectories (include/gie.h "ground signed distance").
 * HIP backend only: included by gie_hip.hip after gie_ground_pose_nf1.inc.h.  It reads the ground field's bit rows, its type and
 * dist_sq planes and writes nothing of the map or of that field; its own plane is one int32 per CELL and one count, allocated at the
 * first call of the section and recomputed at the first call after a gie_ground_compute*.
 *   k_gsdf_inner       the gate: one lane per 64-bit word of the bit rows, the word above and below and a carry bit from the words
 *                      left and right (k_sdf_inner's rule in the plane: outside the rectangle counts as an obstacle); the interior
 *                      obstacle columns are counted, per wave one atomic.  Nothing but the count is kept.
 *   k_gsdf_line        the exact transform of the complement, one wave per x (k_ground_line's shape, beside it: that kernel is
 *                      unchanged).  A site of the line is a row y with a column that is no obstacle: its value the squared distance
 *                      from x to the nearest clear bit of that row (gie_sdf_g1: the scan of the complemented row, the padding bits
 *                      of the last word masked); the lower envelope over the rows (gie_row_compact_push, gie_row_argmin) is stored
 *                      at the line's obstacle columns only, -1 when the rectangle holds no site.  With a count of 0 it returns at
 *                      once — the decision is taken on the device — and lines without an obstacle column are skipped.
 *                      Keys of the envelope are ((u - i)² + a) << 10 | rank: a + Y² < X² + Y² < 2^22 for every size gie_create accepts.
 *   exports, queries   one lane per cell (k_lin) or point (k_gsdf_query).
 *   k_gsdf_rollouts    a wave per trajectory, four per workgroup, a lane per point in chunks of 64 (k_ground_rollouts' shape): the
 *                      query of the lane's point, one ballot per chunk for the end of the prefix, and ONE set of wave reductions
 *                      after the loop on (dist, index) pairs and integers.  No sum of floats: no result depends on lane order.
 * The inside pass is one memset of the count and two launches: no grid barrier, no loop whose trip count depends on device data but
 * the scans of a bit row, no scratch.  The compiler's figures and the times are in DESIGN.md 30.
 */

#define GIE_GSDF_PER_LAUNCH (1ll << 24)     /* trajectories of one launch: 2^22 workgroups */

struct gie_gsdf_dev {
    int32_t *ids;           /* X * Y, read at obstacle columns and only when *count != 0 */
    int32_t *count;         /* interior obstacle columns of the field */
};

/* (a) the gate: one lane per word */
__global__ __launch_bounds__(256) void k_gsdf_inner(const gie_ctx c, const gie_ground_dev g, const gie_gsdf_dev s, const int nwords)
{
    const int wd = blockIdx.x * 256 + threadIdx.x, W = g.W;
    int n = 0;
    if (wd < nwords) {
        const int y = wd / W, wx = wd - y * W;
        const uint64_t o = g.obs[wd];
        if (o) {
            auto on = [&](int r, int k) { return g.obs[(size_t)r * W + k] | gie_sdf_pad(c.X, k, W); };
            const uint64_t o1 = o | gie_sdf_pad(c.X, wx, W);
            const uint64_t xm = (o1 << 1) | (wx > 0 ? on(y, wx - 1) >> 63 : 1ull);
            const uint64_t xp = (o1 >> 1) | (wx < W - 1 ? on(y, wx + 1) << 63 : 1ull << 63);
            const uint64_t ym = y > 0 ? on(y - 1, wx) : ~0ull, yp = y < c.Y - 1 ? on(y + 1, wx) : ~0ull;
            n = __popcll(o & xm & xp & ym & yp);
        }
    }
    for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(s.count, n);
}

/* (b) one wave per line along y at x */
template <int CP>
__global__ __launch_bounds__(64 * GIE_SDF_WAVES) void k_gsdf_line(const gie_ctx c, const gie_ground_dev g, const gie_gsdf_dev s)
{
    if (*(const volatile int32_t *)s.count == 0) return;        /* no interior column: the bit rows have settled everything */
    constexpr int LP = 64 * CP;
    __shared__ __attribute__((aligned(16))) uint2 s_ce[GIE_SDF_WAVES][LP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, W = g.W, X = c.X, Y = c.Y;
    __shared__ uint64_t s_col[GIE_SDF_WAVES][CP];               /* the line's obstacle bits, row 64 m + l at bit l of word m */
    uint2 *ce = s_ce[wave];
    const int u0 = lane * CP;
#pragma unroll 1
    for (int x = blockIdx.x * GIE_SDF_WAVES + wave; x < X; x += gridDim.x * GIE_SDF_WAVES) {
        const int wx = x >> 6, b = x & 63;
        gie_wave_sync();                                        /* (the wave's site list and column bits are reused line after line) */
        uint64_t any = 0;
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int i = 64 * m + lane;
            const uint64_t col = __ballot(i < Y && ((g.obs[(size_t)i * W + wx] >> b) & 1ull));
            if (lane == 0) s_col[wave][m] = col;
            any |= col;
        }
        if (!any) continue;                                     /* wave-uniform: no obstacle column on this line, nothing is read here */
        int K = 0;
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int i = 64 * m + lane;
            const int a = i < Y ? gie_sdf_g1(g.obs + (size_t)i * W, W, X, x) : -1;
            if (64 * m < Y) K = gie_row_compact_push(ce, K, a >= 0, (uint32_t)a, i, 0u, lane);
        }
        gie_wave_sync();
        int sj[CP];
        if (K > 0) gie_row_argmin<CP>(ce, K, Y, lane, sj);      /* (K is the same in all lanes) */
        const uint64_t mine = s_col[wave][u0 >> 6] >> (u0 & 63); /* the lane's CP rows lie in one word: CP divides 64 */
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int u = u0 + m;
            if (u >= Y) break;
            if (!((mine >> m) & 1ull)) continue;
            int d = -1;
            if (K > 0) {
                const uint2 e = ce[sj[m]];
                const int i = (int)((e.y & 0xffffu) >> 5), du = u - i;
                d = du * du + (int)(e.x >> 10);
            }
            s.ids[(size_t)u * X + x] = d;
        }
    }
}

/* inside_dist_sq of cell (x, y) = id, from the bit row and the cache */
GIE_DEV int gie_gsdf_ids(const gie_ground_dev &g, const gie_gsdf_dev &s, const bool flat, const int x, const int y, const int id)
{
    if (!((g.obs[(size_t)y * g.W + (x >> 6)] >> (x & 63)) & 1ull)) return 0;
    return flat ? 1 : s.ids[id];
}
/* gsdf (include/gie.h): gie_read_costmap_ground's d where inside_dist_sq <= 1, one cell minus the inside distance deeper in */
GIE_DEV float gie_gsdf_of(const gie_ctx &c, const gie_ground_dev &g, const bool none, const int d, const int id)
{
    if (d < 0) return -(float)c.max_loc_dist_sq;
    if (d <= 1) return none ? (float)c.max_loc_dist_sq : sqrtf((float)g.dist[id]);
    return 1.0f - sqrtf((float)d);
}

/* gie_read_ground_sdf: one lane per cell */
struct op_gsdf_export {
    gie_ground_dev g; gie_gsdf_dev s; float *sdf; int32_t *ids;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int y = i / c.X, x = i - y * c.X;
        const int d = gie_gsdf_ids(g, s, *(const volatile int32_t *)s.count == 0, x, y, i);
        if (ids) ids[i] = d;
        if (sdf) sdf[i] = gie_gsdf_of(c, g, gie_ground_nobs(g) == 0, d, i);
    }
};

/* the query of one point (include/gie.h: the order of the operations is part of the contract); false outside the rectangle, and
 * then dist = NaN, grad = 0, 0, flags = 0 */
GIE_DEV bool gie_gsdf_point(const gie_ctx &c, const gie_ground_dev &g, const gie_gsdf_dev &s, const bool none, const bool flat, const float px, const float py,
                            float &dist, float grad[2], uint32_t &flags)
{
    const int S[2] = { c.X, c.Y };
    const float p[2] = { px, py };
    int i0[2], i1[2];
    float t[2];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float u = p[k] / c.voxel_width - (float)g.pvt[k];
        i0[k] = i1[k] = 0; t[k] = 0.f;
        if (S[k] >= 2) {
            if (u >= 0.f && u <= (float)(S[k] - 1)) { i0[k] = min((int)floorf(u), S[k] - 2); i1[k] = i0[k] + 1; t[k] = u - (float)i0[k]; }
            else in = false;
        } else if (!(u >= -0.5f && u < 0.5f)) in = false;
    }
    if (!in) { dist = __builtin_nanf(""); grad[0] = grad[1] = 0.f; flags = 0; return false; }
    float v[4];
    bool known = true, obs = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {                               /* corner k: x1 if bit 0, y1 if bit 1 */
        const int x = (k & 1) ? i1[0] : i0[0], y = (k & 2) ? i1[1] : i0[1], id = y * c.X + x;
        const int d = gie_gsdf_ids(g, s, flat, x, y, id);
        known &= g.type[id] != GIE_VOX_UNKNOWN;
        obs |= (bool)((g.obs[(size_t)y * g.W + (x >> 6)] >> (x & 63)) & 1ull);
        v[k] = gie_gsdf_of(c, g, none, d, id);
    }
    const float tx = t[0], ty = t[1], sx = 1.f - tx, sy = 1.f - ty;
    const float c0 = v[0] * sx + v[1] * tx, c1 = v[2] * sx + v[3] * tx;
    dist = (c0 * sy + c1 * ty) * c.voxel_width;
    grad[0] = S[0] >= 2 ? (v[1] - v[0]) * sy + (v[3] - v[2]) * ty : 0.f;
    grad[1] = S[1] >= 2 ? c1 - c0 : 0.f;
    flags = 1u | (known ? 2u : 0u) | (obs ? 4u : 0u);
    return true;
}

/* gie_ground_query_sdf: one lane per point; the four corners are gathered unrolled */
__global__ __launch_bounds__(256) void k_gsdf_query(const gie_ctx c, const gie_ground_dev g, const gie_gsdf_dev s, const float *xy, const int n, float *dist, float *grad, uint8_t *flags)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    float d, gr[2];
    uint32_t f;
    gie_gsdf_point(c, g, s, gie_ground_nobs(g) == 0, *(const volatile int32_t *)s.count == 0, xy[2 * (size_t)p], xy[2 * (size_t)p + 1], d, gr, f);
    if (dist) dist[p] = d;
    if (grad) { grad[2 * (size_t)p] = gr[0]; grad[2 * (size_t)p + 1] = gr[1]; }
    if (flags) flags[p] = (uint8_t)f;
}

/* gie_ground_sdf_rollouts: a wave per trajectory, a lane per point in chunks of 64 */
__global__ __launch_bounds__(256) void k_gsdf_rollouts(const gie_ctx c, const gie_ground_dev g, const gie_gsdf_dev s, const float *xy, const long long first, const long long n,
                                                       const int T, const float margin, gie_ground_sdf_rollout *out, float *dist, float *grad)
{
    const long long i = first + (long long)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                                         /* wave-uniform */
    const float *pts = xy + 2 * (size_t)i * T;
    const bool none = gie_ground_nobs(g) == 0, flat = *(const volatile int32_t *)s.count == 0;
    const int NOK = 0x7fffffff;
    float bd = 0.f, bg[2] = { 0.f, 0.f };                       /* this lane's running values: its points of every chunk below the end */
    int bk = NOK, below = NOK, in0 = NOK, nb = 0;
    int m = 0;                                                  /* the same in all lanes */
    bool open = true;                                           /* the prefix has not ended: the same in all lanes */
#pragma unroll 1
    for (int base = 0; base < T; base += 64) {                  /* base, f and open steer the loop: wave-uniform */
        const int k = base + lane;
        float d = 0.f, gr[2] = { 0.f, 0.f };
        uint32_t fl = 0;
        if (k < T) {
            gie_gsdf_point(c, g, s, none, flat, pts[2 * k], pts[2 * k + 1], d, gr, fl);
            if (dist) dist[(size_t)i * T + k] = d;
            if (grad) { grad[2 * ((size_t)i * T + k)] = gr[0]; grad[2 * ((size_t)i * T + k) + 1] = gr[1]; }
        }
        if (open) {
            const uint64_t bad = __ballot(!(fl & 1u));          /* (a lane with k >= T has no flag) */
            const int f = bad ? (int)__builtin_ctzll(bad) : 64;
            if (lane < f) {
                if (bk == NOK || d < bd) { bd = d; bk = k; bg[0] = gr[0]; bg[1] = gr[1]; }      /* (k rises from chunk to chunk: the first of equals stays) */
                if (d < margin) { nb++; below = below < k ? below : k; }
                if (d <= 0.f) in0 = in0 < k ? in0 : k;
            }
            m = base + f;
            open = f == 64;
        }
        if (!open && !dist && !grad) break;                     /* (with per-point outputs the points behind the prefix are still answered) */
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                          /* (dist, index): the float first, then the index */
        const float od = __shfl_xor(bd, o);
        const int ok = __shfl_xor(bk, o);
        if (ok != NOK && (bk == NOK || od < bd || (od == bd && ok < bk))) { bd = od; bk = ok; }
    }
    below = gie_grol_min32(below);
    in0 = gie_grol_min32(in0);
    nb = gie_grol_sum32(nb);
    const int src = bk == NOK ? 0 : (bk & 63);                  /* the lane whose running value is the winner: point bk is its own */
    const float g0 = __shfl(bg[0], src), g1 = __shfl(bg[1], src);
    if (lane == 0) {
        gie_ground_sdf_rollout r;
        r.points = m;
        r.argmin = m > 0 ? bk : -1;
        r.min_dist = m > 0 ? bd : __builtin_nanf("");
        r.grad[0] = m > 0 ? g0 : 0.f; r.grad[1] = m > 0 ? g1 : 0.f;
        r.first_below = below == NOK ? -1 : below;
        r.n_below = nb;
        r.first_in = in0 == NOK ? -1 : in0;
        out[i] = r;
    }
}

/* ---- host side */
static gie_gsdf_dev gie_gsdf_view(const gie_mapper *m)
{
    gie_gsdf_dev s;
    s.ids = m->gsdf.ids; s.count = m->gsdf.ids + (size_t)m->c.X * m->c.Y;
    return s;
}
template <int CP> static void be_gsdf_lines(be_state *b, const gie_ctx &c, const gie_ground_dev &g, const gie_gsdf_dev &s)
{
    GIE_LAUNCH(b, k_gsdf_line<CP>, dim3(std::min((c.X + GIE_SDF_WAVES - 1) / GIE_SDF_WAVES, b->cu_total * 16)), dim3(64 * GIE_SDF_WAVES), 0, c, g, s);
}
/* the inside distances of the current ground field: allocated at the first call, recomputed after a gie_ground_compute* */
static int gie_gsdf_ready(gie_mapper *m, const char *who)
{
    static_assert(sizeof(gie_ground_sdf_rollout_param) == 32 && sizeof(gie_ground_sdf_rollout) == 32, "the sizes include/gie.h states");
    if (!m->gsdf.ids) {
        m->gsdf.ids = gie_dalloc<int32_t>(m, (size_t)m->c.X * m->c.Y + 1, false);
        if (!m->gsdf.ids) { gie_set_err(std::string(who) + ": device allocation of the ground signed distance plane failed"); return GIE_ERR_DEVICE; }
        m->gsdf.valid = 0;
    }
    if (m->gsdf.valid) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const gie_gsdf_dev s = gie_gsdf_view(m);
    const int nwords = g.W * c.Y;
    be_prof(&m->be, GIE_K_GROUND, 0);
    be_memset(&m->be, s.count, 0, sizeof(int32_t));
    GIE_LAUNCH(&m->be, k_gsdf_inner, dim3((nwords + 255) / 256), dim3(256), 0, c, g, s, nwords);
    if (c.Y <= 64) be_gsdf_lines<1>(&m->be, c, g, s);
    else if (c.Y <= 128) be_gsdf_lines<2>(&m->be, c, g, s);
    else if (c.Y <= 256) be_gsdf_lines<4>(&m->be, c, g, s);
    else if (c.Y <= 512) be_gsdf_lines<8>(&m->be, c, g, s);
    else be_gsdf_lines<16>(&m->be, c, g, s);
    be_prof(&m->be, GIE_K_GROUND, 1);
    m->gsdf.valid = 1;
    return GIE_OK;
}

extern "C" int gie_read_ground_sdf_dev(gie_mapper *m, float *d_sdf, int32_t *d_inside_dist_sq)
{
    int rc = gie_ground_check(m, "gie_read_ground_sdf_dev", true); if (rc) return rc;
    if (!d_sdf && !d_inside_dist_sq) { gie_set_err("gie_read_ground_sdf_dev: both outputs are null"); return GIE_ERR_INVALID; }
    rc = gie_gsdf_ready(m, "gie_read_ground_sdf_dev"); if (rc) return rc;
    gie_ctx c;
    op_gsdf_export op; op.g = gie_ground_view(m, &c); op.s = gie_gsdf_view(m); op.sdf = d_sdf; op.ids = d_inside_dist_sq;
    be_prof(&m->be, GIE_K_GROUND, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground_sdf(gie_mapper *m, float *sdf, int32_t *inside_dist_sq)
{
    int rc = gie_ground_check(m, "gie_read_ground_sdf", true); if (rc) return rc;
    if (!sdf && !inside_dist_sq) { gie_set_err("gie_read_ground_sdf: both outputs are null"); return GIE_ERR_INVALID; }
    const size_t n = (size_t)m->c.X * m->c.Y;
    float *ds = sdf ? (float *)gie_scratch(m, 0, n * 4, "gie_read_ground_sdf") : nullptr;
    int32_t *di = inside_dist_sq ? (int32_t *)gie_scratch(m, 1, n * 4, "gie_read_ground_sdf") : nullptr;
    if ((sdf && !ds) || (inside_dist_sq && !di)) return GIE_ERR_DEVICE;
    rc = gie_read_ground_sdf_dev(m, ds, di); if (rc) return rc;
    if (ds) be_d2h(&m->be, sdf, ds, n * 4);
    if (di) be_d2h(&m->be, inside_dist_sq, di, n * 4);
    return gie_sync(m);
}
static int gie_gsdf_query_check(gie_mapper *m, const char *who, const float *xy, int n, const void *dist, const void *grad, const void *flags)
{
    const int rc = gie_ground_check(m, who, true); if (rc) return rc;
    const char *bad = nullptr;
    if (!dist && !grad && !flags) bad = "all three outputs are null";
    else if (n < 0) bad = "n must be >= 0";
    else if (n > 0 && !xy) bad = "n > 0 with a null xy";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_ground_query_sdf_dev(gie_mapper *m, const float *d_xy, int n, float *d_dist, float *d_grad, uint8_t *d_flags)
{
    int rc = gie_gsdf_query_check(m, "gie_ground_query_sdf_dev", d_xy, n, d_dist, d_grad, d_flags); if (rc) return rc;
    if (n == 0) return GIE_OK;
    rc = gie_gsdf_ready(m, "gie_ground_query_sdf_dev"); if (rc) return rc;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    GIE_LAUNCH(&m->be, k_gsdf_query, dim3((n + 255) / 256), dim3(256), 0, c, g, gie_gsdf_view(m), d_xy, n, d_dist, d_grad, d_flags);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_ground_query_sdf(gie_mapper *m, const float *xy, int n, float *dist, float *grad, uint8_t *flags)
{
    int rc = gie_gsdf_query_check(m, "gie_ground_query_sdf", xy, n, dist, grad, flags); if (rc) return rc;
    if (n == 0) return GIE_OK;
    /* points (8 B) in the first export buffer, results (dist 4 + grad 8 + flags 1 B per point) in the second */
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_query_sdf");
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 13, "gie_ground_query_sdf");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    float *dg = (float *)dr, *dd = (float *)(dr + (size_t)n * 8);
    uint8_t *df = (uint8_t *)(dr + (size_t)n * 12);
    be_h2d(&m->be, dx, xy, (size_t)n * 8);
    rc = gie_ground_query_sdf_dev(m, dx, n, dist ? dd : nullptr, grad ? dg : nullptr, flags ? df : nullptr); if (rc) return rc;
    if (dist) be_d2h(&m->be, dist, dd, (size_t)n * 4);
    if (grad) be_d2h(&m->be, grad, dg, (size_t)n * 8);
    if (flags) be_d2h(&m->be, flags, df, (size_t)n);
    gie_scratch_trim(m);
    return gie_sync(m);
}

static int gie_gsdf_rollout_check(gie_mapper *m, const char *who, const float *xy, int n, int T, const gie_ground_sdf_rollout_param *p, const gie_ground_sdf_rollout *out)
{
    const int rc = gie_ground_check(m, who, true); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (!(std::isfinite(p->margin) && p->margin >= 0.f)) bad = "margin must be finite and >= 0";
    else if (p->flags) bad = "flags must be 0";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3] || p->reserved[4] || p->reserved[5]) bad = "reserved must be 0";
    else if (n < 0) bad = "n must be >= 0";
    else if (T < 1 || T > GIE_GROUND_ROLLOUT_MAX_POSES) bad = "T must be in 1..4096";
    else if (n > 0 && (!xy || !out)) bad = "n > 0 with a null xy or record buffer";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_ground_sdf_rollouts_dev(gie_mapper *m, const float *d_xy, int n, int T, const gie_ground_sdf_rollout_param *p, gie_ground_sdf_rollout *d_out,
                                           float *d_dist, float *d_grad)
{
    int rc = gie_gsdf_rollout_check(m, "gie_ground_sdf_rollouts_dev", d_xy, n, T, p, d_out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    rc = gie_gsdf_ready(m, "gie_ground_sdf_rollouts_dev"); if (rc) return rc;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const gie_gsdf_dev s = gie_gsdf_view(m);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    for (long long t0 = 0; t0 < n; t0 += GIE_GSDF_PER_LAUNCH) {  /* (one launch up to 2^24 trajectories) */
        const long long k = n - t0 < GIE_GSDF_PER_LAUNCH ? n - t0 : GIE_GSDF_PER_LAUNCH;
        GIE_LAUNCH(&m->be, k_gsdf_rollouts, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, c, g, s, d_xy, t0, (long long)n, T, p->margin, d_out, d_dist, d_grad);
    }
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_ground_sdf_rollouts(gie_mapper *m, const float *xy, int n, int T, const gie_ground_sdf_rollout_param *p, gie_ground_sdf_rollout *out, float *dist, float *grad)
{
    int rc = gie_gsdf_rollout_check(m, "gie_ground_sdf_rollouts", xy, n, T, p, out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    if ((size_t)n > SIZE_MAX / 16 / (size_t)T) { gie_set_err("gie_ground_sdf_rollouts: n * T * 8 bytes exceed size_t"); return GIE_ERR_INVALID; }
    /* points in the first export buffer; the gradients (8 B a point), the distances (4) and the records in the second */
    const size_t pts = (size_t)n * T, rbytes = (size_t)n * sizeof(gie_ground_sdf_rollout);
    float *dx = (float *)gie_scratch(m, 0, pts * 8, "gie_ground_sdf_rollouts");
    char *dr = (char *)gie_scratch(m, 1, (grad ? pts * 8 : 0) + (dist ? pts * 4 : 0) + rbytes, "gie_ground_sdf_rollouts");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    float *dg = (float *)dr, *dd = (float *)(dr + (grad ? pts * 8 : 0));
    gie_ground_sdf_rollout *dout = (gie_ground_sdf_rollout *)((char *)dd + (dist ? pts * 4 : 0));
    be_h2d(&m->be, dx, xy, pts * 8);
    rc = gie_ground_sdf_rollouts_dev(m, dx, n, T, p, dout, dist ? dd : nullptr, grad ? dg : nullptr); if (rc) return rc;
    be_d2h(&m->be, out, dout, rbytes);
    if (dist) be_d2h(&m->be, dist, dd, pts * 4);
    if (grad) be_d2h(&m->be, grad, dg, pts * 8);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_ground_footprint.inc.h — ground footprints: n candidate trajectories of T poses each, every pose an oriented rectangle of
 * cells tested against the ground field in one call — one record per trajectory (include/gie.h "ground footprints").
 * HIP backend only: included by gie_hip.hip after gie_ground_rollout.inc.h.  It reads the ground field's type and dist_sq planes and
 * writes nothing of the map, of that field or of the ground navigation function; it has no plane of its own: the blocked plane is
 * ground line of sight's (glos_blk, k_glos_prep), rebuilt in front of the one query launch.
 *   k_ground_footprints<MARGIN>  a wave per trajectory, four trajectories per workgroup (k_ground_rollouts' shape).  The poses
 *                      are LOADED in chunks of 64 (lane l: pose base + l, its cell by gie_ground_cell_of and its heading) and TAKEN one
 *                      at a time, in order, their seven values broadcast from the owning lane; the first pose without a placement
 *                      or with a blocked footprint cell ends both loops (wave-uniform breaks: a colliding trajectory is cheap).
 *                      Within a pose lane l takes the footprint row dy = -R + l (+ 64 per chunk of rows; R <= 362, 12 chunks at
 *                      the cap).  The predicate of the header is, for integers a and b, -isqrt(back_sq n2) <= a <= isqrt(front_sq
 *                      n2) and |b| <= isqrt(side_sq n2) with the three exact integer roots taken once per pose, by the lane that
 *                      loaded it; in a row a and b are linear in dx, so the row's interval is the intersection of [-R, R] with two exact floor/ceiling
 *                      divisions of int32 values below 2^26 — the predicate itself, solved for dx, not an estimate of it.  The
 *                      interval is clipped to the rectangle (the clipped part counts as outside cells: blocked without the flag),
 *                      and the one to several 64-bit words of blk it touches are tested with edge masks, which also keep the SET
 *                      padding bits beyond X out: popcount gives the row's blocked cells, ctz of the first non-zero word its first
 *                      blocked x.  Per pose ONE ballot of "my rows have a blocked cell"; only the pose that ends the prefix pays
 *                      a wave sum (hit_cells) and a wave minimum of the key (y, x) (hit).  MARGIN lanes whose row is clear read
 *                      dist_sq over their interval and keep the least (value << 12 | pose) of the poses that turned out clear;
 *                      one wave minimum after the loop.  With a mask (one pose, T = 1; a wave-uniform test of the pointer per
 *                      row) the lanes also write the mask bytes of their interval, 1 + the blocked bit; the mask is zeroed by a
 *                      memset in front of the two launches.
 * No LDS, no barrier, no atomics; everything that steers a loop is the same in all lanes of the wave.  Integers only (the two
 * double square roots are corrected to the exact integer root): a result does not depend on scheduling.
 * The compiler's figures and the times are in DESIGN.md 26.
 */

#define GIE_GFP_PER_LAUNCH (1ll << 24)      /* trajectories of one launch: 2^22 workgroups */
#define GIE_GFP_BIAS (1 << 20)              /* makes both halves of the (y, x) key non-negative */

/* floor(sqrt(v)) for 0 <= v < 2^48 */
GIE_DEV int gie_gfp_isqrt(const long long v)
{
    long long r = (long long)sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return (int)r;
}
/* floor(a / k), k > 0 */
GIE_DEV int gie_gfp_floordiv(const int a, const int k)
{
    const int q = a / k;
    return q - ((a - q * k) < 0 ? 1 : 0);
}
/* [x0, x1] cut to the dx with lo <= dx * k + c0 <= hi; all terms below 2^26 */
GIE_DEV void gie_gfp_clip(int k, const int c0, const int lo, const int hi, int &x0, int &x1)
{
    int L = lo - c0, H = hi - c0;                               /* L <= dx * k <= H */
    if (k == 0) { if (L > 0 || H < 0) x1 = x0 - 1; return; }
    if (k < 0) { k = -k; const int t = L; L = -H; H = -t; }
    const int a = -gie_gfp_floordiv(-L, k), b = gie_gfp_floordiv(H, k);
    x0 = a > x0 ? a : x0;
    x1 = b < x1 ? b : x1;
}

struct gie_gfp_arg { int front_sq, back_sq, side_sq, R, unknown_ok; };

template <bool MARGIN>
__global__ __launch_bounds__(256) void k_ground_footprints(const gie_ctx c, const gie_ground_dev g, const gie_glos_dev s, const gie_gfp_arg a, const float *xy,
                                                           const int32_t *heading, const long long first, const long long n, const int T,
                                                           gie_ground_footprint *out, uint8_t *mask)
{
    const long long i = first + (long long)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                                         /* wave-uniform */
    const float2 *pts = reinterpret_cast<const float2 *>(xy) + (size_t)i * T;
    const int2 *hds = reinterpret_cast<const int2 *>(heading) + (size_t)i * T;
    const bool none = gie_ground_nobs(g) == 0;
    const long long NOKEY = 0x7fffffffffffffffll;
    long long key = NOKEY;                                      /* this lane's least (dist_sq << 12 | pose) over the clear poses */
    int m = 0, end = 0, hit[2] = { 0, 0 }, hit_cells = 0;       /* the same in all lanes */
    bool stop = false;
#pragma unroll 1
    for (int base = 0; base < T && !stop; base += 64) {         /* base, j, stop steer the loops: wave-uniform */
        const int k = base + lane;
        int v[2] = { 0, 0 }, h[2] = { 0, 0 }, lim3[3] = { 0, 0, 0 };       /* lim3: isqrt(front_sq n2), isqrt(back_sq n2), isqrt(side_sq n2) of this lane's pose */
        bool has = false;
        if (k < T) {
            const float2 q = pts[k];
            const int2 d = hds[k];
            const float p[2] = { q.x, q.y };
            has = gie_ground_cell_of(c.voxel_width, s.X, s.Y, s.pvt, p, v);
            has = has && (d.x != 0 || d.y != 0) && d.x >= -32767 && d.x <= 32767 && d.y >= -32767 && d.y <= 32767;
            h[0] = has ? d.x : 0; h[1] = has ? d.y : 0;
            if (has) {                                          /* the three roots here, 64 poses at a time, not in the loop over the poses */
                const long long n2 = (long long)h[0] * h[0] + (long long)h[1] * h[1];
                lim3[0] = gie_gfp_isqrt(a.front_sq * n2); lim3[1] = gie_gfp_isqrt(a.back_sq * n2); lim3[2] = gie_gfp_isqrt(a.side_sq * n2);
            }
        }
        const uint64_t hm = __ballot(has);
        const int lim = T - base < 64 ? T - base : 64;
        int j = 0;
#pragma unroll 1
        for (; j < lim; j++) {
            if (!((hm >> j) & 1ull)) { end = 2; stop = true; break; }
            const int cx = __shfl(v[0], j), cy = __shfl(v[1], j), hx = __shfl(h[0], j), hy = __shfl(h[1], j);
            const int ah = __shfl(lim3[0], j), al = __shfl(lim3[1], j), bm = __shfl(lim3[2], j);
            int cnt = 0, lmd = 0x7fffffff;                      /* this lane's rows of this pose */
            long long hk = NOKEY;
#pragma unroll 1
            for (int rb = -a.R; rb <= a.R; rb += 64) {
                const int dy = rb + lane;
                int x0 = -a.R, x1 = a.R;
                if (dy > a.R) x1 = x0 - 1;
                gie_gfp_clip(hx, dy * hy, -al, ah, x0, x1);     /* -al <= a = dx hx + dy hy <= ah */
                gie_gfp_clip(hy, -dy * hx, -bm, bm, x0, x1);    /* -bm <= b = dx hy - dy hx <= bm */
                if (x0 > x1) continue;
                const int y = cy + dy, gx0 = cx + x0, gx1 = cx + x1;
                const int ix0 = gx0 > 0 ? gx0 : 0, ix1 = gx1 < s.X - 1 ? gx1 : s.X - 1;
                const int inside = (y >= 0 && y < s.Y && ix0 <= ix1) ? ix1 - ix0 + 1 : 0, outside = (x1 - x0 + 1) - inside;
                int rc = 0, fx = 0x7fffffff;                    /* the row's blocked cells and the first of them */
                if (!a.unknown_ok && outside > 0) { rc = outside; if (inside == 0 || gx0 < 0) fx = gx0; }
                if (inside > 0) {
                    const uint64_t *row = s.blk + (size_t)y * s.W;
                    const int w0 = ix0 >> 6, w1 = ix1 >> 6;
                    for (int w = w0; w <= w1; w++) {
                        uint64_t b = row[w];
                        if (w == w0) b &= ~0ull << (ix0 & 63);
                        if (w == w1) b &= ~0ull >> (63 - (ix1 & 63));               /* (ix1 < X: no padding bit passes) */
                        if (b) {
                            if (fx == 0x7fffffff) fx = w * 64 + (int)__builtin_ctzll(b);
                            rc += (int)__popcll(b);
                        }
                    }
                    if (mask)
                        for (int x = ix0; x <= ix1; x++) mask[(size_t)y * s.X + x] = gie_glos_blocked(s, x, y) ? 2 : 1;
                    if (MARGIN && !none && rc == 0) {
                        const int32_t *dr = s.dist + (size_t)y * s.X;
                        for (int x = ix0; x <= ix1; x++) { const int d = dr[x]; lmd = d < lmd ? d : lmd; }
                    }
                    if (!a.unknown_ok && fx == 0x7fffffff && gx1 >= s.X) fx = s.X;
                }
                if (rc > 0) {
                    if (hk == NOKEY) hk = ((long long)(y + GIE_GFP_BIAS) << 32) | (long long)(fx + GIE_GFP_BIAS);      /* (rows ascend within a lane) */
                    cnt += rc;
                }
            }
            if (__ballot(cnt > 0)) {                            /* pose base + j ends the prefix */
                hit_cells = gie_grol_sum32(cnt);
                hk = gie_grol_min64(hk);
                hit[0] = (int)(hk & 0xffffffffll) - GIE_GFP_BIAS + s.pvt[0];
                hit[1] = (int)(hk >> 32) - GIE_GFP_BIAS + s.pvt[1];
                end = 1; stop = true;
                break;
            }
            if (MARGIN && lmd != 0x7fffffff) { const long long q = ((long long)lmd << 12) | (base + j); key = q < key ? q : key; }
        }
        m = base + j;
    }
    if (MARGIN) key = gie_grol_min64(key);
    if (lane == 0 && out) {
        gie_ground_footprint r;
        r.end = end; r.poses = m; r.hit[0] = hit[0]; r.hit[1] = hit[1]; r.hit_cells = hit_cells;
        if (MARGIN) {
            r.min_dist_sq = m == 0 ? 0 : (none ? -1 : (int)(key >> 12));
            r.min_at = m == 0 ? -1 : (none ? 0 : (int)(key & 4095));
        } else r.min_dist_sq = r.min_at = -2;
        r.reserved = 0;
        out[i] = r;
    }
}

/* ---- host side */
static int gie_gfp_check(gie_mapper *m, const char *who, const float *xy, const int32_t *heading, int n, int T, const gie_ground_footprint_param *p,
                         const gie_ground_footprint *out, bool mask_form, const void *mask)
{
    static_assert(sizeof(gie_ground_footprint_param) == 32 && sizeof(gie_ground_footprint) == 32, "the sizes include/gie.h states");
    static_assert(GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE == GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE && GIE_GROUND_ROLLOUT_MAX_POSES == 4096 &&
                  GIE_GROUND_FOOTPRINT_MAX_SQ == (1 << 16), "k_glos_prep's flag; 12 bits of the pose in the margin key; products below 2^48");
    const int rc = gie_glos_check(m, who); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->front_sq < 0 || p->front_sq > GIE_GROUND_FOOTPRINT_MAX_SQ || p->back_sq < 0 || p->back_sq > GIE_GROUND_FOOTPRINT_MAX_SQ ||
             p->side_sq < 0 || p->side_sq > GIE_GROUND_FOOTPRINT_MAX_SQ) bad = "front_sq, back_sq and side_sq must be in 0 .. 1 << 16";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->flags & ~(GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE | GIE_GROUND_FOOTPRINT_MARGIN)) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2]) bad = "reserved must be 0";
    else if (n < 0) bad = "n must be >= 0";
    else if (T < 1 || T > GIE_GROUND_ROLLOUT_MAX_POSES) bad = "T must be in 1..4096";
    else if (n > 0 && (!xy || !heading || (!mask_form && !out))) bad = "n > 0 with a null buffer";
    else if (mask_form && !mask) bad = "null mask";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* the two launches (more footprint launches only beyond 2^24 trajectories); with d_mask its zeroing in front of them */
static int gie_gfp_run(gie_mapper *m, const char *who, const float *d_xy, const int32_t *d_heading, int n, int T, const gie_ground_footprint_param *p,
                       gie_ground_footprint *d_out, uint8_t *d_mask)
{
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    gie_glos_dev s;
    gie_gfp_arg a;
    a.front_sq = (int)p->front_sq; a.back_sq = (int)p->back_sq; a.side_sq = (int)p->side_sq;
    a.unknown_ok = (p->flags & GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE) != 0;
    const int q = std::max(a.front_sq, a.back_sq) + a.side_sq;
    int R = (int)std::sqrt((double)q);
    while (R * R > q) R--;
    while ((R + 1) * (R + 1) <= q) R++;
    a.R = R;                                                    /* <= 362 */
    const bool margin = (p->flags & GIE_GROUND_FOOTPRINT_MARGIN) != 0;
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    if (d_mask) be_memset(&m->be, d_mask, 0, (size_t)c.X * c.Y);
    const bool ok = gie_glos_prepare(m, who, c, g, (int)p->clearance_sq, (int)p->flags & GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE, &s);
    for (long long t0 = 0; ok && t0 < n; t0 += GIE_GFP_PER_LAUNCH) {       /* (one launch up to 2^24 trajectories) */
        const long long k = n - t0 < GIE_GFP_PER_LAUNCH ? n - t0 : GIE_GFP_PER_LAUNCH;
        const dim3 grid((unsigned)((k + 3) / 4));
        if (margin) GIE_LAUNCH(&m->be, k_ground_footprints<true>, grid, dim3(256), 0, c, g, s, a, d_xy, d_heading, t0, (long long)n, T, d_out, d_mask);
        else GIE_LAUNCH(&m->be, k_ground_footprints<false>, grid, dim3(256), 0, c, g, s, a, d_xy, d_heading, t0, (long long)n, T, d_out, d_mask);
    }
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return ok ? GIE_OK : GIE_ERR_DEVICE;
}

extern "C" int gie_ground_footprints_dev(gie_mapper *m, const float *d_xy, const int32_t *d_heading, int n, int T, const gie_ground_footprint_param *p,
                                         gie_ground_footprint *d_out)
{
    const int rc = gie_gfp_check(m, "gie_ground_footprints_dev", d_xy, d_heading, n, T, p, d_out, false, nullptr); if (rc) return rc;
    if (n == 0) return GIE_OK;
    return gie_gfp_run(m, "gie_ground_footprints_dev", d_xy, d_heading, n, T, p, d_out, nullptr);
}
extern "C" int gie_ground_footprints(gie_mapper *m, const float *xy, const int32_t *heading, int n, int T, const gie_ground_footprint_param *p,
                                     gie_ground_footprint *out)
{
    int rc = gie_gfp_check(m, "gie_ground_footprints", xy, heading, n, T, p, out, false, nullptr); if (rc) return rc;
    if (n == 0) return GIE_OK;
    if ((size_t)n > SIZE_MAX / 16 / (size_t)T) { gie_set_err("gie_ground_footprints: n * T * 16 bytes exceed size_t"); return GIE_ERR_INVALID; }
    const size_t xbytes = (size_t)n * T * 8, rbytes = (size_t)n * sizeof(gie_ground_footprint);
    char *di = (char *)gie_scratch(m, 0, 2 * xbytes, "gie_ground_footprints");                   /* the poses, then the headings */
    gie_ground_footprint *dr = (gie_ground_footprint *)gie_scratch(m, 1, rbytes, "gie_ground_footprints");
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, xy, xbytes);
    be_h2d(&m->be, di + xbytes, heading, xbytes);
    rc = gie_gfp_run(m, "gie_ground_footprints", (const float *)di, (const int32_t *)(di + xbytes), n, T, p, dr, nullptr); if (rc) return rc;
    be_d2h(&m->be, out, dr, rbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_ground_footprint_mask_dev(gie_mapper *m, const float *d_xy, const int32_t *d_heading, const gie_ground_footprint_param *p, uint8_t *d_mask,
                                             gie_ground_footprint *d_rec)
{
    const int rc = gie_gfp_check(m, "gie_ground_footprint_mask_dev", d_xy, d_heading, 1, 1, p, d_rec, true, d_mask); if (rc) return rc;
    return gie_gfp_run(m, "gie_ground_footprint_mask_dev", d_xy, d_heading, 1, 1, p, d_rec, d_mask);
}
extern "C" int gie_ground_footprint_mask(gie_mapper *m, const float *xy, const int32_t *heading, const gie_ground_footprint_param *p, uint8_t *mask,
                                         gie_ground_footprint *rec)
{
    int rc = gie_gfp_check(m, "gie_ground_footprint_mask", xy, heading, 1, 1, p, rec, true, mask); if (rc) return rc;
    const size_t cells = (size_t)m->c.X * m->c.Y;
    char *di = (char *)gie_scratch(m, 0, 16, "gie_ground_footprint_mask");                        /* the pose, then the heading */
    char *dr = (char *)gie_scratch(m, 1, sizeof(gie_ground_footprint) + cells, "gie_ground_footprint_mask");   /* the record, then the mask */
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, xy, 8);
    be_h2d(&m->be, di + 8, heading, 8);
    rc = gie_gfp_run(m, "gie_ground_footprint_mask", (const float *)di, (const int32_t *)(di + 8), 1, 1, p, (gie_ground_footprint *)dr,
                     (uint8_t *)dr + sizeof(gie_ground_footprint));
    if (rc) return rc;
    if (rec) be_d2h(&m->be, rec, dr, sizeof(gie_ground_footprint));
    be_d2h(&m->be, mask, dr + sizeof(gie_ground_footprint), cells);
    gie_scratch_trim(m);
    return gie_sync(m);
}

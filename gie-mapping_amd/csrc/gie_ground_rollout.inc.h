/*
 * gie_ground_rollout.inc.h — ground rollouts: n candidate trajectories of T poses each, scored on the ground field in one call — one
 * record per trajectory (include/gie.h "ground rollouts").
 * HIP backend only: included by gie_hip.hip after gie_ground_view.inc.h.  It reads the ground field's type and dist_sq planes and the
 * ground navigation function's field and writes nothing of the map, of that field or of that function; it has no plane of its own:
 * the blocked plane is ground line of sight's (glos_blk, k_glos_prep), rebuilt in front of the one query launch.
 *   k_ground_rollouts<NF1>  a wave per trajectory, four trajectories per workgroup (k_ground_shortcut's shape).  The poses go in chunks
 *                      of 64, in order; in chunk `base` lane l owns pose k = base + l: one float2 load, gie_ground_cell_of, the cell of
 *                      pose k - 1 from the lane below (a wave shuffle; lane 0 takes the previous chunk's last cell from two scalar
 *                      registers), then the walk of L2(c_{k-1}, c_k) from the cell AFTER c_{k-1} (pose 0: c_0 alone): a bit test and
 *                      a dist_sq load per cell, leaving at its first blocked cell.  f = ctz(ballot(no pose || no cell || blocked)) is
 *                      the first lane that ends the prefix; the lanes below f add their chunk's cells, minimum, cost and NF1 key to
 *                      their running values, and a chunk with f < 64 is the last.  ONE set of wave reductions after the loop:
 *                      an int32 sum, an int32 minimum, an int64 sum and, for NF1, the minimum of the 64-bit key (value << 12) | k
 *                      — the first pose with the least value wins.  Everything that steers the loop (base, f) is the same in all
 *                      lanes; there is no LDS and no barrier.
 * The bit plane (128 KiB at most) and the dist_sq plane are read where they lie, as in gie_ground_los.inc.h: no LDS staging
 * ("not built").  Integers only: a result does not depend on scheduling.
 * The compiler's figures and the times are in DESIGN.md 25.
 */

#define GIE_GROL_PER_LAUNCH (1ll << 24)     /* trajectories of one launch: 2^22 workgroups */

GIE_DEV int gie_grol_sum32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
GIE_DEV int gie_grol_min32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
GIE_DEV long long gie_grol_sum64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
GIE_DEV long long gie_grol_min64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}

template <bool NF1>
__global__ __launch_bounds__(256) void k_ground_rollouts(const gie_ctx c, const gie_ground_dev g, const gie_glos_dev s, const int32_t *nf, const float *xy,
                                                         const long long first, const long long n, const int T, const int inflate_sq, gie_ground_rollout *out)
{
    const long long i = first + (long long)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                                         /* wave-uniform */
    const float2 *pts = reinterpret_cast<const float2 *>(xy) + (size_t)i * T;
    const bool none = gie_ground_nobs(g) == 0;
    const long long NOKEY = 0x7fffffffffffffffll;
    int cells = 0, md = 0x7fffffff;                             /* this lane's running values: its poses of every chunk below the end */
    long long cost = 0, key = NOKEY;
    int m = 0, end = 0, hit[2] = { 0, 0 }, nf_end = -1;         /* the same in all lanes */
    int pc[2] = { 0, 0 };                                       /* the previous chunk's last cell */
#pragma unroll 1
    for (int base = 0; base < T; base += 64) {                  /* base and f steer the loop: wave-uniform */
        const int k = base + lane;
        int v[2] = { 0, 0 };
        bool has = false;
        if (k < T) {
            const float2 q = pts[k];
            const float p[2] = { q.x, q.y };
            has = gie_ground_cell_of(c.voxel_width, s.X, s.Y, s.pvt, p, v);
        }
        int a[2] = { __shfl_up(v[0], 1), __shfl_up(v[1], 1) };
        const uint64_t hm = __ballot(has);
        const bool below = lane == 0 ? true : (hm >> (lane - 1)) & 1ull;      /* pose k - 1 has a cell (lane 0: a chunk is entered only then) */
        if (lane == 0) { a[0] = pc[0]; a[1] = pc[1]; }
        bool blk = false;
        int lc = 0, lmd = 0x7fffffff, h[2] = { 0, 0 }, val = -1;
        long long lcost = 0;
        if (has && below) {                                     /* (a lane behind a pose without a cell is behind the end: no walk) */
            gie_gwalk w;
            int u[2] = { a[0], a[1] };
            bool more = true;
            if (k == 0) { u[0] = v[0]; u[1] = v[1]; w.T[0] = w.T[1] = GIE_GLOS_T_DONE; }       /* c_0 alone */
            else { gie_gwalk_init(w, a, v); more = gie_gwalk_step(w, u); }                      /* from the cell after c_{k-1} */
            while (more) {
                if (gie_glos_blocked(s, u[0], u[1])) { blk = true; h[0] = u[0]; h[1] = u[1]; break; }
                const int d = gie_glos_dist(s, none, u[0], u[1]);
                lmd = d < lmd ? d : lmd;
                lcost += (none || d >= inflate_sq) ? 0 : inflate_sq - d;
                lc++;
                more = gie_gwalk_step(w, u);
            }
            if (NF1 && !blk) val = nf[(size_t)v[1] * s.X + v[0]];
        }
        const uint64_t bad = __ballot(k >= T || !has || blk);
        const int f = bad ? (int)__builtin_ctzll(bad) : 64;
        if (lane < f) {
            cells += lc; md = lmd < md ? lmd : md; cost += lcost;
            if (NF1 && val >= 0) { const long long q = ((long long)val << 12) | k; key = q < key ? q : key; }
        }
        m = base + f;
        if (NF1 && f > 0) nf_end = __shfl(val, f - 1);
        if (f < 64) {
            if (m < T) {                                        /* lane f ended it: without a cell, or at a blocked cell */
                const int fh = __shfl((int)has, f);
                end = fh ? 1 : 2;
                hit[0] = fh ? __shfl(h[0], f) + s.pvt[0] : 0;
                hit[1] = fh ? __shfl(h[1], f) + s.pvt[1] : 0;
            }
            break;
        }
        pc[0] = __builtin_amdgcn_readlane(v[0], 63); pc[1] = __builtin_amdgcn_readlane(v[1], 63);
    }
    cells = gie_grol_sum32(cells);
    md = gie_grol_min32(md);
    cost = gie_grol_sum64(cost);
    if (NF1) key = gie_grol_min64(key);
    if (lane == 0) {
        gie_ground_rollout r;
        r.end = end; r.poses = m; r.hit[0] = hit[0]; r.hit[1] = hit[1];
        r.cells = cells; r.min_dist_sq = m > 0 ? md : 0; r.cost = cost;
        if (NF1) {
            r.nf1_end = nf_end;
            r.nf1_min = key == NOKEY ? -1 : (int)(key >> 12);
            r.nf1_min_at = key == NOKEY ? -1 : (int)(key & 4095);
        } else r.nf1_end = r.nf1_min = r.nf1_min_at = -2;
        r.reserved = 0;
        out[i] = r;
    }
}

/* ---- host side */
static int gie_grol_check(gie_mapper *m, const char *who, const float *xy, int n, int T, const gie_ground_rollout_param *p, const gie_ground_rollout *out)
{
    static_assert(sizeof(gie_ground_rollout_param) == 32 && sizeof(gie_ground_rollout) == 48 && offsetof(gie_ground_rollout, cost) == 24,
                  "the sizes include/gie.h states");
    static_assert(GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE == GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE && GIE_GROUND_ROLLOUT_MAX_POSES == 4096, "k_glos_prep's flag; 12 bits of k in the NF1 key");
    const int rc = gie_glos_check(m, who); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->inflate_sq < 0 || p->inflate_sq > (1 << 22)) bad = "inflate_sq must be in 0 .. 1 << 22";
    else if (p->flags & ~(GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE | GIE_GROUND_ROLLOUT_NF1)) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3] || p->reserved[4]) bad = "reserved must be 0";
    else if ((p->flags & GIE_GROUND_ROLLOUT_NF1) && !m->gnf1.valid) bad = "GIE_GROUND_ROLLOUT_NF1 without a ground navigation function of this ground field (gie_ground_nf1_compute first)";
    else if (n < 0) bad = "n must be >= 0";
    else if (T < 1 || T > GIE_GROUND_ROLLOUT_MAX_POSES) bad = "T must be in 1..4096";
    else if (n > 0 && (!xy || !out)) bad = "n > 0 with a null buffer";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_ground_rollouts_dev(gie_mapper *m, const float *d_xy, int n, int T, const gie_ground_rollout_param *p, gie_ground_rollout *d_out)
{
    const int rc = gie_grol_check(m, "gie_ground_rollouts_dev", d_xy, n, T, p, d_out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    gie_glos_dev s;
    const bool nf1 = (p->flags & GIE_GROUND_ROLLOUT_NF1) != 0;
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    const bool ok = gie_glos_prepare(m, "gie_ground_rollouts_dev", c, g, (int)p->clearance_sq, (int)p->flags & GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE, &s);
    for (long long t0 = 0; ok && t0 < n; t0 += GIE_GROL_PER_LAUNCH) {      /* (one launch up to 2^24 trajectories) */
        const long long k = n - t0 < GIE_GROL_PER_LAUNCH ? n - t0 : GIE_GROL_PER_LAUNCH;
        const dim3 grid((unsigned)((k + 3) / 4));
        if (nf1) GIE_LAUNCH(&m->be, k_ground_rollouts<true>, grid, dim3(256), 0, c, g, s, m->gnf1.f, d_xy, t0, (long long)n, T, (int)p->inflate_sq, d_out);
        else GIE_LAUNCH(&m->be, k_ground_rollouts<false>, grid, dim3(256), 0, c, g, s, (const int32_t *)nullptr, d_xy, t0, (long long)n, T, (int)p->inflate_sq, d_out);
    }
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return ok ? GIE_OK : GIE_ERR_DEVICE;
}
extern "C" int gie_ground_rollouts(gie_mapper *m, const float *xy, int n, int T, const gie_ground_rollout_param *p, gie_ground_rollout *out)
{
    int rc = gie_grol_check(m, "gie_ground_rollouts", xy, n, T, p, out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    if ((size_t)n > SIZE_MAX / 8 / (size_t)T) { gie_set_err("gie_ground_rollouts: n * T * 8 bytes exceed size_t"); return GIE_ERR_INVALID; }
    const size_t xbytes = (size_t)n * T * 8, rbytes = (size_t)n * sizeof(gie_ground_rollout);
    float *dx = (float *)gie_scratch(m, 0, xbytes, "gie_ground_rollouts");
    gie_ground_rollout *dr = (gie_ground_rollout *)gie_scratch(m, 1, rbytes, "gie_ground_rollouts");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xy, xbytes);
    rc = gie_ground_rollouts_dev(m, dx, n, T, p, dr); if (rc) return rc;
    be_d2h(&m->be, out, dr, rbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_ground_los.inc.h — ground line of sight: batched segment checks over exact 2-D cell lines on the ground field, and any-angle
 * waypoints from a polyline of cells (include/gie.h "ground line of sight").
 * HIP backend only: included by gie_hip.hip after gie_ground_nf1.inc.h.  It reads the ground field's type and dist_sq planes and
 * writes nothing of the map, of that field or of the ground navigation function; its one plane is allocated at the first call.
 *   k_glos_prep        one lane per cell, a wave per 64-cell word (k_gnf1_prep's ballot form): the bit row blk = ~traversable (rows of
 *                      W = ceil(X/64) words, bit x & 63 of word x >> 6; the padding bits beyond X are SET).  One launch in front of
 *                      every query launch: no result is kept, a call sees the field as it stands where it is enqueued.  Ground
 *                      NF1's blk plane is not this one: after the propagation it means "blocked or visited".
 *   k_ground_segments  a lane per segment (k_los_segments' form): the walk of L2(a, b), a bit test and a dist_sq load per step up
 *                      to the first blocked cell; after it only the length is counted.
 *   k_ground_shortcut  a wave per path, four paths per workgroup (k_path_shortcut's window form).  With top = min(k + K, m - 1),
 *                      chunk c gives lane l the candidate j = top - 64 c - l; the lane walks L2(v_k, v_j) and leaves at its first
 *                      blocked cell; the first chunk with a clear lane decides, k' = top - 64 c - ctz(ballot).  A v_k outside the
 *                      field or blocked forces the leg without a walk.  The chosen leg's min_dist_sq is a SECOND walk of that one
 *                      line by the wave's first lane, with loads of the dist_sq plane.  Everything that steers a loop is the same
 *                      in all lanes of the wave.
 * The walk (gie_gwalk): crossing j of axis k lies at t = (2j - 1) / (2 n_k); with two axes T_x = (2 j_x - 1) * n_y and
 * T_y = (2 j_y - 1) * n_x order the crossings exactly, below 2^22 for sides <= 1024: two 32-bit terms, a step is the smaller of them
 * and both axes move on a tie.  The bit plane of the largest field is 128 KiB and stays in L2: it is read where it lies, not staged
 * in LDS.  Integers and one float sum in leg order: a result does not depend on scheduling.
 */

#define GIE_GLOS_T_DONE 0x7fffffff

struct gie_glos_dev {
    uint64_t *blk;          /* W words per row y: blocked */
    const int32_t *dist;    /* the ground field's dist_sq plane (holds nothing when `none`) */
    int W, X, Y;
    int pvt[2];
};

__global__ __launch_bounds__(256) void k_glos_prep(const gie_ctx c, const gie_ground_dev g, uint64_t *blk, const int nwords, const int clearance_sq,
                                                   const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const bool none = gie_ground_nobs(g) == 0;                  /* no obstacle column: dist_sq is -1 everywhere */
    const int y = wd / g.W, x = (wd - y * g.W) * 64 + lane;
    bool tr = false;
    if (x < c.X) tr = gie_ground_traversable(g, y * c.X + x, none, clearance_sq, flags & GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE);
    const uint64_t bt = __ballot(tr);
    if (lane == 0) blk[wd] = ~bt;
}

GIE_DEV bool gie_glos_blocked(const gie_glos_dev &s, const int x, const int y)
{
    return (s.blk[(size_t)y * s.W + (x >> 6)] >> (x & 63)) & 1ull;
}
GIE_DEV int gie_glos_dist(const gie_glos_dev &s, const bool none, const int x, const int y)
{
    return none ? -1 : s.dist[(size_t)y * s.X + x];
}

/* the walk of L2(a, b): T_k the next crossing of axis k (GIE_GLOS_T_DONE: none left), D_k the distance between two of them */
struct gie_gwalk { int T[2], D[2], left[2], s[2]; };
GIE_DEV void gie_gwalk_init(gie_gwalk &w, const int a[2], const int b[2])
{
    int n[2];
#pragma unroll
    for (int k = 0; k < 2; k++) { const int d = b[k] - a[k]; n[k] = d < 0 ? -d : d; w.s[k] = d < 0 ? -1 : 1; w.left[k] = n[k]; }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int M = n[1 - k] ? n[1 - k] : 1;
        w.D[k] = 2 * M; w.T[k] = n[k] ? M : GIE_GLOS_T_DONE;
    }
}
/* the next cell of the line into v; false when v is the last one */
GIE_DEV bool gie_gwalk_step(gie_gwalk &w, int v[2])
{
    const int t = w.T[0] < w.T[1] ? w.T[0] : w.T[1];
    if (t == GIE_GLOS_T_DONE) return false;
#pragma unroll
    for (int k = 0; k < 2; k++)
        if (w.T[k] == t) { v[k] += w.s[k]; w.left[k] -= 1; w.T[k] = w.left[k] ? w.T[k] + w.D[k] : GIE_GLOS_T_DONE; }
    return true;
}

/* the local cell of a path point (any int32: the difference in 64 bits); false outside the rectangle */
GIE_DEV bool gie_glos_local(const gie_glos_dev &s, const int32_t *g, int v[2])
{
    const long long x = (long long)g[0] - s.pvt[0], y = (long long)g[1] - s.pvt[1];
    const bool in = x >= 0 && x < s.X && y >= 0 && y < s.Y;
    v[0] = in ? (int)x : 0; v[1] = in ? (int)y : 0;
    return in;
}

__global__ __launch_bounds__(256) void k_ground_segments(const gie_ctx c, const gie_ground_dev g, const gie_glos_dev s, const float *a_xy, const float *b_xy,
                                                         const int n, gie_ground_hit *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int a[2], b[2];
    gie_ground_hit h;
    h.reserved = 0;
    const bool ina = gie_ground_cell_of(c.voxel_width, s.X, s.Y, s.pvt, a_xy + 2 * (size_t)i, a), inb = gie_ground_cell_of(c.voxel_width, s.X, s.Y, s.pvt, b_xy + 2 * (size_t)i, b);
    if (!ina || !inb) {
        h.first = -2; h.len = 0; h.hit[0] = h.hit[1] = 0; h.min_dist_sq = 0;
        out[i] = h;
        return;
    }
    const bool none = gie_ground_nobs(g) == 0;
    gie_gwalk w;
    gie_gwalk_init(w, a, b);
    int v[2] = { a[0], a[1] }, idx = 0, first = -1;
    int md = gie_glos_dist(s, none, a[0], a[1]);
    h.hit[0] = b[0]; h.hit[1] = b[1];
    for (;;) {
        if (first < 0) {                                        /* (after the hit only the length is still wanted: no loads) */
            const int d = gie_glos_dist(s, none, v[0], v[1]);
            md = d < md ? d : md;
            if (gie_glos_blocked(s, v[0], v[1])) { first = idx; h.hit[0] = v[0]; h.hit[1] = v[1]; }
        }
        if (!gie_gwalk_step(w, v)) break;
        idx++;
    }
    h.first = first; h.len = idx + 1; h.min_dist_sq = md;
    h.hit[0] += s.pvt[0]; h.hit[1] += s.pvt[1];
    out[i] = h;
}

__global__ __launch_bounds__(256) void k_ground_shortcut(const gie_ground_dev g, const gie_glos_dev s, const int32_t *path, const int32_t *len, const int n,
                                                         const int max_len, const int K, const int max_wp, gie_ground_waypoint *wp, gie_shortcut_info *info)
{
    const int p = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n) return;                                         /* wave-uniform */
    const int32_t *pts = path + (size_t)p * max_len * 2;
    gie_ground_waypoint *out = wp + (size_t)p * max_wp;         /* (not touched when max_wp == 0) */
    int m = len[p];
    m = m < 0 ? 0 : (m > max_len ? max_len : m);
    int count = 0, forced = 0;
    float length = 0.f;
    if (m > 0) {
        const bool none = gie_ground_nobs(g) == 0;
        int a[2], k = 0;
        bool ina = gie_glos_local(s, pts, a);
        if (lane == 0 && max_wp > 0) {
            gie_ground_waypoint r;
            r.xy[0] = pts[0]; r.xy[1] = pts[1]; r.index = 0; r.forced = 0; r.reserved = 0;
            r.min_dist_sq = ina ? gie_glos_dist(s, none, a[0], a[1]) : -2;
            out[0] = r;
        }
        count = 1;
        /* everything that steers the loops below is the same in all lanes of the wave: k, a, the ballots */
#pragma unroll 1
        while (k < m - 1) {
            int nk = -1;
            if (ina && !gie_glos_blocked(s, a[0], a[1])) {
                const int top = m - 1 - k > K ? k + K : m - 1;
#pragma unroll 1
                for (int base = top; base > k; base -= 64) {
                    const int j = base - lane;
                    bool clear = false;
                    int b[2];
                    if (j > k && gie_glos_local(s, pts + 2 * (size_t)j, b)) {
                        gie_gwalk w;
                        gie_gwalk_init(w, a, b);
                        int v[2] = { a[0], a[1] };
                        clear = true;
                        while (gie_gwalk_step(w, v))
                            if (gie_glos_blocked(s, v[0], v[1])) { clear = false; break; }
                    }
                    const uint64_t bal = __ballot(clear);
                    if (bal) { nk = base - (int)__builtin_ctzll(bal); break; }
                }
            }
            const bool f = nk < 0;
            if (f) nk = k + 1;
            int b[2];
            const bool inb = gie_glos_local(s, pts + 2 * (size_t)nk, b);
            if (lane == 0) {
                gie_ground_waypoint r;
                r.xy[0] = pts[2 * (size_t)nk]; r.xy[1] = pts[2 * (size_t)nk + 1];
                r.index = nk; r.forced = f ? 1 : 0; r.min_dist_sq = -2; r.reserved = 0;
                if (f) forced++;
                else {
                    const int dx = b[0] - a[0], dy = b[1] - a[1];
                    length += sqrtf((float)(dx * dx + dy * dy));
                    if (count < max_wp) {                       /* (a record that is not written needs no minimum) */
                        gie_gwalk w;
                        gie_gwalk_init(w, a, b);
                        int v[2] = { a[0], a[1] };
                        int md = gie_glos_dist(s, none, v[0], v[1]);
                        while (gie_gwalk_step(w, v)) { const int d = gie_glos_dist(s, none, v[0], v[1]); md = d < md ? d : md; }
                        r.min_dist_sq = md;
                    }
                }
                if (count < max_wp) out[count] = r;
            }
            count++;
            k = nk; ina = inb; a[0] = b[0]; a[1] = b[1];
        }
    }
    if (lane == 0 && info) { gie_shortcut_info q; q.count = count; q.forced = forced; q.length = length; q.reserved = 0; info[p] = q; }
}

/* ---- host side */
static int gie_glos_check(gie_mapper *m, const char *who)
{
    static_assert(sizeof(gie_ground_los_param) == 16 && sizeof(gie_ground_hit) == 24 && sizeof(gie_ground_shortcut_param) == 32 &&
                  sizeof(gie_ground_waypoint) == 24, "the sizes include/gie.h states");
    return gie_ground_check(m, who, true, "lines");
}
static const char *gie_glos_bad_rule(int clearance_sq, int flags, const int32_t *reserved, int n_reserved)
{
    if (clearance_sq < 0) return "clearance_sq must be >= 0";
    if (flags & ~GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE) return "unknown flags";
    for (int i = 0; i < n_reserved; i++) if (reserved[i]) return "reserved must be 0";
    return nullptr;
}
static int gie_ground_segments_args(const char *who, const float *a_xy, const float *b_xy, int n, const gie_ground_los_param *p, const gie_ground_hit *out)
{
    const char *bad = p ? gie_glos_bad_rule(p->clearance_sq, p->flags, p->reserved, 2) : "null parameters";
    if (bad) { }
    else if (n < 0) bad = "n must be >= 0";
    else if (n > 0 && (!a_xy || !b_xy || !out)) bad = "n > 0 with a null buffer";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_ground_shortcut_args(const char *who, const int32_t *path_xy, const int32_t *len, int n, int max_len, const gie_ground_shortcut_param *p,
                                    const gie_ground_waypoint *wp, const gie_shortcut_info *info)
{
    const char *bad = p ? gie_glos_bad_rule(p->clearance_sq, p->flags, p->reserved, 4) : "null parameters";
    if (bad) { }
    else if (p->lookahead < 1 || p->lookahead > 4096) bad = "lookahead must be in 1..4096";
    else if (p->max_wp < 0) bad = "max_wp must be >= 0";
    else if (n < 0) bad = "n must be >= 0";
    else if (max_len < 1) bad = "max_len must be >= 1";
    else if (n > 0 && (!path_xy || !len)) bad = "n > 0 with a null path buffer";
    else if (!wp && p->max_wp > 0) bad = "null waypoint buffer with max_wp > 0";
    else if (!wp && !info) bad = "nothing to write: both outputs null";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* the blocked plane of the field as it stands, enqueued in front of a query launch; false when its allocation failed */
static bool gie_glos_prepare(gie_mapper *m, const char *who, const gie_ctx &c, const gie_ground_dev &g, int clearance_sq, int flags, gie_glos_dev *s)
{
    const int nwords = g.W * c.Y;
    if (!m->glos_blk) {
        m->glos_blk = gie_dalloc<uint64_t>(m, (size_t)nwords, false);
        if (!m->glos_blk) { gie_set_err(std::string(who) + ": device allocation of the blocked plane failed"); return false; }
    }
    s->blk = m->glos_blk; s->dist = g.dist; s->W = g.W; s->X = c.X; s->Y = c.Y; s->pvt[0] = g.pvt[0]; s->pvt[1] = g.pvt[1];
    GIE_LAUNCH(&m->be, k_glos_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, g, s->blk, nwords, clearance_sq, flags);
    return true;
}

extern "C" int gie_ground_segments_dev(gie_mapper *m, const float *d_a_xy, const float *d_b_xy, int n, const gie_ground_los_param *p, gie_ground_hit *d_out)
{
    int rc = gie_glos_check(m, "gie_ground_segments_dev"); if (rc) return rc;
    rc = gie_ground_segments_args("gie_ground_segments_dev", d_a_xy, d_b_xy, n, p, d_out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    gie_glos_dev s;
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    const bool ok = gie_glos_prepare(m, "gie_ground_segments_dev", c, g, (int)p->clearance_sq, (int)p->flags, &s);
    if (ok) GIE_LAUNCH(&m->be, k_ground_segments, dim3((n + 255) / 256), dim3(256), 0, c, g, s, d_a_xy, d_b_xy, n, d_out);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return ok ? GIE_OK : GIE_ERR_DEVICE;
}
extern "C" int gie_ground_segments(gie_mapper *m, const float *a_xy, const float *b_xy, int n, const gie_ground_los_param *p, gie_ground_hit *out)
{
    int rc = gie_glos_check(m, "gie_ground_segments"); if (rc) return rc;
    rc = gie_ground_segments_args("gie_ground_segments", a_xy, b_xy, n, p, out); if (rc) return rc;
    if (n == 0) return GIE_OK;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 16, "gie_ground_segments");           /* a, then b */
    gie_ground_hit *dr = (gie_ground_hit *)gie_scratch(m, 1, (size_t)n * sizeof(gie_ground_hit), "gie_ground_segments");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, a_xy, (size_t)n * 8);
    be_h2d(&m->be, dx + 2 * (size_t)n, b_xy, (size_t)n * 8);
    rc = gie_ground_segments_dev(m, dx, dx + 2 * (size_t)n, n, p, dr); if (rc) return rc;
    be_d2h(&m->be, out, dr, (size_t)n * sizeof(gie_ground_hit));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_ground_shortcut_dev(gie_mapper *m, const int32_t *d_path_xy, const int32_t *d_len, int n, int max_len, const gie_ground_shortcut_param *p,
                                       gie_ground_waypoint *d_wp, gie_shortcut_info *d_info)
{
    int rc = gie_glos_check(m, "gie_ground_shortcut_dev"); if (rc) return rc;
    rc = gie_ground_shortcut_args("gie_ground_shortcut_dev", d_path_xy, d_len, n, max_len, p, d_wp, d_info); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    gie_glos_dev s;
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    const bool ok = gie_glos_prepare(m, "gie_ground_shortcut_dev", c, g, (int)p->clearance_sq, (int)p->flags, &s);
    if (ok) GIE_LAUNCH(&m->be, k_ground_shortcut, dim3((n + 3) / 4), dim3(256), 0, g, s, d_path_xy, d_len, n, max_len, (int)p->lookahead, (int)p->max_wp, d_wp, d_info);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return ok ? GIE_OK : GIE_ERR_DEVICE;
}
extern "C" int gie_ground_shortcut(gie_mapper *m, const int32_t *path_xy, const int32_t *len, int n, int max_len, const gie_ground_shortcut_param *p,
                                   gie_ground_waypoint *wp, gie_shortcut_info *info)
{
    int rc = gie_glos_check(m, "gie_ground_shortcut"); if (rc) return rc;
    rc = gie_ground_shortcut_args("gie_ground_shortcut", path_xy, len, n, max_len, p, wp, info); if (rc) return rc;
    if (n == 0) return GIE_OK;
    /* slot 0: the lengths, then the points.  Slot 1: the infos, then the waypoints — the caller's own bytes first, so that the
     * entries beyond a path's records come back as they were */
    const size_t lbytes = (size_t)n * 4, pbytes = (size_t)n * max_len * 8;
    const size_t ibytes = (size_t)n * sizeof(gie_shortcut_info), wbytes = (size_t)n * p->max_wp * sizeof(gie_ground_waypoint);
    char *di = (char *)gie_scratch(m, 0, lbytes + pbytes, "gie_ground_shortcut");
    char *dr = (char *)gie_scratch(m, 1, ibytes + wbytes, "gie_ground_shortcut");
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, len, lbytes);
    be_h2d(&m->be, di + lbytes, path_xy, pbytes);
    if (wbytes) be_h2d(&m->be, dr + ibytes, wp, wbytes);
    rc = gie_ground_shortcut_dev(m, (const int32_t *)(di + lbytes), (const int32_t *)di, n, max_len, p, wbytes ? (gie_ground_waypoint *)(dr + ibytes) : nullptr,
                                 (gie_shortcut_info *)dr);
    if (rc) return rc;
    if (info) be_d2h(&m->be, info, dr, ibytes);
    if (wbytes) be_d2h(&m->be, wp, dr + ibytes, wbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_los.inc.h — line of sight over the local volume: an opaque bit plane, batched segment checks and batched view gain over it
 * (include/gie.h "line of sight").
 * HIP backend only: included by gie_hip.hip after gie_frontier.inc.h; nothing of the map update reads what is computed here.
 *
 * The cache (gie_mapper::los), allocated at the first prepare:
 *   bits   one bit per voxel, opaque: rows of W = ceil(X/64) 64-bit words, bit x & 63 of word x >> 6 (as the SDF's occ plane and
 *          NF1's trav plane): 8 * ceil(X/64) / X bytes per voxel, 16.8 MB at 512^3 — what the walks read, L2 / Infinity Cache resident;
 *   type   int8 per voxel: the committed types at the prepare (the gain counts by them);
 *   edt    float per voxel: gie_edt_value at the prepare (a segment's min_edt);
 *   w      GIE_LOS_NWORDS control words (the count of opaque voxels).
 * type and edt are copies because a result belongs to its prepare whatever the map does afterwards.
 *   k_los_prep      a lane per voxel, a wave per row word: the three planes;
 *   k_los_count     the plane's popcount, one atomic per workgroup of a fixed small grid;
 *   k_los_segments  a lane per segment: the walk of L(a, b), a bit test per step, edt at the visited voxels up to the first hit;
 *   k_los_gain      a workgroup per (view, z-slice of the candidate box), a wave per row, a lane per candidate: each candidate walks
 *                   TOWARDS the view's voxel (L(v, p) is L(p, v) reversed, and most occluders sit near the candidate's surface),
 *                   leaves at its first opaque voxel; ballot popcounts per wave, one set of atomics per workgroup.
 * The walk (gie_los_walk): crossing j of axis k lies at t = (2j - 1) / (2 n_k) = (2j - 1) * M_k / (2 P), P the product of the
 * non-zero n and M_k = P / n_k — so the integers T_k = (2j - 1) * M_k order the crossings exactly (below 2^32: 64-bit), a step is
 * the minimum of three of them and every axis equal to it moves.  Sums of integers and exact comparisons only: a result does not
 * depend on scheduling.
 */

enum { GIE_LOS_W_NOPQ = 0,      /* opaque voxels */
       GIE_LOS_NWORDS = 4 };
#define GIE_LOS_T_DONE 0x7fffffffffffffffll

struct gie_los_dev {
    uint64_t *bits;
    int8_t *type;
    float *edt;
    int32_t *w;
    int W, nwords;
    int pvt[3];
};
struct gie_los_gain_arg { float rmin2, rmax2, tan2; int R; };

__global__ __launch_bounds__(256) void k_los_prep(const gie_ctx c, const gie_los_dev s, const float clearance, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane;
    bool op = false;
    if (x < c.X) {
        const int id = row * c.X + x;
        const int8_t ty = c.glb_type[id];
        const float e = gie_edt_value(c, id);
        s.type[id] = ty; s.edt[id] = e;
        op = ty == GIE_VOX_OCCUPIED || (ty == GIE_VOX_UNKNOWN && (flags & GIE_LOS_UNKNOWN_OPAQUE)) || (clearance > 0.f && e < clearance);
    }
    const uint64_t m = __ballot(op);
    if (lane == 0) s.bits[wd] = m;
}
/* the popcount of the plane: GIE_LOS_COUNT_WGS workgroups stride over its words, one atomic each (an atomic per workgroup of
 * k_los_prep, half a million on one address at 512^3, took ten times the kernel's own time) */
#define GIE_LOS_COUNT_WGS 256
__global__ __launch_bounds__(256) void k_los_count(const gie_los_dev s)
{
    __shared__ int s_n[4];
    int n = 0;
    for (int wd = blockIdx.x * 256 + threadIdx.x; wd < s.nwords; wd += GIE_LOS_COUNT_WGS * 256) n += __popcll(s.bits[wd]);
    for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) { const int t = s_n[0] + s_n[1] + s_n[2] + s_n[3]; if (t) gie_aadd32(&s.w[GIE_LOS_W_NOPQ], t); }
}
__global__ void k_los_count_out(const gie_los_dev s, int32_t *d_n_opaque) { if (blockIdx.x == 0 && threadIdx.x == 0) *d_n_opaque = s.w[GIE_LOS_W_NOPQ]; }

GIE_DEV bool gie_los_opaque(const gie_ctx &c, const gie_los_dev &s, const int x, const int y, const int z)
{
    return (s.bits[((size_t)z * c.Y + y) * s.W + (x >> 6)] >> (x & 63)) & 1ull;
}

/* the walk of L(a, b): T_k the next crossing of axis k (GIE_LOS_T_DONE: none left), D_k the distance between two of them */
struct gie_los_walk { long long T[3], D[3]; int left[3], s[3]; };
GIE_DEV void gie_los_walk_init(gie_los_walk &w, const int a[3], const int b[3])
{
    int n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { const int d = b[k] - a[k]; n[k] = d < 0 ? -d : d; w.s[k] = d < 0 ? -1 : 1; w.left[k] = n[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int n1 = n[(k + 1) % 3], n2 = n[(k + 2) % 3];
        const long long M = (long long)(n1 ? n1 : 1) * (long long)(n2 ? n2 : 1);
        w.D[k] = 2 * M; w.T[k] = n[k] ? M : GIE_LOS_T_DONE;
    }
}
/* the next voxel of the line into v; false when v is the last one */
GIE_DEV bool gie_los_walk_step(gie_los_walk &w, int v[3])
{
    long long t = w.T[0] < w.T[1] ? w.T[0] : w.T[1];
    t = t < w.T[2] ? t : w.T[2];
    if (t == GIE_LOS_T_DONE) return false;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (w.T[k] == t) { v[k] += w.s[k]; w.left[k] -= 1; w.T[k] = w.left[k] ? w.T[k] + w.D[k] : GIE_LOS_T_DONE; }
    return true;
}

__global__ __launch_bounds__(256) void k_los_segments(const gie_ctx c, const gie_los_dev s, const float *a_xyz, const float *b_xyz, const int n, gie_los_hit *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int a[3], b[3];
    gie_los_hit h;
    if (!gie_nf1_voxel(c, s.pvt[0], s.pvt[1], s.pvt[2], a_xyz + 3 * (size_t)i, a) || !gie_nf1_voxel(c, s.pvt[0], s.pvt[1], s.pvt[2], b_xyz + 3 * (size_t)i, b)) {
        h.first = -2; h.len = 0; h.hit[0] = h.hit[1] = h.hit[2] = 0; h.min_edt = 0.f;
        out[i] = h;
        return;
    }
    gie_los_walk w;
    gie_los_walk_init(w, a, b);
    int v[3] = { a[0], a[1], a[2] }, idx = 0, first = -1;
    float me = s.edt[gie_lid(c, a[0], a[1], a[2])];
    h.hit[0] = b[0]; h.hit[1] = b[1]; h.hit[2] = b[2];
    for (;;) {
        if (first < 0) {                                        /* (after the hit only the length is still wanted: no loads) */
            const float e = s.edt[gie_lid(c, v[0], v[1], v[2])];
            me = e < me ? e : me;
            if (gie_los_opaque(c, s, v[0], v[1], v[2])) { first = idx; h.hit[0] = v[0]; h.hit[1] = v[1]; h.hit[2] = v[2]; }
        }
        if (!gie_los_walk_step(w, v)) break;
        idx++;
    }
    h.first = first; h.len = idx + 1; h.min_edt = me;
#pragma unroll
    for (int k = 0; k < 3; k++) h.hit[k] += s.pvt[k];
    out[i] = h;
}

/* what the host form refuses and the _dev form scores -1 */
GIE_DEVM bool gie_los_view_ok(const gie_view &vw)
{
    if (vw.n_planes < 0 || vw.n_planes > 4) return false;
    for (int i = 0; i < vw.n_planes; i++)
        for (int k = 0; k < 3; k++) if (vw.normal[i][k] < -32767 || vw.normal[i][k] > 32767) return false;
    return true;
}
/* a lane per view: zeros for k_los_gain's atomics, -1 for a view that has no voxel */
__global__ __launch_bounds__(256) void k_los_gain_init(const gie_ctx c, const gie_los_dev s, const gie_view *views, const int n, gie_view_score *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const gie_view vw = views[i];
    int p[3];
    const int v = (gie_los_view_ok(vw) && gie_nf1_voxel(c, s.pvt[0], s.pvt[1], s.pvt[2], vw.pos, p)) ? 0 : -1;
    gie_view_score q; q.unknown = q.frontier = q.occupied = q.candidates = v;
    out[i] = q;
}
__global__ __launch_bounds__(256) void k_los_gain(const gie_ctx c, const gie_los_dev s, const gie_view *views, const gie_los_gain_arg g, gie_view_score *out)
{
    __shared__ int s_cnt[4][4];
    const int view = blockIdx.x, wv = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const gie_view vw = views[view];
    int p[3];
    if (!gie_los_view_ok(vw) || !gie_nf1_voxel(c, s.pvt[0], s.pvt[1], s.pvt[2], vw.pos, p)) return;      /* workgroup-uniform */
    const int z = p[2] - g.R + (int)blockIdx.y;
    if (z < 0 || z >= c.Z) return;                              /* workgroup-uniform */
    const int x0 = p[0] - g.R > 0 ? p[0] - g.R : 0, x1 = p[0] + g.R < c.X - 1 ? p[0] + g.R : c.X - 1;
    const int y0 = p[1] - g.R > 0 ? p[1] - g.R : 0, y1 = p[1] + g.R < c.Y - 1 ? p[1] + g.R : c.Y - 1;
    const int dz = z - p[2];
    int nu = 0, nf = 0, no = 0, nc = 0;
#pragma unroll 1
    for (int y = y0 + wv; y <= y1; y += 4) {
        const int dy = y - p[1];
#pragma unroll 1
        for (int xb = x0; xb <= x1; xb += 64) {
            const int x = xb + lane, dx = x - p[0];
            const int dh = dx * dx + dy * dy, d2 = dh + dz * dz;
            bool cand = x <= x1 && d2 != 0 && (float)d2 >= g.rmin2 && (float)d2 <= g.rmax2;
            if (cand && g.tan2 >= 0.f) cand = (float)(dz * dz) <= g.tan2 * (float)dh;
            for (int i = 0; cand && i < vw.n_planes; i++)
                cand = (long long)vw.normal[i][0] * dx + (long long)vw.normal[i][1] * dy + (long long)vw.normal[i][2] * dz >= 0;
            bool vis = cand;
            int ty = -1;
            if (cand) {
                int v[3] = { x, y, z };
                gie_los_walk w;
                gie_los_walk_init(w, v, p);
                while (gie_los_walk_step(w, v)) {
                    if ((w.left[0] | w.left[1] | w.left[2]) == 0) break;       /* v is p: its opacity is ignored */
                    if (gie_los_opaque(c, s, v[0], v[1], v[2])) { vis = false; break; }
                }
                if (vis) ty = s.type[gie_lid(c, x, y, z)];
            }
            nc += __popcll(__ballot(cand));
            nu += __popcll(__ballot(ty == GIE_VOX_UNKNOWN));
            nf += __popcll(__ballot(ty == GIE_VOX_FNT));
            no += __popcll(__ballot(ty == GIE_VOX_OCCUPIED));
        }
    }
    if (lane == 0) { s_cnt[wv][0] = nu; s_cnt[wv][1] = nf; s_cnt[wv][2] = no; s_cnt[wv][3] = nc; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int t = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (t) gie_aadd32(&out[view].unknown + threadIdx.x, t);
    }
}

struct op_los_bytes {
    const uint64_t *bits; int W; uint8_t *out;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int row = i / c.X, x = i - row * c.X;
        out[i] = (uint8_t)((bits[(size_t)row * W + (x >> 6)] >> (x & 63)) & 1ull);
    }
};

/* ---- host side */
static gie_los_dev gie_los_view(const gie_mapper *m)
{
    const gie_ctx &c = m->c;
    gie_los_dev s;
    s.W = (c.X + 63) / 64; s.nwords = s.W * c.Y * c.Z;
    s.bits = m->los.bits; s.type = m->los.type; s.edt = m->los.edt; s.w = m->los.words;
    for (int i = 0; i < 3; i++) s.pvt[i] = m->los.pvt[i];
    return s;
}
static int gie_los_check(gie_mapper *m, const char *who, bool need_plane)
{
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) { gie_set_err(std::string(who) + ": not for a tiled mapper (its lines would stop at the tile's faces)"); return GIE_ERR_INVALID; }
    if (need_plane && !m->los.valid) { gie_set_err(std::string(who) + ": no opaque plane yet (gie_los_prepare first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_los_prepare_dev(gie_mapper *m, const gie_los_param *p, int32_t *d_n_opaque)
{
    static_assert(sizeof(gie_los_hit) == 24 && sizeof(gie_view) == 64 && sizeof(gie_view_score) == 16, "the sizes include/gie.h states");
    int rc = gie_los_check(m, "gie_los_prepare_dev", false); if (rc) return rc;
    if (!p) { gie_set_err("gie_los_prepare_dev: null parameters"); return GIE_ERR_INVALID; }
    if (!(p->clearance >= 0.f && p->clearance <= 3.402823466e38f)) { gie_set_err("gie_los_prepare_dev: clearance must be finite and >= 0"); return GIE_ERR_INVALID; }
    if (p->flags & ~GIE_LOS_UNKNOWN_OPAQUE) { gie_set_err("gie_los_prepare_dev: unknown flags"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this stage) */
    const int nwords = ((c.X + 63) / 64) * c.Y * c.Z;
    if (!m->los.bits) {
        uint64_t *bits = gie_dalloc<uint64_t>(m, (size_t)nwords, false);
        float *edt = bits ? gie_dalloc<float>(m, (size_t)c.N, false) : nullptr;
        int8_t *type = edt ? gie_dalloc<int8_t>(m, (size_t)c.N, false) : nullptr;
        int32_t *words = type ? gie_dalloc<int32_t>(m, GIE_LOS_NWORDS, false) : nullptr;
        if (!words) { gie_set_err("gie_los_prepare_dev: device allocation of the line-of-sight planes failed"); return GIE_ERR_DEVICE; }
        m->los.bits = bits; m->los.edt = edt; m->los.type = type; m->los.words = words;
    }
    for (int i = 0; i < 3; i++) m->los.pvt[i] = c.pvt[i];
    const gie_los_dev s = gie_los_view(m);
    be_prof(&m->be, GIE_K_LOS, 0);
    be_memset(&m->be, s.w, 0, GIE_LOS_NWORDS * sizeof(int32_t));
    GIE_LAUNCH(&m->be, k_los_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, s, p->clearance, (int)p->flags);
    GIE_LAUNCH(&m->be, k_los_count, dim3(GIE_LOS_COUNT_WGS), dim3(256), 0, s);
    if (d_n_opaque) GIE_LAUNCH(&m->be, k_los_count_out, dim3(1), dim3(64), 0, s, d_n_opaque);
    be_prof(&m->be, GIE_K_LOS, 1);
    m->los.valid = 1;
    return GIE_OK;
}
extern "C" int gie_los_prepare(gie_mapper *m, const gie_los_param *p, int32_t *n_opaque)
{
    int rc = gie_los_check(m, "gie_los_prepare", false); if (rc) return rc;
    rc = gie_los_prepare_dev(m, p, nullptr); if (rc) return rc;
    if (n_opaque) be_d2h(&m->be, n_opaque, m->los.words + GIE_LOS_W_NOPQ, sizeof(int32_t));
    return gie_sync(m);
}
extern "C" int gie_read_los_opaque_dev(gie_mapper *m, uint8_t *d_opaque)
{
    int rc = gie_los_check(m, "gie_read_los_opaque_dev", true); if (rc) return rc;
    if (!d_opaque) { gie_set_err("gie_read_los_opaque_dev: null output"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;
    op_los_bytes op; op.bits = m->los.bits; op.W = (c.X + 63) / 64; op.out = d_opaque;
    be_prof(&m->be, GIE_K_LOS, 0);
    be_lin(&m->be, c, op, c.N);
    be_prof(&m->be, GIE_K_LOS, 1);
    return GIE_OK;
}
extern "C" int gie_read_los_opaque(gie_mapper *m, uint8_t *opaque)
{
    int rc = gie_los_check(m, "gie_read_los_opaque", true); if (rc) return rc;
    if (!opaque) { gie_set_err("gie_read_los_opaque: null output"); return GIE_ERR_INVALID; }
    const size_t N = (size_t)m->c.N;
    uint8_t *d = (uint8_t *)gie_scratch(m, 1, N, "gie_read_los_opaque");
    if (!d) return GIE_ERR_DEVICE;
    rc = gie_read_los_opaque_dev(m, d); if (rc) return rc;
    be_d2h(&m->be, opaque, d, N);
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_los_segments_dev(gie_mapper *m, const float *d_a_xyz, const float *d_b_xyz, int n, gie_los_hit *d_out)
{
    int rc = gie_los_check(m, "gie_los_segments_dev", true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_a_xyz || !d_b_xyz || !d_out))) { gie_set_err("gie_los_segments_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    gie_ctx c = m->c;
    c.gate = nullptr;
    be_prof(&m->be, GIE_K_LOS_QUERY, 0);
    GIE_LAUNCH(&m->be, k_los_segments, dim3((n + 255) / 256), dim3(256), 0, c, gie_los_view(m), d_a_xyz, d_b_xyz, n, d_out);
    be_prof(&m->be, GIE_K_LOS_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_los_segments(gie_mapper *m, const float *a_xyz, const float *b_xyz, int n, gie_los_hit *out)
{
    int rc = gie_los_check(m, "gie_los_segments", true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!a_xyz || !b_xyz || !out))) { gie_set_err("gie_los_segments: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 24, "gie_los_segments");          /* a, then b */
    gie_los_hit *dr = (gie_los_hit *)gie_scratch(m, 1, (size_t)n * sizeof(gie_los_hit), "gie_los_segments");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, a_xyz, (size_t)n * 12);
    be_h2d(&m->be, dx + 3 * (size_t)n, b_xyz, (size_t)n * 12);
    rc = gie_los_segments_dev(m, dx, dx + 3 * (size_t)n, n, dr); if (rc) return rc;
    be_d2h(&m->be, out, dr, (size_t)n * sizeof(gie_los_hit));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_view_gain_dev(gie_mapper *m, const gie_view *d_views, int n, const gie_view_param *vp, gie_view_score *d_out)
{
    int rc = gie_los_check(m, "gie_view_gain_dev", true); if (rc) return rc;
    if (!vp || n < 0 || (n > 0 && (!d_views || !d_out))) { gie_set_err("gie_view_gain_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (!(vp->r_min >= 0.f && vp->r_min <= vp->r_max && vp->r_max <= 3.402823466e38f) || vp->tan2_elev != vp->tan2_elev) {
        gie_set_err("gie_view_gain_dev: 0 <= r_min <= r_max, both finite, and tan2_elev not NaN"); return GIE_ERR_INVALID;
    }
    if (n == 0) return GIE_OK;
    gie_ctx c = m->c;
    c.gate = nullptr;
    const float rmin = vp->r_min / c.voxel_width, rmax = vp->r_max / c.voxel_width;
    gie_los_gain_arg g;
    g.rmin2 = rmin * rmin; g.rmax2 = rmax * rmax; g.tan2 = vp->tan2_elev;
    /* the largest |d_k| of a candidate: the largest integer whose square passes the test against rmax * rmax AS ROUNDED (no side
     * of a volume exceeds 1024) */
    g.R = rmax >= 1024.f ? 1024 : (int)rmax;
    if (g.R < 1024 && (float)((g.R + 1) * (g.R + 1)) <= g.rmax2) g.R += 1;
    const gie_los_dev s = gie_los_view(m);
    be_prof(&m->be, GIE_K_LOS_QUERY, 0);
    GIE_LAUNCH(&m->be, k_los_gain_init, dim3((n + 255) / 256), dim3(256), 0, c, s, d_views, n, d_out);
    GIE_LAUNCH(&m->be, k_los_gain, dim3(n, 2 * g.R + 1), dim3(256), 0, c, s, d_views, g, d_out);
    be_prof(&m->be, GIE_K_LOS_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_view_gain(gie_mapper *m, const gie_view *views, int n, const gie_view_param *vp, gie_view_score *out)
{
    int rc = gie_los_check(m, "gie_view_gain", true); if (rc) return rc;
    if (!vp || n < 0 || (n > 0 && (!views || !out))) { gie_set_err("gie_view_gain: bad arguments"); return GIE_ERR_INVALID; }
    for (int i = 0; i < n; i++) {
        bool ok = views[i].n_planes >= 0 && views[i].n_planes <= 4;
        for (int j = 0; ok && j < views[i].n_planes; j++)
            for (int k = 0; k < 3; k++) ok = ok && views[i].normal[j][k] >= -32767 && views[i].normal[j][k] <= 32767;
        if (!ok) { gie_set_err("gie_view_gain: a view has n_planes outside 0..4 or a normal component beyond +-32767"); return GIE_ERR_INVALID; }
    }
    gie_view *dv = nullptr;
    gie_view_score *dr = nullptr;
    if (n > 0) {
        dv = (gie_view *)gie_scratch(m, 0, (size_t)n * sizeof(gie_view), "gie_view_gain");
        dr = (gie_view_score *)gie_scratch(m, 1, (size_t)n * sizeof(gie_view_score), "gie_view_gain");
        if (!dv || !dr) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dv, views, (size_t)n * sizeof(gie_view));
    }
    rc = gie_view_gain_dev(m, dv, n, vp, dr); if (rc) return rc;
    if (n == 0) return GIE_OK;
    be_d2h(&m->be, out, dr, (size_t)n * sizeof(gie_view_score));
    gie_scratch_trim(m);
    return gie_sync(m);
}

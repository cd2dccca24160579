/*
 * gie_ground_view.inc.h — ground view gain: how many cells of the ground field a sensor would see from each of n candidate poses, and
 * the mask of one pose (include/gie.h "ground view gain").
 * HIP backend only: included by gie_hip.hip after gie_ground_costmat.inc.h.  It reads the ground field's type plane and writes nothing
 * of the map, of that field, of the ground navigation function or of the frontier clusters; its one plane is allocated at the first
 * call.
 *   k_gview_prep    k_glos_prep's form, a lane per cell and a wave per 64-cell word: the bit row opq = opaque (rows of W = ceil(X/64)
 *                   words, bit x & 63 of word x >> 6; the padding bits beyond X are SET), and, for the mask form, the mask's zeros.
 *                   In front of the words the launch's threads stride over the n scores: 0 for k_ground_gain's atomics, -1 for a
 *                   view without a cell (or with a normal beyond +-32767).  One launch in front of every gain launch: no result is
 *                   kept, a call sees the field as it stands where it is enqueued.
 *   k_ground_gain   S workgroups per view, workgroup (view, strip) takes H of the view's candidate rows (the rows p_y - Rc .. p_y + Rc,
 *                   Rc = min(R, Y - 1), cut at the rectangle).  It copies the opaque words of the bounding box of p and its strip's
 *                   candidates — the rows between p's and the strip's, the word columns of x = p_x - R .. p_x + R — into dynamic LDS:
 *                   every cell of L2(p, v) lies in the bounding box of p and v.  Then a wave takes a unit of 64 cells of one row at a
 *                   time (unit u of the strip's rows x ceil(columns / 64), u = wave + 4 k: the same bounds in all lanes), a lane one
 *                   candidate: the float tests, the sector test, its type byte (one row read per wave), and the walk of L2 from v
 *                   TOWARDS p (L2(v, p) is L2(p, v) reversed, and most occluders sit near the candidate), a bit test in LDS per step,
 *                   leaving at the first opaque cell; p's own cell ends the walk untested.  The walk loop issues no global load.
 *                   Ballot popcounts per wave, LDS per workgroup, one set of four integer atomics per workgroup.  MASK = true also
 *                   stores 1 (hidden) or 2 (visible) at every candidate; the zeros are k_gview_prep's.
 * The launch shape (host): H = ceil(span * n / GIE_GVIEW_TARGET_WGS) clamped to 1 .. span, span = 2 Rc + 1, S = ceil(span / H): about
 * GIE_GVIEW_TARGET_WGS workgroups whatever n and the radius are — one large view spreads over the machine in strips of a row or two,
 * 256 small views get a few strips each, and beyond that a view is one workgroup.  The dynamic LDS is the largest box a strip of that
 * shape can have, min(Y, max(Rc + 1, H)) rows of min(W, 2 R / 64 + 2) words: 128 KiB at most (sides <= 1024), a few hundred bytes for
 * a small radius — there is no other form.
 * R only bounds the box and may only over-cover: the float test against rmax * rmax decides alone.
 * Integers and exact float comparisons, sums of integers: a result does not depend on scheduling.  No grid barrier.
 * The compiler's figures and the times are in DESIGN.md 24.
 */

#define GIE_GVIEW_TARGET_WGS 1024
#define GIE_GVIEW_LDS_BYTES (128 * 1024)

struct gie_gview_arg {
    float rmin2, rmax2;     /* (r / w)^2 as rounded */
    int R;                  /* no candidate has |d_k| > R */
    int n_planes, flags;
    int H, S;               /* rows per strip, strips per view */
    int lds_words;          /* what the launch's dynamic LDS holds */
};

/* the cell of view i, and its normals into nr; false for a view that scores -1 */
GIE_DEV bool gie_gview_load(const gie_ctx &c, const gie_glos_dev &s, const gie_gview_arg &a, const float *xy, const int32_t *normals, const size_t i, int p[2], int nr[4])
{
    bool ok = gie_ground_cell_of(c.voxel_width, s.X, s.Y, s.pvt, xy + 2 * i, p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        nr[k] = 0;
        if (k < 2 * a.n_planes) {
            nr[k] = normals[2 * (size_t)a.n_planes * i + k];
            ok &= nr[k] >= -32767 && nr[k] <= 32767;
        }
    }
    return ok;
}

__global__ __launch_bounds__(256) void k_gview_prep(const gie_ctx c, const gie_ground_dev g, const gie_glos_dev s, const int nwords, const gie_gview_arg a,
                                                    const float *xy, const int32_t *normals, const long long n, gie_view_score *out, uint8_t *mask)
{
    if (out) {
        const long long stride = (long long)gridDim.x * 256;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            int p[2], nr[4];
            const int v = gie_gview_load(c, s, a, xy, normals, (size_t)i, p, nr) ? 0 : -1;
            gie_view_score q; q.unknown = q.frontier = q.occupied = q.candidates = v;
            out[i] = q;
        }
    }
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const int y = wd / s.W, x = (wd - y * s.W) * 64 + lane;
    bool op = true;                                             /* the padding bits are set */
    if (x < c.X) {
        const int id = y * c.X + x;
        const int8_t ty = g.type[id];
        op = ty == GIE_VOX_OCCUPIED || (ty == GIE_VOX_UNKNOWN && (a.flags & GIE_GROUND_VIEW_UNKNOWN_OPAQUE));
        if (mask) mask[id] = 0;
    }
    const uint64_t bt = __ballot(op);
    if (lane == 0) s.blk[wd] = bt;
}

template <bool MASK>
__global__ __launch_bounds__(256) void k_ground_gain(const gie_ctx c, const gie_ground_dev g, const gie_glos_dev s, const gie_gview_arg a, const float *xy,
                                                     const int32_t *normals, const long long view0, gie_view_score *out, uint8_t *mask)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_opq[];       /* the box's opaque words, nw per row */
    __shared__ int s_cnt[4][4];
    const size_t view = (size_t)(view0 + blockIdx.x / a.S);
    const int strip = blockIdx.x % a.S, wv = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, X = s.X, Y = s.Y;
    int p[2], nr[4];
    if (!gie_gview_load(c, s, a, xy, normals, view, p, nr)) return;        /* workgroup-uniform */
    const int Rc = a.R < Y - 1 ? a.R : Y - 1;
    const int r0 = p[1] - Rc + strip * a.H, r1 = r0 + a.H - 1, rl = p[1] + Rc < Y - 1 ? p[1] + Rc : Y - 1;
    const int ya = r0 > 0 ? r0 : 0, yb = r1 < rl ? r1 : rl;
    if (ya > yb) return;                                        /* workgroup-uniform: the strip lies outside the rectangle */
    const int xa = p[0] - a.R > 0 ? p[0] - a.R : 0, xb = p[0] + a.R < X - 1 ? p[0] + a.R : X - 1;
    const int by0 = p[1] < ya ? p[1] : ya, by1 = p[1] > yb ? p[1] : yb, bw0 = xa >> 6, nw = (xb >> 6) - bw0 + 1;
    const int nbox = (by1 - by0 + 1) * nw;
    if (nbox > a.lds_words) return;                             /* (workgroup-uniform; the host's bound covers every box: never taken) */
    for (int i = threadIdx.x; i < nbox; i += 256) {
        const int r = i / nw, wc = i - r * nw;
        s_opq[i] = s.blk[(size_t)(by0 + r) * s.W + bw0 + wc];
    }
    __syncthreads();
    const int nch = (xb - xa + 64) >> 6, nunits = (yb - ya + 1) * nch;
    int nu = 0, nf = 0, no = 0, nc = 0;
#pragma unroll 1
    for (int u = wv; u < nunits; u += 4) {                      /* wave-uniform bounds */
        const int row = u / nch, y = ya + row, x = xa + (u - row * nch) * 64 + lane;
        const int dx = x - p[0], dy = y - p[1], d2 = dx * dx + dy * dy;
        bool cand = x <= xb && d2 != 0 && (float)d2 >= a.rmin2 && (float)d2 <= a.rmax2;
        if (cand && a.n_planes > 0) {
            const bool h0 = nr[0] * dx + nr[1] * dy >= 0;
            if (a.n_planes == 1) cand = h0;
            else {
                const bool h1 = nr[2] * dx + nr[3] * dy >= 0;
                cand = (a.flags & GIE_GROUND_VIEW_UNION) ? (h0 || h1) : (h0 && h1);
            }
        }
        int ty = -1;
        if (cand) {
            const int8_t tv = g.type[(size_t)y * X + x];
            int v[2] = { x, y };
            gie_gwalk w;
            gie_gwalk_init(w, v, p);
            bool vis = true;
            while (gie_gwalk_step(w, v)) {
                if ((w.left[0] | w.left[1]) == 0) break;        /* v is p: its opacity is ignored */
                if ((s_opq[(v[1] - by0) * nw + (v[0] >> 6) - bw0] >> (v[0] & 63)) & 1ull) { vis = false; break; }
            }
            if (vis) ty = tv;
            if (MASK) mask[(size_t)y * X + x] = vis ? 2 : 1;
        }
        nc += __popcll(__ballot(cand));
        nu += __popcll(__ballot(ty == GIE_VOX_UNKNOWN));
        nf += __popcll(__ballot(ty == GIE_VOX_FNT));
        no += __popcll(__ballot(ty == GIE_VOX_OCCUPIED));
    }
    if (!out) return;                                           /* (the mask form without a score) */
    if (lane == 0) { s_cnt[wv][0] = nu; s_cnt[wv][1] = nf; s_cnt[wv][2] = no; s_cnt[wv][3] = nc; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int t = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (t) gie_aadd32(&out[view].unknown + threadIdx.x, t);
    }
}

/* ---- host side */
static int gie_gview_check(gie_mapper *m, const char *who, const float *xy, const int32_t *normals, long long n, const gie_ground_view_param *p, const void *out,
                           bool mask_form, const void *mask)
{
    static_assert(sizeof(gie_ground_view_param) == 32 && sizeof(gie_view_score) == 16, "the sizes include/gie.h states");
    const int rc = gie_glos_check(m, who); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (!(p->r_min >= 0.f && p->r_min <= p->r_max && p->r_max <= 3.402823466e38f)) bad = "0 <= r_min <= r_max, both finite";
    else if (p->n_planes < 0 || p->n_planes > 2) bad = "n_planes must be in 0..2";
    else if (p->flags & ~(GIE_GROUND_VIEW_UNKNOWN_OPAQUE | GIE_GROUND_VIEW_UNION)) bad = "unknown flags";
    else if ((p->flags & GIE_GROUND_VIEW_UNION) && p->n_planes != 2) bad = "GIE_GROUND_VIEW_UNION needs n_planes == 2";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) bad = "reserved must be 0";
    else if (n < 0) bad = "n must be >= 0";
    else if (n > 0 && (!xy || (!mask_form && !out))) bad = "n > 0 with a null buffer";
    else if (n > 0 && !normals && p->n_planes > 0) bad = "null normals with n_planes > 0";
    else if (mask_form && !mask) bad = "null mask";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* what only the host forms can refuse: a normal component beyond +-32767 */
static int gie_gview_normals(const char *who, const int32_t *normals, long long n, const gie_ground_view_param *p)
{
    const size_t k = (size_t)n * 2 * (size_t)p->n_planes;
    for (size_t i = 0; i < k; i++)
        if (normals[i] < -32767 || normals[i] > 32767) { gie_set_err(std::string(who) + ": a normal component beyond +-32767"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* the two launches (more gain launches only when n * S exceeds a grid) */
static int gie_gview_run(gie_mapper *m, const char *who, const float *d_xy, const int32_t *d_normals, long long n, const gie_ground_view_param *p,
                         gie_view_score *d_out, uint8_t *d_mask)
{
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const int nwords = g.W * c.Y;
    static bool attr_done = false;
    const int ra = gie_ground_lds_limit(&attr_done, who, reinterpret_cast<const void *>(&k_ground_gain<true>), reinterpret_cast<const void *>(&k_ground_gain<false>),
                                        GIE_GVIEW_LDS_BYTES);
    if (ra) return ra;
    if (!m->gview_opq) {
        m->gview_opq = gie_dalloc<uint64_t>(m, (size_t)nwords, false);
        if (!m->gview_opq) { gie_set_err(std::string(who) + ": device allocation of the opaque plane failed"); return GIE_ERR_DEVICE; }
    }
    gie_glos_dev s;
    s.blk = m->gview_opq; s.dist = g.dist; s.W = g.W; s.X = c.X; s.Y = c.Y; s.pvt[0] = g.pvt[0]; s.pvt[1] = g.pvt[1];
    const float rmin = p->r_min / c.voxel_width, rmax = p->r_max / c.voxel_width;
    gie_gview_arg a;
    a.rmin2 = rmin * rmin; a.rmax2 = rmax * rmax; a.n_planes = (int)p->n_planes; a.flags = (int)p->flags;
    /* |d_k| <= sqrt(rmax2) < rmax + 1 while rmax < 1023 (one rounding of the product); beyond that the field's side bounds it */
    a.R = rmax >= 1023.f ? 1024 : (int)rmax + 1;
    const int Rc = a.R < c.Y - 1 ? a.R : c.Y - 1, span = 2 * Rc + 1;
    long long H = ((long long)span * n + GIE_GVIEW_TARGET_WGS - 1) / GIE_GVIEW_TARGET_WGS;
    a.H = H < 1 ? 1 : (H > span ? span : (int)H);
    a.S = (span + a.H - 1) / a.H;
    const int rows = std::min(c.Y, std::max(Rc + 1, a.H)), words = std::min(g.W, 2 * a.R / 64 + 2);
    a.lds_words = rows * words;                                 /* <= 1024 * 16 */
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    GIE_LAUNCH(&m->be, k_gview_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, g, s, nwords, a, d_xy, d_normals, n, d_out, d_mask);
    const long long per = (1ll << 30) / a.S;                    /* views of one launch */
    for (long long v0 = 0; v0 < n; v0 += per) {
        const long long k = n - v0 < per ? n - v0 : per;
        const dim3 grid((unsigned)(k * a.S));
        if (d_mask) GIE_LAUNCH(&m->be, k_ground_gain<true>, grid, dim3(256), (size_t)a.lds_words * sizeof(uint64_t), c, g, s, a, d_xy, d_normals, v0, d_out, d_mask);
        else GIE_LAUNCH(&m->be, k_ground_gain<false>, grid, dim3(256), (size_t)a.lds_words * sizeof(uint64_t), c, g, s, a, d_xy, d_normals, v0, d_out, d_mask);
    }
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return GIE_OK;
}

extern "C" int gie_ground_view_gain_dev(gie_mapper *m, const float *d_xy, const int32_t *d_normals, int n, const gie_ground_view_param *p, gie_view_score *d_out)
{
    const int rc = gie_gview_check(m, "gie_ground_view_gain_dev", d_xy, d_normals, n, p, d_out, false, nullptr); if (rc) return rc;
    if (n == 0) return GIE_OK;
    return gie_gview_run(m, "gie_ground_view_gain_dev", d_xy, d_normals, n, p, d_out, nullptr);
}
extern "C" int gie_ground_view_gain(gie_mapper *m, const float *xy, const int32_t *normals, int n, const gie_ground_view_param *p, gie_view_score *out)
{
    int rc = gie_gview_check(m, "gie_ground_view_gain", xy, normals, n, p, out, false, nullptr); if (rc) return rc;
    if (n == 0) return GIE_OK;
    rc = gie_gview_normals("gie_ground_view_gain", normals, n, p); if (rc) return rc;
    const size_t xbytes = (size_t)n * 8, nbytes = (size_t)n * 8 * (size_t)p->n_planes;
    char *di = (char *)gie_scratch(m, 0, xbytes + nbytes, "gie_ground_view_gain");               /* the points, then the normals */
    gie_view_score *dr = (gie_view_score *)gie_scratch(m, 1, (size_t)n * sizeof(gie_view_score), "gie_ground_view_gain");
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, xy, xbytes);
    if (nbytes) be_h2d(&m->be, di + xbytes, normals, nbytes);
    rc = gie_gview_run(m, "gie_ground_view_gain", (const float *)di, nbytes ? (const int32_t *)(di + xbytes) : nullptr, n, p, dr, nullptr); if (rc) return rc;
    be_d2h(&m->be, out, dr, (size_t)n * sizeof(gie_view_score));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_ground_view_mask_dev(gie_mapper *m, const float *d_xy, const int32_t *d_normals, const gie_ground_view_param *p, uint8_t *d_mask, gie_view_score *d_score)
{
    const int rc = gie_gview_check(m, "gie_ground_view_mask_dev", d_xy, d_normals, 1, p, d_score, true, d_mask); if (rc) return rc;
    return gie_gview_run(m, "gie_ground_view_mask_dev", d_xy, d_normals, 1, p, d_score, d_mask);
}
extern "C" int gie_ground_view_mask(gie_mapper *m, const float *xy, const int32_t *normals, const gie_ground_view_param *p, uint8_t *mask, gie_view_score *score)
{
    int rc = gie_gview_check(m, "gie_ground_view_mask", xy, normals, 1, p, score, true, mask); if (rc) return rc;
    rc = gie_gview_normals("gie_ground_view_mask", normals, 1, p); if (rc) return rc;
    const size_t cells = (size_t)m->c.X * m->c.Y, nbytes = 8 * (size_t)p->n_planes;
    char *di = (char *)gie_scratch(m, 0, 8 + nbytes, "gie_ground_view_mask");                    /* the point, then the normals */
    char *dr = (char *)gie_scratch(m, 1, sizeof(gie_view_score) + cells, "gie_ground_view_mask");   /* the score, then the mask */
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, xy, 8);
    if (nbytes) be_h2d(&m->be, di + 8, normals, nbytes);
    rc = gie_gview_run(m, "gie_ground_view_mask", (const float *)di, nbytes ? (const int32_t *)(di + 8) : nullptr, 1, p, (gie_view_score *)dr,
                       (uint8_t *)dr + sizeof(gie_view_score));
    if (rc) return rc;
    if (score) be_d2h(&m->be, score, dr, sizeof(gie_view_score));
    be_d2h(&m->be, mask, dr + sizeof(gie_view_score), cells);
    gie_scratch_trim(m);
    return gie_sync(m);
}

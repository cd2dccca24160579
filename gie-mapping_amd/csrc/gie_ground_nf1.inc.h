/*
 * gie_ground_nf1.inc.h — the NF1 navigation function of the ground costmap and its descent paths (include/gie.h "ground navigation
 * function").
 * HIP backend only: included by gie_hip.hip after gie_ground.inc.h.  It reads the ground field's type and dist_sq planes and writes
 * nothing of the map or of that field; its own planes are per CELL (x, y) and are allocated at the first compute.
 *   k_gnf1_prep    one lane per cell, a wave per 64-cell word (k_nf1_prep's form): the field at -1, the FNT sources at 0, the bit
 *                  row blk = ~traversable | source ("blocked or visited": rows of W = ceil(X/64) words, bit x & 63 of word x >> 6;
 *                  the padding bits beyond X are SET) and the level-0 frontier fr (padding bits clear).
 *   k_gnf1_goals   one lane per goal point (k_nf1_goals' form): ONE atomic OR on blk decides whether the goal's cell becomes a source.
 *   k_gnf1_bfs     ONE workgroup of 1024 threads runs the whole propagation.  A thread owns the words tid + 1024 k.  Level L, for every
 *                  own word:
 *                    next = (F | F << 1 | F >> 1 | carries of the words left and right | the words of rows y - 1, y + 1) & ~blk
 *                  goes to a plane of its own in LDS, blk |= next (blk is only ever touched by a word's owner) and L + 1 to the
 *                  field at each new bit; "any bit new" is ORed in LDS and ONE workgroup barrier ends the level (the loop ends on
 *                  0).  A 2-D bit plane is small: with three planes — next, F, blk — of at most GIE_GNF1_LDS_BYTES the kernel
 *                  copies F and blk into LDS first, next and F swap after the barrier, and the level loop touches global memory
 *                  only to write new values (LDS = true: dynamic shared memory above the 64 KB default, raised with
 *                  hipFuncSetAttribute).  A larger field runs the same loop on F and blk where they lie, with next still in LDS
 *                  (16 x 1024 words at most, 128 KiB) and copied to F behind a second barrier (LDS = false).  The host picks the
 *                  form by the size alone.  Holding next in registers between two barriers instead would need an array sized by
 *                  the field: 16 words a thread on global planes cost 300 bytes of scratch per lane.  No grid barrier, no
 *                  cooperative residency: the launch is no member of the chain of grid-barrier launches and has no timeout
 *                  path; the level count is bounded by X * Y whatever the planes hold.
 *   k_gnf1_path    one lane per start point (k_nf1_path's form in the plane).
 *   k_gnf1_query   one lane per point: the gather of the field (the route costs to gie_ground_frontier.inc.h's goals).
 *   exports        one lane per cell (k_lin).
 * The compiler's figures and the times are in DESIGN.md 20.
 */

#define GIE_GNF1_THREADS 1024
#define GIE_GNF1_LDS_BYTES (144 * 1024)                         /* the LDS budget of the kernel's bit planes: 160 KiB less room for its other words */
#define GIE_GNF1_LDS_WORDS (GIE_GNF1_LDS_BYTES / 24)            /* words of ONE plane when three fit: 6144 */
enum { GIE_GNF1_W_SRC = 0,      /* sources of the current field */
       GIE_GNF1_NWORDS = 4 };

struct gie_gnf1_dev {
    int32_t *f;             /* X * Y: the field */
    uint64_t *blk, *fr;     /* W words per row y: blocked or visited; the frontier of level 0 */
    int32_t *w;             /* control words */
    int W;
};

/* prep (a): the bit rows, the field at -1 and the FNT sources at 0 */
__global__ __launch_bounds__(256) void k_gnf1_prep(const gie_ctx c, const gie_ground_dev g, const gie_gnf1_dev s, const int nwords,
                                                   const int clearance_sq, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const bool none = gie_ground_nobs(g) == 0;                  /* no obstacle column: dist_sq is -1 everywhere */
    const int y = wd / s.W, x = (wd - y * s.W) * 64 + lane;
    bool tr = false, src = false;
    if (x < c.X) {
        const int id = y * c.X + x;
        tr = gie_ground_traversable(g, id, none, clearance_sq, flags & GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE);
        src = tr && g.type[id] == GIE_VOX_FNT && (flags & GIE_GROUND_NF1_FROM_FRONTIERS);
        s.f[id] = src ? 0 : -1;
    }
    const uint64_t bt = __ballot(tr), bs = __ballot(src);
    if (lane == 0) { s.blk[wd] = ~bt | bs; s.fr[wd] = bs; }
}

/* prep (b): one lane per goal point; gie_ground_query's mapping of a point to its cell; traversable goals join the sources */
__global__ __launch_bounds__(256) void k_gnf1_goals(const gie_ctx c, const gie_gnf1_dev s, const int pvt0, const int pvt1, const float *xy, const int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int S[2] = { c.X, c.Y }, P[2] = { pvt0, pvt1 };
    int v[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {                               /* (gie_ground_cell_of, written out: through the function the kernel's register count changes) */
        const float u = floorf(xy[2 * (size_t)p + k] / c.voxel_width + 0.5f);
        if (!(u >= -1.0e9f && u <= 1.0e9f)) return;
        v[k] = (int)u - P[k];
        if (v[k] < 0 || v[k] >= S[k]) return;
    }
    const int wd = v[1] * s.W + (v[0] >> 6);
    const unsigned long long bit = 1ull << (v[0] & 63);
    if (atomicOr((unsigned long long *)&s.blk[wd], bit) & bit) return;       /* blocked, or a source already */
    atomicOr((unsigned long long *)&s.fr[wd], bit);
    s.f[v[1] * c.X + v[0]] = 0;
}

/* the propagation: one workgroup, a level per workgroup barrier (two on global planes) */
template <bool LDS>
__global__ __launch_bounds__(GIE_GNF1_THREADS) void k_gnf1_bfs(const gie_ctx c, const gie_gnf1_dev s, const int nwords, int32_t *n_sources)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_planes[];     /* next; in the LDS form the frontier and blk behind it */
    __shared__ int s_cnt[GIE_GNF1_THREADS / 64], s_any[3];     /* s_any[L % 3]: some wave found a new bit in level L */
    uint64_t *NX = s_planes, *F = LDS ? s_planes + nwords : s.fr, *B = LDS ? s_planes + 2 * (size_t)nwords : s.blk;
    const int tid = threadIdx.x, W = s.W, X = c.X, Y = c.Y;
    const gie_ground_words w0 = gie_ground_words_first(tid, GIE_GNF1_THREADS, W);
    int n = 0;
    for (int wd = tid; wd < nwords; wd += GIE_GNF1_THREADS) {   /* the sources counted, the planes into LDS */
        const uint64_t f = s.fr[wd];
        n += __popcll(f);
        if (LDS) { F[wd] = f; B[wd] = s.blk[wd]; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = n;
    if (tid == 0) s_any[0] = s_any[1] = s_any[2] = 0;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int i = 0; i < GIE_GNF1_THREADS / 64; i++) t += s_cnt[i];
        s.w[GIE_GNF1_W_SRC] = t;
        if (n_sources) *n_sources = t;
    }
    const int max_levels = X * Y;                               /* no path is longer: the loop ends here whatever the planes hold */
#pragma unroll 1
    for (int level = 0; level < max_levels; level++) {
        if (tid == 0) s_any[(level + 1) % 3] = 0;               /* (last read after the barrier of level - 2, next set in level + 1) */
        int any = 0;
        gie_ground_words w = w0;
#pragma unroll 1
        for (int wd = tid; wd < nwords; wd += GIE_GNF1_THREADS) {
            const uint64_t d = gie_ground_dilate4(F, wd, w.tx, w.y, W, Y), bl = B[wd], nx = d & ~bl;        /* (blk holds the padding bits beyond X; only its owner touches a word of it) */
            NX[wd] = nx;
            if (nx) {
                any = 1;
                B[wd] = bl | nx;
                int32_t *fr = s.f + (size_t)w.y * X + w.tx * 64;
                for (uint64_t b = nx; b; b &= b - 1) fr[__builtin_ctzll(b)] = level + 1;
            }
            gie_ground_words_next(w, W);
        }
        if (__any(any) && (tid & 63) == 0) s_any[level % 3] = 1;
        __syncthreads();                                        /* every read of F is done, next is complete */
        if (!s_any[level % 3]) break;                           /* (workgroup-uniform) nothing new: the field is complete */
        if (LDS) { uint64_t *t = F; F = NX; NX = t; }           /* next is the frontier now; the old frontier is written after this barrier only */
        else {
            for (int wd = tid; wd < nwords; wd += GIE_GNF1_THREADS) F[wd] = NX[wd];
            __syncthreads();
        }
    }
}

/* gie_ground_nf1_path: one lane per start point, a descent of nf1(s) steps */
__global__ __launch_bounds__(256) void k_gnf1_path(const gie_ctx c, const int32_t *f, const int pvt0, const int pvt1, const float *xy, const int n,
                                                   const int max_len, int32_t *path, int32_t *len)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int X = c.X, Y = c.Y, S[2] = { X, Y }, P[2] = { pvt0, pvt1 };
    int v[2] = { 0, 0 };
    bool in = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {                               /* (gie_ground_cell_of, written out: through the function the kernel's register count changes) */
        const float u = floorf(xy[2 * (size_t)p + k] / c.voxel_width + 0.5f);
        if (!(u >= -1.0e9f && u <= 1.0e9f)) { in = false; continue; }
        v[k] = (int)u - P[k];
        in &= v[k] >= 0 && v[k] < S[k];
    }
    int x = v[0], y = v[1], id = in ? y * X + x : 0;
    int cur = in ? f[id] : -1;
    len[p] = cur + 1;                                           /* (0 outside the field and where nf1 < 0) */
    if (cur < 0) return;
    int32_t *out = path + (size_t)p * max_len * 2;
    for (int i = 0; i < max_len; i++) {
        out[2 * i] = x + pvt0; out[2 * i + 1] = y + pvt1;
        if (cur == 0 || i + 1 == max_len) break;
        const int nb[4] = { x > 0 ? f[id - 1] : -1, x < X - 1 ? f[id + 1] : -1, y > 0 ? f[id - X] : -1, y < Y - 1 ? f[id + X] : -1 };
        const int want = cur - 1;
        if (nb[0] == want) { x--; id--; }
        else if (nb[1] == want) { x++; id++; }
        else if (nb[2] == want) { y--; id -= X; }
        else if (nb[3] == want) { y++; id += X; }
        else break;                                             /* (never in a complete field) */
        cur = want;
    }
}

/* gie_ground_nf1_query: one lane per point */
__global__ __launch_bounds__(256) void k_gnf1_query(const gie_ctx c, const int32_t *f, const int pvt0, const int pvt1, const float *xy, const int n, int32_t *steps)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int S[2] = { c.X, c.Y }, P[2] = { pvt0, pvt1 };
    int v[2] = { 0, 0 };
    bool in = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {                               /* (gie_ground_cell_of, written out: through the function the kernel's register count changes) */
        const float u = floorf(xy[2 * (size_t)p + k] / c.voxel_width + 0.5f);
        if (!(u >= -1.0e9f && u <= 1.0e9f)) { in = false; continue; }
        v[k] = (int)u - P[k];
        in &= v[k] >= 0 && v[k] < S[k];
    }
    steps[p] = in ? f[v[1] * c.X + v[0]] : -1;
}

/* the one-layer TYPE_NF1 CostMap payload; `o` from the ground field's type plane as it stands (no copy is kept) */
struct op_gnf1_costmap {
    const int32_t *f; const int8_t *type; gie_seendist *out;
    GIE_DEVM void operator()(const gie_ctx &, int i) const {
        const int v = f[i];
        gie_seendist sd; sd.d = v >= 0 ? (float)v : -1.0f; sd.s = 0;
        sd.o = (uint8_t)(type[i] != GIE_VOX_UNKNOWN); sd.pad[0] = sd.pad[1] = 0;
        out[i] = sd;
    }
};
struct op_gnf1_copy { const int32_t *f; int32_t *out; GIE_DEVM void operator()(const gie_ctx &, int i) const { out[i] = f[i]; } };

/* ---- host side */
static int gie_gnf1_check(gie_mapper *m, const char *who, bool need_field)
{
    static_assert(sizeof(gie_ground_nf1_param) == 32, "the size include/gie.h states");
    const int rc = gie_ground_check(m, who, true); if (rc) return rc;
    if (need_field && !m->gnf1.valid) { gie_set_err(std::string(who) + ": no ground navigation function of this ground field (gie_ground_nf1_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_gnf1_check_compute(gie_mapper *m, const char *who, const float *goal_xy, int n, const gie_ground_nf1_param *p)
{
    const int rc = gie_gnf1_check(m, who, false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->flags & ~(GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE | GIE_GROUND_NF1_FROM_FRONTIERS)) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3] || p->reserved[4] || p->reserved[5]) bad = "reserved must be 0";
    else if (n < 0 || (n > 0 && !goal_xy)) bad = "n < 0, or n > 0 without goals";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_gnf1_check_path(gie_mapper *m, const char *who, const float *start_xy, int n, int max_len, const int32_t *path_xy, const int32_t *len)
{
    const int rc = gie_gnf1_check(m, who, true); if (rc) return rc;
    if (n < 0 || max_len < 1 || (n > 0 && (!start_xy || !path_xy || !len))) { gie_set_err(std::string(who) + ": bad arguments"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static gie_gnf1_dev gie_gnf1_view(const gie_mapper *m)
{
    gie_gnf1_dev s;
    s.W = (m->c.X + 63) / 64;
    s.f = m->gnf1.f; s.blk = m->gnf1.bits; s.fr = s.blk + (size_t)s.W * m->c.Y; s.w = m->gnf1.words;
    return s;
}

extern "C" int gie_ground_nf1_compute_dev(gie_mapper *m, const float *d_goal_xy, int n, const gie_ground_nf1_param *p, int32_t *d_n_sources)
{
    const int rc = gie_gnf1_check_compute(m, "gie_ground_nf1_compute_dev", d_goal_xy, n, p); if (rc) return rc;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const int W = g.W, nwords = W * c.Y;
    const bool lds = nwords <= GIE_GNF1_LDS_WORDS;              /* by the size alone */
    static bool attr_done = false;
    const int ra = gie_ground_lds_limit(&attr_done, "gie_ground_nf1_compute_dev", reinterpret_cast<const void *>(&k_gnf1_bfs<true>),
                                        reinterpret_cast<const void *>(&k_gnf1_bfs<false>), GIE_GNF1_LDS_BYTES);
    if (ra) return ra;
    if (!m->gnf1.f) {
        int32_t *f = gie_dalloc<int32_t>(m, (size_t)c.X * c.Y, false);
        uint64_t *bits = f ? gie_dalloc<uint64_t>(m, 2 * (size_t)nwords, false) : nullptr;
        int32_t *words = bits ? gie_dalloc<int32_t>(m, GIE_GNF1_NWORDS, false) : nullptr;
        if (!words) { gie_set_err("gie_ground_nf1_compute_dev: device allocation of the ground navigation function failed"); return GIE_ERR_DEVICE; }
        m->gnf1.f = f; m->gnf1.bits = bits; m->gnf1.words = words;
    }
    const gie_gnf1_dev s = gie_gnf1_view(m);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_gnf1_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, g, s, nwords, (int)p->clearance_sq, (int)p->flags);
    if (n > 0) GIE_LAUNCH(&m->be, k_gnf1_goals, dim3((n + 255) / 256), dim3(256), 0, c, s, g.pvt[0], g.pvt[1], d_goal_xy, n);
    if (lds) GIE_LAUNCH(&m->be, k_gnf1_bfs<true>, dim3(1), dim3(GIE_GNF1_THREADS), 3 * (size_t)nwords * sizeof(uint64_t), c, s, nwords, d_n_sources);
    else GIE_LAUNCH(&m->be, k_gnf1_bfs<false>, dim3(1), dim3(GIE_GNF1_THREADS), (size_t)nwords * sizeof(uint64_t), c, s, nwords, d_n_sources);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    m->gnf1.valid = 1;
    return GIE_OK;
}
extern "C" int gie_ground_nf1_compute(gie_mapper *m, const float *goal_xy, int n, const gie_ground_nf1_param *p, int32_t *n_sources)
{
    int rc = gie_gnf1_check_compute(m, "gie_ground_nf1_compute", goal_xy, n, p); if (rc) return rc;
    float *dg = nullptr;
    if (n > 0) {
        dg = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_nf1_compute");
        if (!dg) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dg, goal_xy, (size_t)n * 8);
    }
    rc = gie_ground_nf1_compute_dev(m, dg, n, p, nullptr); if (rc) return rc;
    if (n_sources) be_d2h(&m->be, n_sources, m->gnf1.words + GIE_GNF1_W_SRC, sizeof(int32_t));
    return gie_sync(m);
}
extern "C" int gie_read_ground_nf1_dev(gie_mapper *m, int32_t *d_nf1)
{
    const int rc = gie_gnf1_check(m, "gie_read_ground_nf1_dev", true); if (rc) return rc;
    if (!d_nf1) { gie_set_err("gie_read_ground_nf1_dev: null output"); return GIE_ERR_INVALID; }
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    op_gnf1_copy op; op.f = m->gnf1.f; op.out = d_nf1;
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground_nf1(gie_mapper *m, int32_t *nf1)
{
    const int rc = gie_gnf1_check(m, "gie_read_ground_nf1", true); if (rc) return rc;
    if (nf1) be_d2h(&m->be, nf1, m->gnf1.f, (size_t)m->c.X * m->c.Y * 4);
    return gie_sync(m);
}
extern "C" int gie_ground_nf1_path_dev(gie_mapper *m, const float *d_start_xy, int n, int max_len, int32_t *d_path_xy, int32_t *d_len)
{
    const int rc = gie_gnf1_check_path(m, "gie_ground_nf1_path_dev", d_start_xy, n, max_len, d_path_xy, d_len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_gnf1_path, dim3((n + 255) / 256), dim3(256), 0, c, m->gnf1.f, m->ground.pvt[0], m->ground.pvt[1], d_start_xy, n, max_len, d_path_xy, d_len);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_ground_nf1_path(gie_mapper *m, const float *start_xy, int n, int max_len, int32_t *path_xy, int32_t *len)
{
    int rc = gie_gnf1_check_path(m, "gie_ground_nf1_path", start_xy, n, max_len, path_xy, len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    const size_t pbytes = (size_t)n * max_len * 8;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_nf1_path");
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 4 + pbytes, "gie_ground_nf1_path");      /* lengths, then the points */
    if (!dx || !dr) return GIE_ERR_DEVICE;
    /* only the points the descent writes reach the caller: the device buffer takes the caller's bytes first */
    be_h2d(&m->be, dx, start_xy, (size_t)n * 8);
    be_h2d(&m->be, dr + (size_t)n * 4, path_xy, pbytes);
    rc = gie_ground_nf1_path_dev(m, dx, n, max_len, (int32_t *)(dr + (size_t)n * 4), (int32_t *)dr); if (rc) return rc;
    be_d2h(&m->be, len, dr, (size_t)n * 4);
    be_d2h(&m->be, path_xy, dr + (size_t)n * 4, pbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}
static int gie_gnf1_check_query(gie_mapper *m, const char *who, const float *xy, int n, const int32_t *steps)
{
    const int rc = gie_gnf1_check(m, who, true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!xy || !steps))) { gie_set_err(std::string(who) + ": n < 0, or n > 0 with a null array"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_ground_nf1_query_dev(gie_mapper *m, const float *d_xy, int n, int32_t *d_steps)
{
    const int rc = gie_gnf1_check_query(m, "gie_ground_nf1_query_dev", d_xy, n, d_steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_gnf1_query, dim3((n + 255) / 256), dim3(256), 0, c, m->gnf1.f, m->ground.pvt[0], m->ground.pvt[1], d_xy, n, d_steps);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_ground_nf1_query(gie_mapper *m, const float *xy, int n, int32_t *steps)
{
    int rc = gie_gnf1_check_query(m, "gie_ground_nf1_query", xy, n, steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_nf1_query");
    int32_t *dr = (int32_t *)gie_scratch(m, 1, (size_t)n * 4, "gie_ground_nf1_query");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xy, (size_t)n * 8);
    rc = gie_ground_nf1_query_dev(m, dx, n, dr); if (rc) return rc;
    be_d2h(&m->be, steps, dr, (size_t)n * 4);
    gie_scratch_trim(m);
    return gie_sync(m);
}
static void gie_gnf1_costmap_hdr(const gie_mapper *m, gie_costmap_hdr *hdr)
{
    gie_ground_costmap_hdr(m, hdr);
    hdr->type = 2;
}
extern "C" int gie_read_costmap_ground_nf1_dev(gie_mapper *m, gie_seendist *d_payload, gie_costmap_hdr *hdr)
{
    const int rc = gie_gnf1_check(m, "gie_read_costmap_ground_nf1_dev", true); if (rc) return rc;
    if (!d_payload) { gie_set_err("gie_read_costmap_ground_nf1_dev: null payload"); return GIE_ERR_INVALID; }
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    op_gnf1_costmap op; op.f = m->gnf1.f; op.type = g.type; op.out = d_payload;
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    if (hdr) gie_gnf1_costmap_hdr(m, hdr);
    return GIE_OK;
}
extern "C" int gie_read_costmap_ground_nf1(gie_mapper *m, gie_seendist *payload, gie_costmap_hdr *hdr)
{
    int rc = gie_gnf1_check(m, "gie_read_costmap_ground_nf1", true); if (rc) return rc;
    if (payload) {
        const size_t n = (size_t)m->c.X * m->c.Y;
        gie_seendist *d = (gie_seendist *)gie_scratch(m, 1, n * sizeof(gie_seendist), "gie_read_costmap_ground_nf1");
        if (!d) return GIE_ERR_DEVICE;
        rc = gie_read_costmap_ground_nf1_dev(m, d, nullptr); if (rc) return rc;
        be_d2h(&m->be, payload, d, n * sizeof(gie_seendist));
    }
    if (hdr) gie_gnf1_costmap_hdr(m, hdr);
    return gie_sync(m);
}

/*
 * gie_ground_pose_nf1.inc.h — the NF1 navigation function of the (cell, heading) configuration space of an oriented rectangle on
 * the ground costmap, and its descent paths (include/gie.h "ground pose navigation function").
 * HIP backend only: included by gie_hip.hip after gie_ground_footprint.inc.h.  It reads the ground field's type and dist_sq planes
 * and writes nothing of the map, of that field or of the ground navigation function; its own planes are allocated at the first
 * compute.  A bit plane here has EIGHT layers of nwords = W * Y words, layer k at k * nwords, in glos_blk's word layout.
 *   k_glos_prep      unchanged (gie_glos_prepare): the blocked plane of clearance_sq and the UNKNOWN flag.
 *   k_gpose_cspace   the obstruction planes C, BIT-PARALLEL: a workgroup serves one heading k; its first 2R + 1 threads solve the
 *                    footprint predicate for the row intervals [x0, x1](dy) of d_k (gie_gfp_isqrt / gie_gfp_clip, the footprint
 *                    kernel's own two clips) into LDS, once per workgroup.  Then a lane per output word: for every row dy with an
 *                    interval it loads the five words of blk's row y + dy from word w + floor(x0 / 64) on, ORs the window with
 *                    itself shifted by 1, 2, 4 .. (shift doubling, the last step cut to the interval's length: at most eight steps
 *                    for 181 cells), and takes the 64 bits at x0 mod 64: bit x of the result is the OR of blk over x + x0 .. x + x1.
 *                    Words and rows outside the rectangle, and blk's padding bits beyond X, are all-ones without the UNKNOWN flag
 *                    and all-zeros with it.  C's own padding bits beyond X are SET.
 *   k_gpose_prep     a wave per 64-cell word and layer (k_gnf1_prep's ballot form): the field at -1, the FNT sources at 0, the
 *                    working plane B = C | sources ("blocked or visited") and the level-0 frontier.
 *   k_gpose_goals    one lane per goal (k_gnf1_goals' form): one atomic OR on B per heading decides whether a state becomes a source.
 *   k_gpose_bfs      ONE workgroup of 1024 threads, one workgroup barrier per level, at most 8 * X * Y levels.  A thread owns the
 *                    words tid + 1024 j of ALL eight layers: the eight frontier words are in registers, so the two turns of layer k
 *                    are F[k + 1] | F[k - 1] without a load.  The field is built from the sources over PREDECESSORS: a state gets
 *                    level L + 1 when one of its moves leads into the frontier of level L —
 *                      next_k = (F_k[row y + sy] moved by -sx | with REVERSE F_k[row y - sy] moved by +sx | F_{k+1} | F_{k-1}) & ~B_k
 *                    with the carry bit of the neighbouring word and nothing from beyond the rows 0 .. Y - 1.  LDS = true: next, F
 *                    and B in dynamic LDS (three planes of eight layers: 192 bytes per word, nwords <= 768), next and F swapped
 *                    behind the barrier.  LDS = false: the same loop on the planes where they lie in global memory, the two
 *                    frontier planes swapped by pointer behind the barrier (a level only reads the plane the last level wrote and
 *                    writes the one the last level read: one barrier is enough).  The host picks the form by the size alone.  No
 *                    grid barrier, no cooperative launch, no timeout path, no spin-wait.
 *   k_gpose_path / k_gpose_query   one lane per start / point.    k_gpose_bytes   one lane per cell: the C-space byte.
 * The compiler's figures and the times are in DESIGN.md 27.
 */

#define GIE_GPOSE_LDS_WORDS (GIE_GNF1_LDS_BYTES / (24 * GIE_GROUND_POSE_HEADINGS))      /* words of ONE layer when three 8-layer planes fit: 768 */
#define GIE_GPOSE_ROWS 181                                      /* 2 R + 1 with R <= 90 */
enum { GIE_GPOSE_W_SRC = 0,     /* the distinct source states */
       GIE_GPOSE_W_FREE = 1,    /* the free states */
       GIE_GPOSE_NWORDS = 4 };

struct gie_gpose_dev {
    int32_t *f;                 /* 8 * X * Y: the field, k slowest */
    uint64_t *C, *B, *F0, *F1;  /* 8 * nwords each: not free; blocked or visited; the two frontier planes */
    int32_t *w;                 /* control words */
    int W, nwords;
};

GIE_DEV void gie_gpose_dir(const int k, int &sx, int &sy)
{
    sx = (k == 0 || k == 1 || k == 7) ? 1 : ((k >= 3 && k <= 5) ? -1 : 0);
    sy = (k >= 1 && k <= 3) ? 1 : (k >= 5 ? -1 : 0);
}

/* bits [s, s + 64) of the pair (lo, hi), 0 <= s <= 64 */
GIE_DEV uint64_t gie_gpose_shr(const uint64_t lo, const uint64_t hi, const int s)
{
    return s == 0 ? lo : (s == 64 ? hi : ((lo >> s) | (hi << (64 - s))));
}

struct gie_gpose_arg { int front_sq, back_sq, side_sq, R, unknown_ok; };

__global__ __launch_bounds__(256) void k_gpose_cspace(const gie_glos_dev s, const gie_gpose_arg a, const int nwords, uint64_t *C)
{
    __shared__ int s_x0[GIE_GPOSE_ROWS], s_x1[GIE_GPOSE_ROWS];
    const int k = blockIdx.y, tid = threadIdx.x;
    int hx, hy;
    gie_gpose_dir(k, hx, hy);
    if (tid < 2 * a.R + 1) {                                    /* the row intervals of heading d_k: once per workgroup */
        const int dy = tid - a.R;
        const long long n2 = (long long)(hx * hx + hy * hy);
        const int ah = gie_gfp_isqrt(a.front_sq * n2), al = gie_gfp_isqrt(a.back_sq * n2), bm = gie_gfp_isqrt(a.side_sq * n2);
        int x0 = -a.R, x1 = a.R;
        gie_gfp_clip(hx, dy * hy, -al, ah, x0, x1);             /* -al <= a = dx hx + dy hy <= ah */
        gie_gfp_clip(hy, -dy * hx, -bm, bm, x0, x1);            /* -bm <= b = dx hy - dy hx <= bm */
        s_x0[tid] = x0; s_x1[tid] = x1;
    }
    __syncthreads();
    const int wd = blockIdx.x * 256 + tid;
    if (wd >= nwords) return;
    const int y = wd / s.W, tx = wd - y * s.W;
    const uint64_t fill = a.unknown_ok ? 0ull : ~0ull;          /* what lies outside the rectangle */
    const uint64_t last = (s.X & 63) ? ((1ull << (s.X & 63)) - 1ull) : ~0ull;      /* the cells of a row's last word */
    uint64_t acc = 0;
#pragma unroll 1
    for (int r = 0; r <= 2 * a.R; r++) {
        const int x0 = s_x0[r], x1 = s_x1[r];
        if (x0 > x1) continue;                                  /* (workgroup-uniform) */
        const int yy = y + r - a.R, len = x1 - x0 + 1;
        const int q = x0 >> 6, sh = x0 & 63;                    /* x0 = 64 q + sh, floor division */
        uint64_t S[6];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int wi = tx + q + i;
            uint64_t v = fill;
            if (yy >= 0 && yy < s.Y && wi >= 0 && wi < s.W) {
                v = s.blk[(size_t)yy * s.W + wi];
                if (wi == s.W - 1) v = (v & last) | (fill & ~last);       /* blk's padding bits are no cells */
            }
            S[i] = v;
        }
        S[5] = 0;
        /* S[i] := OR of the window's bits i .. i + have - 1; bits up to sh + 63 + len - 1 <= 306 are needed, 320 are held */
#pragma unroll 1
        for (int have = 1; have < len;) {                       /* (workgroup-uniform) */
            const int step = have < len - have ? have : len - have;       /* <= 64 */
#pragma unroll
            for (int i = 0; i < 5; i++) S[i] |= gie_gpose_shr(S[i], S[i + 1], step);
            have += step;
        }
        acc |= gie_gpose_shr(S[0], S[1], sh);
    }
    if (tx == s.W - 1) acc |= ~last;                            /* C's padding bits beyond X are SET */
    C[(size_t)k * nwords + wd] = acc;
}

/* prep (a): the field at -1, the FNT sources at 0, B and the level-0 frontier; a wave per word and layer */
__global__ __launch_bounds__(256) void k_gpose_prep(const gie_ctx c, const gie_ground_dev g, const gie_gpose_dev s, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const int y = wd / s.W, x = (wd - y * s.W) * 64 + lane;
    const uint64_t cw = s.C[(size_t)k * s.nwords + wd];
    bool src = false;
    if (x < c.X) {
        src = (flags & GIE_GROUND_POSE_NF1_FROM_FRONTIERS) && g.type[y * c.X + x] == GIE_VOX_FNT && !((cw >> lane) & 1ull);
        s.f[((size_t)k * c.Y + y) * c.X + x] = src ? 0 : -1;
    }
    const uint64_t bs = __ballot(src);
    if (lane == 0) { s.B[(size_t)k * s.nwords + wd] = cw | bs; s.F0[(size_t)k * s.nwords + wd] = bs; }
}

/* prep (b): one lane per goal; gie_ground_query's mapping of a point to its cell; its free states of goal_k join the sources */
__global__ __launch_bounds__(256) void k_gpose_goals(const gie_ctx c, const gie_gpose_dev s, const int pvt0, const int pvt1, const float *xy, const int32_t *gk,
                                                     const int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int P[2] = { pvt0, pvt1 };
    int v[2];
    if (!gie_ground_cell_of(c.voxel_width, c.X, c.Y, P, xy + 2 * (size_t)p, v)) return;
    const int want = gk ? gk[p] : -1;
    if (want < -1 || want >= GIE_GROUND_POSE_HEADINGS) return;
    const int wd = v[1] * s.W + (v[0] >> 6);
    const unsigned long long bit = 1ull << (v[0] & 63);
    for (int k = 0; k < GIE_GROUND_POSE_HEADINGS; k++) {
        if (want >= 0 && k != want) continue;
        const size_t at = (size_t)k * s.nwords + wd;
        if (atomicOr((unsigned long long *)&s.B[at], bit) & bit) continue;      /* not free, or a source already */
        atomicOr((unsigned long long *)&s.F0[at], bit);
        s.f[((size_t)k * c.Y + v[1]) * c.X + v[0]] = 0;
    }
}

/* bit x of the result = bit x + SX of layer row `row` (word column tx): the word moved by -SX with the neighbour's carry */
template <int SX>
GIE_DEV uint64_t gie_gpose_moved(const uint64_t *row, const int tx, const int W)
{
    const uint64_t m = row[tx];
    if (SX == 0) return m;
    if (SX > 0) return (m >> 1) | (tx < W - 1 ? row[tx + 1] << 63 : 0ull);
    return (m << 1) | (tx > 0 ? row[tx - 1] >> 63 : 0ull);
}

/* the states whose F move (and, REV, whose B move) leads into layer K's frontier */
template <int K>
GIE_DEV uint64_t gie_gpose_straight(const uint64_t *F, const bool REV, const int nwords, const int y, const int tx, const int W, const int Y)
{
    constexpr int SX = (K == 0 || K == 1 || K == 7) ? 1 : ((K >= 3 && K <= 5) ? -1 : 0);
    constexpr int SY = (K >= 1 && K <= 3) ? 1 : (K >= 5 ? -1 : 0);
    const uint64_t *L = F + (size_t)K * nwords;
    uint64_t d = 0;
    const int yf = y + SY, yb = y - SY;
    if (yf >= 0 && yf < Y) d |= gie_gpose_moved<SX>(L + (size_t)yf * W, tx, W);
    if (REV && yb >= 0 && yb < Y) d |= gie_gpose_moved<-SX>(L + (size_t)yb * W, tx, W);
    return d;
}

template <bool LDS>
__global__ __launch_bounds__(GIE_GNF1_THREADS) void k_gpose_bfs(const gie_ctx c, const gie_gpose_dev s, const int reverse, int32_t *counts)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_planes[];     /* LDS form: next, the frontier and B, eight layers each */
    __shared__ int s_cnt[2][GIE_GNF1_THREADS / 64], s_any[3];  /* s_any[L % 3]: some wave found a new bit in level L */
    const int tid = threadIdx.x, W = s.W, X = c.X, Y = c.Y, nwords = s.nwords, all = GIE_GROUND_POSE_HEADINGS * nwords;
    uint64_t *NX = LDS ? s_planes : s.F1, *F = LDS ? s_planes + all : s.F0, *B = LDS ? s_planes + 2 * (size_t)all : s.B;
    const bool REV = reverse != 0;                              /* (workgroup-uniform) */
    int n = 0, nfree = 0;
    for (int i = tid; i < all; i += GIE_GNF1_THREADS) {        /* the sources and the free states counted, the planes into LDS */
        const uint64_t f = s.F0[i];
        n += __popcll(f);
        nfree += __popcll(~s.C[i]);
        if (LDS) { F[i] = f; B[i] = s.B[i]; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { n += __shfl_xor(n, d); nfree += __shfl_xor(nfree, d); }
    if ((tid & 63) == 0) { s_cnt[0][tid >> 6] = n; s_cnt[1][tid >> 6] = nfree; }
    if (tid == 0) s_any[0] = s_any[1] = s_any[2] = 0;
    __syncthreads();
    if (tid == 0) {
        int t = 0, u = 0;
        for (int i = 0; i < GIE_GNF1_THREADS / 64; i++) { t += s_cnt[0][i]; u += s_cnt[1][i]; }
        s.w[GIE_GPOSE_W_SRC] = t; s.w[GIE_GPOSE_W_FREE] = u;
        if (counts) { counts[0] = t; counts[1] = u; }
    }
    /* (gie_ground_words, written out: with it both forms measured above the parent's range, profiles/r28_ground_helpers_times.txt) */
    const int y0 = tid / W, tx0 = tid - y0 * W, dy = GIE_GNF1_THREADS / W, dtx = GIE_GNF1_THREADS - dy * W;
    const long long max_levels = (long long)GIE_GROUND_POSE_HEADINGS * X * Y;      /* no route is longer: the loop ends here whatever the planes hold */
#pragma unroll 1
    for (int level = 0; level < max_levels; level++) {
        if (tid == 0) s_any[(level + 1) % 3] = 0;               /* (last read after the barrier of level - 2, next set in level + 1) */
        int any = 0;
#pragma unroll 1
        for (int wd = tid, y = y0, tx = tx0; wd < nwords; wd += GIE_GNF1_THREADS) {
            uint64_t cur[8], d[8];
#pragma unroll
            for (int k = 0; k < 8; k++) cur[k] = F[(size_t)k * nwords + wd];
            d[0] = gie_gpose_straight<0>(F, REV, nwords, y, tx, W, Y);
            d[1] = gie_gpose_straight<1>(F, REV, nwords, y, tx, W, Y);
            d[2] = gie_gpose_straight<2>(F, REV, nwords, y, tx, W, Y);
            d[3] = gie_gpose_straight<3>(F, REV, nwords, y, tx, W, Y);
            d[4] = gie_gpose_straight<4>(F, REV, nwords, y, tx, W, Y);
            d[5] = gie_gpose_straight<5>(F, REV, nwords, y, tx, W, Y);
            d[6] = gie_gpose_straight<6>(F, REV, nwords, y, tx, W, Y);
            d[7] = gie_gpose_straight<7>(F, REV, nwords, y, tx, W, Y);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const size_t at = (size_t)k * nwords + wd;
                const uint64_t bl = B[at], nx = (d[k] | cur[(k + 1) & 7] | cur[(k + 7) & 7]) & ~bl;      /* (B holds the padding bits; only its owner touches a word of it) */
                NX[at] = nx;
                if (nx) {
                    any = 1;
                    B[at] = bl | nx;
                    int32_t *fr = s.f + ((size_t)k * Y + y) * X + tx * 64;
                    for (uint64_t b = nx; b; b &= b - 1) fr[__builtin_ctzll(b)] = level + 1;
                }
            }
            y += dy; tx += dtx;
            if (tx >= W) { tx -= W; y++; }
        }
        if (__any(any) && (tid & 63) == 0) s_any[level % 3] = 1;
        __syncthreads();                                        /* every read of F is done, next is complete */
        if (!s_any[level % 3]) break;                           /* (workgroup-uniform) nothing new: the field is complete */
        { uint64_t *t = F; F = NX; NX = t; }                    /* next is the frontier now; the old frontier is written after this barrier only */
    }
}

/* the cell of point p and the field's value there; k == -1: the lowest heading with the least value >= 0 */
GIE_DEV int gie_gpose_lookup(const gie_ctx &c, const int32_t *f, const int pvt0, const int pvt1, const float *xy, int k, int v[2], int &kk)
{
    const int P[2] = { pvt0, pvt1 };
    const bool in = gie_ground_cell_of(c.voxel_width, c.X, c.Y, P, xy, v);
    kk = 0;
    if (!in || k < -1 || k >= GIE_GROUND_POSE_HEADINGS) return -1;
    const size_t plane = (size_t)c.X * c.Y, id = (size_t)v[1] * c.X + v[0];
    if (k >= 0) { kk = k; return f[k * plane + id]; }
    int best = -1;
    for (int j = 0; j < GIE_GROUND_POSE_HEADINGS; j++) {
        const int val = f[j * plane + id];
        if (val >= 0 && (best < 0 || val < best)) { best = val; kk = j; }
    }
    return best;
}

__global__ __launch_bounds__(256) void k_gpose_query(const gie_ctx c, const int32_t *f, const int pvt0, const int pvt1, const float *xy, const int32_t *k,
                                                     const int n, int32_t *steps)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[2], kk;
    steps[p] = gie_gpose_lookup(c, f, pvt0, pvt1, xy + 2 * (size_t)p, k ? k[p] : -1, v, kk);
}

/* gie_ground_pose_nf1_path: one lane per start, a descent of pnf1(start) moves; the first of F, B, L, R one step closer */
__global__ __launch_bounds__(256) void k_gpose_path(const gie_ctx c, const int32_t *f, const int pvt0, const int pvt1, const float *xy, const int32_t *sk,
                                                    const int n, const int max_len, const int reverse, int32_t *path, int32_t *len)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int X = c.X, Y = c.Y;
    const size_t plane = (size_t)X * Y;
    int v[2], k;
    int cur = gie_gpose_lookup(c, f, pvt0, pvt1, xy + 2 * (size_t)p, sk ? sk[p] : -1, v, k);
    len[p] = cur + 1;                                           /* (0 without a cell, with a k outside -1..7 and where pnf1 < 0) */
    if (cur < 0) return;
    int x = v[0], y = v[1];
    int32_t *out = path + (size_t)p * max_len * 3;
    for (int i = 0; i < max_len; i++) {
        out[3 * i] = x + pvt0; out[3 * i + 1] = y + pvt1; out[3 * i + 2] = k;
        if (cur == 0 || i + 1 == max_len) break;
        int sx, sy;
        gie_gpose_dir(k, sx, sy);
        const int want = cur - 1, fx = x + sx, fy = y + sy, bx = x - sx, by = y - sy, kl = (k + 1) & 7, kr = (k + 7) & 7;
        if (fx >= 0 && fx < X && fy >= 0 && fy < Y && f[k * plane + (size_t)fy * X + fx] == want) { x = fx; y = fy; }
        else if (reverse && bx >= 0 && bx < X && by >= 0 && by < Y && f[k * plane + (size_t)by * X + bx] == want) { x = bx; y = by; }
        else if (f[kl * plane + (size_t)y * X + x] == want) k = kl;
        else if (f[kr * plane + (size_t)y * X + x] == want) k = kr;
        else break;                                             /* (never in a complete field) */
        cur = want;
    }
}

/* the C-space byte of a cell: bit k set iff (c, k) is not free */
struct op_gpose_bytes {
    const uint64_t *C; uint8_t *out; int W, nwords;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int y = i / c.X, x = i - y * c.X;
        const size_t wd = (size_t)y * W + (x >> 6);
        unsigned b = 0;
        for (int k = 0; k < GIE_GROUND_POSE_HEADINGS; k++) b |= (unsigned)((C[(size_t)k * nwords + wd] >> (x & 63)) & 1ull) << k;
        out[i] = (uint8_t)b;
    }
};

/* ---- host side */
static int gie_gpose_check(gie_mapper *m, const char *who, bool need_field)
{
    static_assert(sizeof(gie_ground_pose_nf1_param) == 32, "the size include/gie.h states");
    static_assert(GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE == GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE && GIE_GROUND_POSE_HEADINGS == 8 &&
                  GIE_GROUND_POSE_MAX_SQ == (1 << 12) && GIE_GPOSE_LDS_WORDS == 768, "k_glos_prep's flag; eight layers; R <= 90: 181 rows of at most 181 cells");
    const int rc = gie_glos_check(m, who); if (rc) return rc;
    if (need_field && !m->gpose.valid) {
        gie_set_err(std::string(who) + ": no ground pose navigation function of this ground field (gie_ground_pose_nf1_compute first)");
        return GIE_ERR_INVALID;
    }
    return GIE_OK;
}
static int gie_gpose_check_compute(gie_mapper *m, const char *who, const float *goal_xy, int n, const gie_ground_pose_nf1_param *p)
{
    const int rc = gie_gpose_check(m, who, false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->front_sq < 0 || p->front_sq > GIE_GROUND_POSE_MAX_SQ || p->back_sq < 0 || p->back_sq > GIE_GROUND_POSE_MAX_SQ ||
             p->side_sq < 0 || p->side_sq > GIE_GROUND_POSE_MAX_SQ) bad = "front_sq, back_sq and side_sq must be in 0 .. 1 << 12";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->flags & ~(GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE | GIE_GROUND_POSE_NF1_FROM_FRONTIERS | GIE_GROUND_POSE_NF1_REVERSE)) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2]) bad = "reserved must be 0";
    else if (n < 0 || (n > 0 && !goal_xy)) bad = "n < 0, or n > 0 without goals";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_gpose_check_points(gie_mapper *m, const char *who, const float *xy, int n, int max_len, const void *out0, const void *out1)
{
    const int rc = gie_gpose_check(m, who, true); if (rc) return rc;
    if (n < 0 || max_len < 1 || (n > 0 && (!xy || !out0 || !out1))) { gie_set_err(std::string(who) + ": bad arguments"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static gie_gpose_dev gie_gpose_view(const gie_mapper *m)
{
    gie_gpose_dev s;
    s.W = (m->c.X + 63) / 64; s.nwords = s.W * m->c.Y;
    const size_t all = (size_t)GIE_GROUND_POSE_HEADINGS * s.nwords;
    s.f = m->gpose.f; s.C = m->gpose.bits; s.B = s.C + all; s.F0 = s.B + all; s.F1 = s.F0 + all; s.w = m->gpose.words;
    return s;
}

extern "C" int gie_ground_pose_nf1_compute_dev(gie_mapper *m, const float *d_goal_xy, const int32_t *d_goal_k, int n, const gie_ground_pose_nf1_param *p,
                                               int32_t *d_counts)
{
    const char *who = "gie_ground_pose_nf1_compute_dev";
    const int rc = gie_gpose_check_compute(m, who, d_goal_xy, n, p); if (rc) return rc;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const int W = g.W, nwords = W * c.Y;
    const bool lds = nwords <= GIE_GPOSE_LDS_WORDS;             /* by the size alone */
    static bool attr_done = false;
    const int ra = gie_ground_lds_limit(&attr_done, who, reinterpret_cast<const void *>(&k_gpose_bfs<true>), nullptr, GIE_GNF1_LDS_BYTES);
    if (ra) return ra;
    if (!m->gpose.f) {
        int32_t *f = gie_dalloc<int32_t>(m, (size_t)GIE_GROUND_POSE_HEADINGS * c.X * c.Y, false);
        uint64_t *bits = f ? gie_dalloc<uint64_t>(m, 4 * (size_t)GIE_GROUND_POSE_HEADINGS * nwords, false) : nullptr;
        int32_t *words = bits ? gie_dalloc<int32_t>(m, GIE_GPOSE_NWORDS, false) : nullptr;
        if (!words) { gie_set_err(std::string(who) + ": device allocation of the ground pose navigation function failed"); return GIE_ERR_DEVICE; }
        m->gpose.f = f; m->gpose.bits = bits; m->gpose.words = words;
    }
    const gie_gpose_dev s = gie_gpose_view(m);
    gie_gpose_arg a;
    a.front_sq = (int)p->front_sq; a.back_sq = (int)p->back_sq; a.side_sq = (int)p->side_sq;
    a.unknown_ok = (p->flags & GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE) != 0;
    const int q = std::max(a.front_sq, a.back_sq) + a.side_sq;
    int R = (int)std::sqrt((double)q);
    while (R * R > q) R--;
    while ((R + 1) * (R + 1) <= q) R++;
    a.R = R;                                                    /* <= 90 */
    const bool rev = (p->flags & GIE_GROUND_POSE_NF1_REVERSE) != 0;
    gie_glos_dev gl;
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    const bool ok = gie_glos_prepare(m, who, c, g, (int)p->clearance_sq, (int)p->flags & GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE, &gl);
    if (ok) {
        const size_t lds_bytes = 3 * (size_t)GIE_GROUND_POSE_HEADINGS * nwords * sizeof(uint64_t);
        GIE_LAUNCH(&m->be, k_gpose_cspace, dim3((nwords + 255) / 256, GIE_GROUND_POSE_HEADINGS), dim3(256), 0, gl, a, nwords, s.C);
        GIE_LAUNCH(&m->be, k_gpose_prep, dim3((nwords + 3) / 4, GIE_GROUND_POSE_HEADINGS), dim3(256), 0, c, g, s, (int)p->flags);
        if (n > 0) GIE_LAUNCH(&m->be, k_gpose_goals, dim3((n + 255) / 256), dim3(256), 0, c, s, g.pvt[0], g.pvt[1], d_goal_xy, d_goal_k, n);
        if (lds) GIE_LAUNCH(&m->be, k_gpose_bfs<true>, dim3(1), dim3(GIE_GNF1_THREADS), lds_bytes, c, s, (int)rev, d_counts);
        else GIE_LAUNCH(&m->be, k_gpose_bfs<false>, dim3(1), dim3(GIE_GNF1_THREADS), 0, c, s, (int)rev, d_counts);
    }
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    if (!ok) return GIE_ERR_DEVICE;
    m->gpose.valid = 1; m->gpose.reverse = rev;
    return GIE_OK;
}
extern "C" int gie_ground_pose_nf1_compute(gie_mapper *m, const float *goal_xy, const int32_t *goal_k, int n, const gie_ground_pose_nf1_param *p, int32_t *counts)
{
    int rc = gie_gpose_check_compute(m, "gie_ground_pose_nf1_compute", goal_xy, n, p); if (rc) return rc;
    char *dg = nullptr;
    if (n > 0) {
        dg = (char *)gie_scratch(m, 0, (size_t)n * 12, "gie_ground_pose_nf1_compute");      /* the goals, then their headings */
        if (!dg) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dg, goal_xy, (size_t)n * 8);
        if (goal_k) be_h2d(&m->be, dg + (size_t)n * 8, goal_k, (size_t)n * 4);
    }
    rc = gie_ground_pose_nf1_compute_dev(m, (const float *)dg, goal_k && n > 0 ? (const int32_t *)(dg + (size_t)n * 8) : nullptr, n, p, nullptr);
    if (rc) return rc;
    if (counts) be_d2h(&m->be, counts, m->gpose.words + GIE_GPOSE_W_SRC, 2 * sizeof(int32_t));
    return gie_sync(m);
}
static int gie_gpose_check_read(gie_mapper *m, const char *who, const void *pnf1, const void *cspace)
{
    const int rc = gie_gpose_check(m, who, true); if (rc) return rc;
    if (!pnf1 && !cspace) { gie_set_err(std::string(who) + ": nothing to write: both outputs null"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_read_ground_pose_nf1_dev(gie_mapper *m, int32_t *d_pnf1, uint8_t *d_cspace)
{
    const int rc = gie_gpose_check_read(m, "gie_read_ground_pose_nf1_dev", d_pnf1, d_cspace); if (rc) return rc;
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    const gie_gpose_dev s = gie_gpose_view(m);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    if (d_pnf1) { op_gnf1_copy op; op.f = s.f; op.out = d_pnf1; be_lin(&m->be, c, op, GIE_GROUND_POSE_HEADINGS * c.X * c.Y); }
    if (d_cspace) { op_gpose_bytes op; op.C = s.C; op.out = d_cspace; op.W = s.W; op.nwords = s.nwords; be_lin(&m->be, c, op, c.X * c.Y); }
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground_pose_nf1(gie_mapper *m, int32_t *pnf1, uint8_t *cspace)
{
    int rc = gie_gpose_check_read(m, "gie_read_ground_pose_nf1", pnf1, cspace); if (rc) return rc;
    const size_t cells = (size_t)m->c.X * m->c.Y;
    if (cspace) {
        uint8_t *d = (uint8_t *)gie_scratch(m, 1, cells, "gie_read_ground_pose_nf1");
        if (!d) return GIE_ERR_DEVICE;
        rc = gie_read_ground_pose_nf1_dev(m, nullptr, d); if (rc) return rc;
        be_d2h(&m->be, cspace, d, cells);
    } else { be_prof(&m->be, GIE_K_GROUND_NF1, 0); be_prof(&m->be, GIE_K_GROUND_NF1, 1); }      /* (a copy alone launches nothing: still one entry per call) */
    if (pnf1) be_d2h(&m->be, pnf1, m->gpose.f, GIE_GROUND_POSE_HEADINGS * cells * 4);
    return gie_sync(m);
}
extern "C" int gie_ground_pose_nf1_query_dev(gie_mapper *m, const float *d_xy, const int32_t *d_k, int n, int32_t *d_steps)
{
    const int rc = gie_gpose_check_points(m, "gie_ground_pose_nf1_query_dev", d_xy, n, 1, d_steps, d_steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_gpose_query, dim3((n + 255) / 256), dim3(256), 0, c, m->gpose.f, m->ground.pvt[0], m->ground.pvt[1], d_xy, d_k, n, d_steps);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_ground_pose_nf1_query(gie_mapper *m, const float *xy, const int32_t *k, int n, int32_t *steps)
{
    int rc = gie_gpose_check_points(m, "gie_ground_pose_nf1_query", xy, n, 1, steps, steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    char *dx = (char *)gie_scratch(m, 0, (size_t)n * 12, "gie_ground_pose_nf1_query");          /* the points, then their headings */
    int32_t *dr = (int32_t *)gie_scratch(m, 1, (size_t)n * 4, "gie_ground_pose_nf1_query");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xy, (size_t)n * 8);
    if (k) be_h2d(&m->be, dx + (size_t)n * 8, k, (size_t)n * 4);
    rc = gie_ground_pose_nf1_query_dev(m, (const float *)dx, k ? (const int32_t *)(dx + (size_t)n * 8) : nullptr, n, dr); if (rc) return rc;
    be_d2h(&m->be, steps, dr, (size_t)n * 4);
    return gie_sync(m);
}
extern "C" int gie_ground_pose_nf1_path_dev(gie_mapper *m, const float *d_start_xy, const int32_t *d_start_k, int n, int max_len, int32_t *d_path_xyk, int32_t *d_len)
{
    const int rc = gie_gpose_check_points(m, "gie_ground_pose_nf1_path_dev", d_start_xy, n, max_len, d_path_xyk, d_len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_gpose_path, dim3((n + 255) / 256), dim3(256), 0, c, m->gpose.f, m->ground.pvt[0], m->ground.pvt[1], d_start_xy, d_start_k, n, max_len,
               m->gpose.reverse, d_path_xyk, d_len);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_ground_pose_nf1_path(gie_mapper *m, const float *start_xy, const int32_t *start_k, int n, int max_len, int32_t *path_xyk, int32_t *len)
{
    int rc = gie_gpose_check_points(m, "gie_ground_pose_nf1_path", start_xy, n, max_len, path_xyk, len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    if ((size_t)n > SIZE_MAX / 16 / (size_t)max_len) { gie_set_err("gie_ground_pose_nf1_path: n * max_len * 12 bytes exceed size_t"); return GIE_ERR_INVALID; }
    const size_t pbytes = (size_t)n * max_len * 12;
    char *dx = (char *)gie_scratch(m, 0, (size_t)n * 12, "gie_ground_pose_nf1_path");            /* the starts, then their headings */
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 4 + pbytes, "gie_ground_pose_nf1_path");    /* lengths, then the triples */
    if (!dx || !dr) return GIE_ERR_DEVICE;
    /* only the triples the descent writes reach the caller: the device buffer takes the caller's bytes first */
    be_h2d(&m->be, dx, start_xy, (size_t)n * 8);
    if (start_k) be_h2d(&m->be, dx + (size_t)n * 8, start_k, (size_t)n * 4);
    be_h2d(&m->be, dr + (size_t)n * 4, path_xyk, pbytes);
    rc = gie_ground_pose_nf1_path_dev(m, (const float *)dx, start_k ? (const int32_t *)(dx + (size_t)n * 8) : nullptr, n, max_len, (int32_t *)(dr + (size_t)n * 4),
                                      (int32_t *)dr);
    if (rc) return rc;
    be_d2h(&m->be, len, dr, (size_t)n * 4);
    be_d2h(&m->be, path_xyk, dr + (size_t)n * 4, pbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}

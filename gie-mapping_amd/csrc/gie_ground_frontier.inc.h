/*
 * gie_ground_frontier.inc.h — ground frontier clusters: the connected components of the ground field's FNT cells, filtered by size,
 * with a record (size, box, centroid, representative cell and its dist_sq) per kept component (include/gie.h "ground frontier
 * clusters"; the gather of the ground navigation function at their goals, gie_ground_nf1_query, is in gie_ground_nf1.inc.h).
 * HIP backend only: included by gie_hip.hip after gie_ground_los.inc.h.  It reads the ground field's type and dist_sq planes and
 * writes nothing of the map or of that field.
 *
 * The cache (gie_mapper::gfr), per CELL, allocated at the first compute:
 *   par    int32 per cell, written at members only: the union-find forest.  A member that is not the first cell of its x-run
 *          inside its 64-bit word (the run's HEAD) points at that head for good; find and unite only ever see heads, and after
 *          k_gfr_tile<0> a head points at its root: label(c) = par[par[c]];
 *   size   int32 per cell, written at members only, read at roots: the component's size;
 *   mem    one bit per cell, member: rows of W = ceil(X/64) 64-bit words, bit x & 63 of word x >> 6; the padding bits beyond X are
 *          CLEAR (the opposite of ground NF1's blk: a set one would join the two rows behind a wall);
 *   kept   same layout: the roots of the kept components;
 *   cnt    int32 per word: popcount of kept; rank: its exclusive scan (the rank of a word's first kept root);
 *   w      GIE_GFR_NWORDS control words (the two counts);
 *   rec    max_clusters records (grows with the largest max_clusters asked for).
 * A compute is a fixed sequence of launches, none of them a loop of the host's and none with a grid barrier (gie_frontier.inc.h's
 * algorithm on one layer, with other statistics kernels):
 *   k_gfr_prep     a lane per cell, a wave per word (k_gnf1_prep's form, 5 bytes per cell): the member plane; par = the head, size = 0;
 *   k_gfr_merge    a lane per word: every run of the word is united with the runs it touches in row y - 1 (at connectivity 8 the
 *                  run dilated by one bit, with the edge bits of the words beside that one) and with the word before it;
 *                  gie_fr_unite: a compare-and-swap hangs the larger root below the smaller, so the final root is the
 *                  component's smallest index whatever the schedule;
 *   k_gfr_tile<0>  heads get their root; sizes;
 *   k_gfr_kept     the kept roots as a bit plane, their popcount per word, the members in kept components (one atomic per workgroup);
 *   rocPRIM exclusive scan over the popcounts: ranks in ascending label order;
 *   k_gfr_recinit  the counts; a record per kept root of rank < max_clusters, emptied;
 *   k_gfr_tile<1>  sums and boxes;
 *   k_gfr_tile<2>  (the sums are complete) the representative: the least dist^2 << 32 | id;
 *   k_gfr_finish   a lane per record: rep and its dist_sq, centroid, box in global coordinates.
 * k_gfr_tile is the statistics pass.  A WAVE takes a tile of 64 rows of one word column (64 x 64 cells), a lane one word of it.  A
 * lane walks the runs of its word; what a run adds to its component is closed form (length, n x0 + n (n - 1) / 2, n y, its ends,
 * the cell of the run nearest the centre) and is merged into the lane's pending sum while the component stays the same.  What has
 * to leave is aggregated over the wave first: while lanes remain, the first one's component is broadcast, the lanes that hold the
 * same are balloted, their values reduced by cross-lane butterflies (the other lanes feed the identity), and that lane issues ONE
 * set of atomics.  A component costs about one set per tile it crosses, not one per run: in gie_frontier.inc.h nine atomics per
 * stretch into one record were 80 % of a compute with one large component.  The loops are steered by ballots alone:
 * every lane of the wave takes every shuffle.
 * Every statistic is an integer atomic and every float is derived from the integers, so a result does not depend on scheduling.
 * The compiler's figures and the times are in DESIGN.md 22.
 */

enum { GIE_GFR_W_NCL = 0,       /* kept components */
       GIE_GFR_W_NCELL = 1,     /* members in kept components */
       GIE_GFR_NWORDS = 4 };
#define GIE_GFR_KEPT_WORDS 8    /* words a wave of k_gfr_kept takes, one after the other */

struct gie_gfr_dev {
    int32_t *par, *size;
    uint64_t *mem, *kept;
    int32_t *cnt, *rank, *w;
    gie_ground_frontier_cluster *rec;
    int W, nwords, ntiles, max_clusters, min_size;
};

/* bit index of the first cell of the run of set bits of w that holds bit b */
GIE_DEV int gie_gfr_head(const uint64_t w, const int b)
{
    const uint64_t gaps = ~w & ((1ull << b) - 1ull);            /* clear bits below b: the run starts above the highest */
    return gaps ? 64 - __builtin_clzll(gaps) : 0;
}

__global__ __launch_bounds__(256) void k_gfr_prep(const gie_ctx c, const gie_ground_dev g, const gie_gfr_dev s, const int clearance_sq)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const bool none = gie_ground_nobs(g) == 0;                  /* no obstacle column: dist_sq is -1 everywhere */
    const int y = wd / s.W, x0 = (wd - y * s.W) * 64, x = x0 + lane, id = y * c.X + x;
    bool mb = false;
    if (x < c.X) mb = g.type[id] == GIE_VOX_FNT && (none || g.dist[id] >= clearance_sq);
    const uint64_t m = __ballot(mb);
    if (lane == 0) s.mem[wd] = m;
    if (mb) {
        s.par[id] = y * c.X + x0 + gie_gfr_head(m, lane);
        s.size[id] = 0;
    }
}

__global__ __launch_bounds__(256) void k_gfr_merge(const gie_ctx c, const gie_gfr_dev s, const int conn8)
{
    const int wd = blockIdx.x * 256 + threadIdx.x;
    if (wd >= s.nwords) return;
    const uint64_t m = s.mem[wd];
    if (!m) return;
    const int W = s.W, X = c.X;
    const int y = wd / W, tx = wd - y * W;
    const int base = y * X + tx * 64;                           /* the cell of bit 0 */
    if ((m & 1ull) && tx > 0) {
        const uint64_t pm = s.mem[wd - 1];
        if (pm >> 63) gie_fr_unite(s.par, base, base - 64 + gie_gfr_head(pm, 63));
    }
    if (y == 0) return;
    const int nwd = wd - W, nbase = base - X;                   /* row y - 1: the other half of the neighbourhood is the neighbour's "before" */
    const uint64_t n = s.mem[nwd];
    const uint64_t nlw = conn8 && tx > 0 ? s.mem[nwd - 1] : 0ull;
    const bool nl = nlw >> 63;
    const bool nr = conn8 && tx < W - 1 && (s.mem[nwd + 1] & 1ull);
    if (!n && !nl && !nr) return;
    uint64_t mm = m;
    while (mm) {
        const int hb = __builtin_ctzll(mm);
        const uint64_t t = mm + (1ull << hb), r = mm & ~t;       /* the lowest run (t wraps to 0 when it ends at bit 63) */
        mm &= t;
        const uint64_t rd = conn8 ? (r | (r << 1) | (r >> 1)) : r;
        const uint64_t o = n & rd;
        for (uint64_t st = o & ~(o << 1); st; st &= st - 1) gie_fr_unite(s.par, base + hb, nbase + gie_gfr_head(n, __builtin_ctzll(st)));
        if (nl && (r & 1ull)) gie_fr_unite(s.par, base + hb, nbase - 64 + gie_gfr_head(nlw, 63));
        if (nr && (r >> 63)) gie_fr_unite(s.par, base + hb, nbase + 64);       /* (bit 0 is its run's head) */
    }
}

/* the record of root `root` (a member's label): -1 when its component is not kept or its rank is beyond the capacity */
GIE_DEV int gie_gfr_rank(const int X, const gie_gfr_dev &s, const int root)
{
    const int y = root / X, x = root - y * X, kwd = y * s.W + (x >> 6);
    const uint64_t kb = s.kept[kwd];
    if (!((kb >> (x & 63)) & 1ull)) return -1;
    const int r = s.rank[kwd] + __popcll(kb & ((1ull << (x & 63)) - 1ull));
    return r < s.max_clusters ? r : -1;
}

/* butterflies over the 64 lanes (every lane of the wave calls them) */
GIE_DEV int gie_gfr_wsum(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
GIE_DEV int gie_gfr_wmin(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
GIE_DEV int gie_gfr_wmax(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
GIE_DEV uint64_t gie_gfr_wmin64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

/* what a lane holds for one component: PASS 0 n; PASS 1 the sums (32 bits hold a tile's: 4096 cells of coordinates below 2^16)
 * and the box; PASS 2 the key */
struct gie_gfr_acc { int n, sx, sy, lox, hix, loy, hiy; uint64_t key; };

/* the lanes with `act` hand their sums to the components `key` (PASS 0: a root; PASS 1, 2: a record), one set of atomics per
 * distinct key.  Called by all lanes of the wave; the loop is steered by ballots alone */
template <int PASS> GIE_DEV void gie_gfr_flush(const gie_gfr_dev &s, const bool act, const int key, const gie_gfr_acc &a)
{
    const int lane = __lane_id();
    uint64_t todo = __ballot(act);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int k0 = __shfl(key, lead);
        const bool mine = act && key == k0;
        todo &= ~__ballot(mine);                                /* (every lane that holds k0 leaves now: lead among them) */
        if (PASS == 0) {
            const int n = gie_gfr_wsum(mine ? a.n : 0);
            if (lane == lead) gie_aadd32(&s.size[k0], n);
        } else if (PASS == 1) {
            const int sx = gie_gfr_wsum(mine ? a.sx : 0), sy = gie_gfr_wsum(mine ? a.sy : 0);
            const int lox = gie_gfr_wmin(mine ? a.lox : 0x7fffffff), hix = gie_gfr_wmax(mine ? a.hix : -0x7fffffff - 1);
            const int loy = gie_gfr_wmin(mine ? a.loy : 0x7fffffff), hiy = gie_gfr_wmax(mine ? a.hiy : -0x7fffffff - 1);
            if (lane == lead) {
                gie_ground_frontier_cluster *q = &s.rec[k0];
                atomicAdd((unsigned long long *)&q->sum[0], (unsigned long long)sx);
                atomicAdd((unsigned long long *)&q->sum[1], (unsigned long long)sy);
                atomicMin(&q->lo[0], lox); atomicMax(&q->hi[0], hix);
                atomicMin(&q->lo[1], loy); atomicMax(&q->hi[1], hiy);
            }
        } else {
            const uint64_t k = gie_gfr_wmin64(mine ? a.key : ~0ull);
            if (lane == lead) {
                uint64_t *kp = reinterpret_cast<uint64_t *>(&s.rec[k0].rep[0]);
                if (k < gie_ld(kp)) gie_amin64(kp, k);
            }
        }
    }
}

/* the statistics pass over 64 x 64 tiles.  PASS 0: heads get their root, sizes.  PASS 1: sums and boxes.  PASS 2: the representative */
template <int PASS>
__global__ __launch_bounds__(256) void k_gfr_tile(const gie_ctx c, const gie_gfr_dev s)
{
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= s.ntiles) return;                               /* wave-uniform */
    const int X = c.X;
    const int ty = tile / s.W, tx = tile - ty * s.W, y = ty * 64 + lane;
    uint64_t m = y < c.Y ? s.mem[y * s.W + tx] : 0ull;
    const int base = y * X + tx * 64;                           /* the cell of bit 0 (used where m has a bit only) */
    int pk = -1;                                                /* the component of the pending sums; -1: none */
    gie_gfr_acc P = { 0, 0, 0, 0, 0, 0, 0, 0ull };
    while (__ballot(m != 0ull)) {                               /* the k-th run of every lane's word */
        const bool has = m != 0ull;
        int k = -1;
        gie_gfr_acc A = { 0, 0, 0, 0, 0, 0, 0, ~0ull };
        if (has) {
            const int hb = __builtin_ctzll(m);
            const uint64_t t = m + (1ull << hb), r = m & ~t;     /* the lowest run (t wraps to 0 when it ends at bit 63) */
            m &= t;
            const int n = __popcll(r), head = base + hb, x0 = tx * 64 + hb, x1 = x0 + n - 1;
            if (PASS == 0) {
                k = gie_fr_root(s.par, head);
                if (k != head) gie_st(&s.par[head], k);          /* (the forest is final: whoever reads this link meanwhile gets to the same root) */
                A.n = n;
            } else {
                k = gie_gfr_rank(X, s, s.par[head]);
                if (PASS == 1) {
                    A.sx = n * x0 + n * (n - 1) / 2; A.sy = n * y;
                    A.lox = x0; A.hix = x1; A.loy = A.hiy = y;
                } else if (k >= 0) {
                    const gie_ground_frontier_cluster *q = &s.rec[k];
                    const long long sz = q->size;
                    const int cx = (int)((2 * q->sum[0] + sz) / (2 * sz)), cy = (int)((2 * q->sum[1] + sz) / (2 * sz));
                    const int xc = cx < x0 ? x0 : (cx > x1 ? x1 : cx);     /* the run's cell nearest the centre; no tie inside a run */
                    const int dx = xc - cx, dy = y - cy;
                    A.key = ((uint64_t)(dx * dx + dy * dy) << 32) | (uint32_t)(y * X + xc);
                }
            }
        }
        const bool same = has && k == pk;
        gie_gfr_flush<PASS>(s, has && !same && pk >= 0, pk, P);
        if (has) {
            if (same) {
                P.n += A.n; P.sx += A.sx; P.sy += A.sy;
                P.lox = A.lox < P.lox ? A.lox : P.lox; P.hix = A.hix > P.hix ? A.hix : P.hix;      /* (one row: loy, hiy stay) */
                P.key = A.key < P.key ? A.key : P.key;
            } else { pk = k; P = A; }
        }
    }
    gie_gfr_flush<PASS>(s, pk >= 0, pk, P);
}

__global__ __launch_bounds__(256) void k_gfr_kept(const gie_ctx c, const gie_gfr_dev s)
{
    __shared__ int s_n[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = (blockIdx.x * 4 + wave) * GIE_GFR_KEPT_WORDS;
    int tot = 0;
#pragma unroll 1
    for (int i = 0; i < GIE_GFR_KEPT_WORDS; i++) {
        const int wd = w0 + i;
        if (wd >= s.nwords) break;                              /* wave-uniform */
        const uint64_t m = s.mem[wd];
        int sz = 0;
        if ((m >> lane) & 1ull) {
            const int y = wd / s.W, id = y * c.X + (wd - y * s.W) * 64 + lane;
            if (s.par[id] == id) { sz = s.size[id]; if (sz < s.min_size) sz = 0; }
        }
        const uint64_t k = __ballot(sz > 0);
        tot += sz;
        if (lane == 0) { s.kept[wd] = k; s.cnt[wd] = __popcll(k); }
    }
    tot = gie_gfr_wsum(tot);
    if (lane == 0) s_n[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        if (t) gie_aadd32(&s.w[GIE_GFR_W_NCELL], t);
    }
}

__global__ __launch_bounds__(256) void k_gfr_recinit(const gie_ctx c, const gie_gfr_dev s, int32_t *d_counts)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int n = s.rank[s.nwords - 1] + s.cnt[s.nwords - 1];
        s.w[GIE_GFR_W_NCL] = n;
        if (d_counts) { d_counts[0] = n; d_counts[1] = s.w[GIE_GFR_W_NCELL]; }
    }
    const int wd = blockIdx.x * 256 + threadIdx.x;
    if (wd >= s.nwords) return;
    const int n = s.cnt[wd];
    if (!n) return;
    int r = s.rank[wd];
    const int y = wd / s.W, base = y * c.X + (wd - y * s.W) * 64;
    for (uint64_t k = s.kept[wd]; k && r < s.max_clusters; k &= k - 1, r++) {
        const int id = base + __builtin_ctzll(k);
        gie_ground_frontier_cluster q;
        q.label = id; q.size = s.size[id];
        for (int i = 0; i < 2; i++) { q.lo[i] = 0x7fffffff; q.hi[i] = -0x7fffffff - 1; q.rep[i] = -1; q.centroid[i] = 0.f; q.sum[i] = 0; }
        q.rep_dist_sq = 0; q.reserved = 0;
        s.rec[r] = q;                                           /* (rep = all ones: the largest key of k_gfr_tile<2>) */
    }
}

__global__ __launch_bounds__(256) void k_gfr_finish(const gie_ctx c, const gie_ground_dev g, const gie_gfr_dev s)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    int n = s.w[GIE_GFR_W_NCL]; if (n > s.max_clusters) n = s.max_clusters;
    if (r >= n) return;
    gie_ground_frontier_cluster *q = &s.rec[r];
    const int id = (int)(uint32_t)(*reinterpret_cast<const uint64_t *>(&q->rep[0]) & 0xffffffffull);
    const int y = id / c.X, x = id - y * c.X;
    const int v[2] = { x, y };
    for (int k = 0; k < 2; k++) {
        q->rep[k] = v[k] + g.pvt[k];
        q->lo[k] += g.pvt[k]; q->hi[k] += g.pvt[k];
        q->centroid[k] = ((float)((double)q->sum[k] / (double)q->size) + (float)g.pvt[k]) * c.voxel_width;
    }
    q->rep_dist_sq = gie_ground_nobs(g) == 0 ? -1 : g.dist[id];
}

/* the cluster reader: a lane per capacity entry */
__global__ __launch_bounds__(256) void k_gfr_read(const gie_gfr_dev s, const float w, gie_ground_frontier_cluster *out, float *goal, int32_t *n_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = s.w[GIE_GFR_W_NCL];
    if (i == 0 && n_out) *n_out = n;
    if (i >= s.max_clusters) return;
    const bool have = i < n;
    if (have && out) out[i] = s.rec[i];
    if (goal) for (int k = 0; k < 2; k++) goal[2 * (size_t)i + k] = have ? (float)s.rec[i].rep[k] * w : __builtin_nanf("");
}

struct op_gfr_labels {
    const int32_t *par, *size; const uint64_t *mem; int W, min_size; int32_t *out;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int y = i / c.X, x = i - y * c.X;
        int v = -1;
        if ((mem[(size_t)y * W + (x >> 6)] >> (x & 63)) & 1ull) { const int root = par[par[i]]; v = size[root] >= min_size ? root : -2; }
        out[i] = v;
    }
};

/* ---- host side */
static gie_gfr_dev gie_gfr_view(const gie_mapper *m)
{
    const int X = m->c.X, Y = m->c.Y;
    const size_t cells = (size_t)X * Y;
    gie_gfr_dev s;
    s.W = (X + 63) / 64; s.nwords = s.W * Y; s.ntiles = s.W * ((Y + 63) / 64);
    s.par = m->gfr.planes; s.size = s.par + cells;
    s.mem = m->gfr.bits; s.kept = s.mem + s.nwords;
    s.cnt = m->gfr.words; s.rank = s.cnt + s.nwords; s.w = s.rank + s.nwords;
    s.rec = (gie_ground_frontier_cluster *)m->gfr.rec;
    s.max_clusters = m->gfr.max_clusters; s.min_size = m->gfr.min_size;
    return s;
}
static int gie_gfr_check(gie_mapper *m, const char *who, bool need_result)
{
    static_assert(sizeof(gie_ground_frontier_cluster) == 64 && offsetof(gie_ground_frontier_cluster, sum) == 40 && offsetof(gie_ground_frontier_cluster, rep) == 24 &&
                  sizeof(gie_ground_frontier_param) == 32, "the sizes include/gie.h states");
    const int rc = gie_ground_check(m, who, true, "components"); if (rc) return rc;
    if (need_result && !m->gfr.valid) { gie_set_err(std::string(who) + ": no frontier clusters of this ground field (gie_ground_frontier_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_gfr_check_compute(gie_mapper *m, const char *who, const gie_ground_frontier_param *p)
{
    const int rc = gie_gfr_check(m, who, false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->min_size < 1) bad = "min_size must be >= 1";
    else if (p->connectivity != 4 && p->connectivity != 8) bad = "connectivity is 4 or 8";
    else if (p->max_clusters < 0) bad = "max_clusters must be >= 0";
    else if (p->flags) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2]) bad = "reserved must be 0";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_ground_frontier_compute_dev(gie_mapper *m, const gie_ground_frontier_param *p, int32_t *d_counts)
{
    const int rc = gie_gfr_check_compute(m, "gie_ground_frontier_compute_dev", p); if (rc) return rc;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const int nwords = g.W * c.Y;
    if (!m->gfr.planes) {
        int32_t *planes = gie_dalloc<int32_t>(m, 2 * (size_t)c.X * c.Y, false);
        uint64_t *bits = planes ? gie_dalloc<uint64_t>(m, 2 * (size_t)nwords, false) : nullptr;
        int32_t *words = bits ? gie_dalloc<int32_t>(m, 2 * (size_t)nwords + GIE_GFR_NWORDS, false) : nullptr;
        if (!words) { gie_set_err("gie_ground_frontier_compute_dev: device allocation of the ground frontier planes failed"); return GIE_ERR_DEVICE; }
        m->gfr.bits = bits; m->gfr.words = words; m->gfr.planes = planes;
    }
    if (p->max_clusters > m->gfr.rec_cap) {                     /* the records grow with the largest capacity asked for */
        void *rec = be_alloc(&m->be, (size_t)p->max_clusters * sizeof(gie_ground_frontier_cluster), false);
        if (!rec) { gie_set_err("gie_ground_frontier_compute_dev: device allocation of the cluster records failed"); return GIE_ERR_DEVICE; }
        if (m->gfr.rec) {
            for (void *&q : m->allocs) if (q == m->gfr.rec) q = rec;
            be_free(&m->be, m->gfr.rec);
        } else m->allocs.push_back(rec);
        m->gfr.rec = rec; m->gfr.rec_cap = p->max_clusters;
    }
    m->gfr.max_clusters = p->max_clusters; m->gfr.min_size = p->min_size;
    const gie_gfr_dev s = gie_gfr_view(m);
    const dim3 gw((nwords + 3) / 4), gl((nwords + 255) / 256), gt((s.ntiles + 3) / 4), t(256);     /* a wave per word / a lane per word / a wave per tile */
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 0);
    be_memset(&m->be, s.w, 0, GIE_GFR_NWORDS * sizeof(int32_t));
    GIE_LAUNCH(&m->be, k_gfr_prep, gw, t, 0, c, g, s, (int)p->clearance_sq);
    GIE_LAUNCH(&m->be, k_gfr_merge, gl, t, 0, c, s, p->connectivity == 8 ? 1 : 0);
    GIE_LAUNCH(&m->be, k_gfr_tile<0>, gt, t, 0, c, s);
    GIE_LAUNCH(&m->be, k_gfr_kept, dim3((nwords + 4 * GIE_GFR_KEPT_WORDS - 1) / (4 * GIE_GFR_KEPT_WORDS)), t, 0, c, s);
    be_exclusive_scan(&m->be, s.cnt, s.rank, nwords);
    GIE_LAUNCH(&m->be, k_gfr_recinit, gl, t, 0, c, s, d_counts);
    if (p->max_clusters > 0) {
        GIE_LAUNCH(&m->be, k_gfr_tile<1>, gt, t, 0, c, s);
        GIE_LAUNCH(&m->be, k_gfr_tile<2>, gt, t, 0, c, s);
        GIE_LAUNCH(&m->be, k_gfr_finish, dim3((p->max_clusters + 255) / 256), t, 0, c, g, s);
    }
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 1);
    m->gfr.valid = 1;
    return GIE_OK;
}
extern "C" int gie_ground_frontier_compute(gie_mapper *m, const gie_ground_frontier_param *p, int32_t *n_clusters, int32_t *n_cells)
{
    int rc = gie_gfr_check_compute(m, "gie_ground_frontier_compute", p); if (rc) return rc;
    rc = gie_ground_frontier_compute_dev(m, p, nullptr); if (rc) return rc;
    int32_t w[2] = { 0, 0 };
    be_d2h(&m->be, w, gie_gfr_view(m).w, sizeof(w));
    rc = gie_sync(m);
    if (n_clusters) *n_clusters = w[GIE_GFR_W_NCL];
    if (n_cells) *n_cells = w[GIE_GFR_W_NCELL];
    return rc;
}
extern "C" int gie_read_ground_frontier_clusters_dev(gie_mapper *m, gie_ground_frontier_cluster *d_out, float *d_goal_xy, int32_t *d_n_clusters)
{
    const int rc = gie_gfr_check(m, "gie_read_ground_frontier_clusters_dev", true); if (rc) return rc;
    if (!d_out && !d_goal_xy) { gie_set_err("gie_read_ground_frontier_clusters_dev: both outputs are null"); return GIE_ERR_INVALID; }
    const gie_gfr_dev s = gie_gfr_view(m);
    const int n = s.max_clusters > 0 ? s.max_clusters : 1;
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 0);
    GIE_LAUNCH(&m->be, k_gfr_read, dim3((n + 255) / 256), dim3(256), 0, s, m->c.voxel_width, d_out, d_goal_xy, d_n_clusters);
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground_frontier_clusters(gie_mapper *m, gie_ground_frontier_cluster *out, float *goal_xy, int32_t *n_clusters)
{
    int rc = gie_gfr_check(m, "gie_read_ground_frontier_clusters", true); if (rc) return rc;
    if (!out && !goal_xy) { gie_set_err("gie_read_ground_frontier_clusters: both outputs are null"); return GIE_ERR_INVALID; }
    const size_t cap = (size_t)m->gfr.max_clusters;
    char *d = (char *)gie_scratch(m, 0, 16 + cap * (sizeof(gie_ground_frontier_cluster) + 8), "gie_read_ground_frontier_clusters");
    if (!d) return GIE_ERR_DEVICE;
    gie_ground_frontier_cluster *dr = (gie_ground_frontier_cluster *)(d + 16);
    float *dg = (float *)(d + 16 + cap * sizeof(gie_ground_frontier_cluster));
    rc = gie_read_ground_frontier_clusters_dev(m, out ? dr : nullptr, goal_xy ? dg : nullptr, (int32_t *)d); if (rc) return rc;
    int32_t n = 0;
    be_d2h(&m->be, &n, d, sizeof(n));
    if (n_clusters) *n_clusters = n;
    const size_t have = (size_t)n < cap ? (size_t)n : cap;      /* (entries beyond the records produced are left as they are) */
    if (out && have) be_d2h(&m->be, out, dr, have * sizeof(gie_ground_frontier_cluster));
    if (goal_xy && cap) be_d2h(&m->be, goal_xy, dg, cap * 8);
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_read_ground_frontier_labels_dev(gie_mapper *m, int32_t *d_labels)
{
    const int rc = gie_gfr_check(m, "gie_read_ground_frontier_labels_dev", true); if (rc) return rc;
    if (!d_labels) { gie_set_err("gie_read_ground_frontier_labels_dev: null output"); return GIE_ERR_INVALID; }
    gie_ctx c;
    (void)gie_ground_view(m, &c);
    const gie_gfr_dev s = gie_gfr_view(m);
    op_gfr_labels op; op.par = s.par; op.size = s.size; op.mem = s.mem; op.W = s.W; op.min_size = s.min_size; op.out = d_labels;
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND_FRONTIER, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground_frontier_labels(gie_mapper *m, int32_t *labels)
{
    int rc = gie_gfr_check(m, "gie_read_ground_frontier_labels", true); if (rc) return rc;
    if (!labels) { gie_set_err("gie_read_ground_frontier_labels: null output"); return GIE_ERR_INVALID; }
    const size_t n = (size_t)m->c.X * m->c.Y;
    int32_t *d = (int32_t *)gie_scratch(m, 1, n * 4, "gie_read_ground_frontier_labels");
    if (!d) return GIE_ERR_DEVICE;
    rc = gie_read_ground_frontier_labels_dev(m, d); if (rc) return rc;
    be_d2h(&m->be, labels, d, n * 4);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_frontier.inc.h — frontier clusters: the connected components of the local volume's FNT voxels, filtered by size, with a
 * record (size, box, centroid, representative voxel) per kept component (include/gie.h "frontier clusters").
 * HIP backend only: included by gie_hip.hip after gie_nf1.inc.h; nothing of the map update reads what is computed here.
 *
 * The cache (gie_mapper::fr), allocated at the first compute:
 *   par    int32 per voxel, written at members only: the union-find forest, after k_fr_flatten the component's label;
 *   size   int32 per voxel, written at members only, read at roots: the component's size;
 *   mem    one bit per voxel, member: rows of W = ceil(X/64) 64-bit words, bit x & 63 of word x >> 6 (as NF1's trav plane);
 *   kept   same layout: the roots of the kept components;
 *   cnt    int32 per row word: popcount of kept; rank: its exclusive scan (the rank of a word's first kept root);
 *   w      GIE_FR_NWORDS control words (the two counts);
 *   rec    max_clusters records (grows with the largest max_clusters asked for).
 * A compute is a fixed sequence of launches, none of them a loop of the host's and none with a grid barrier:
 *   k_fr_prep     a lane per voxel, a wave per row word: the member plane; par = the first voxel of the member's x-run inside
 *                 its word, size = 0;
 *   k_fr_merge    a lane per row word: every run of the word is united with the runs it touches in the rows before it (2 rows at
 *                 connectivity 6, 4 at 26 — the other half of the neighbourhood is the neighbour's "before") and in the word
 *                 before it; union-find: a compare-and-swap hangs the larger root below the smaller, so a root is always its
 *                 tree's smallest index and the final root is the component's label whatever the schedule;
 *   k_fr_flatten  a lane per voxel: par = root; one atomicAdd on size[root] per stretch of lanes that share a root;
 *   k_fr_kept     the kept roots as a bit plane, their popcount per word, the members in kept components;
 *   rocPRIM exclusive scan over the popcounts: ranks in ascending label order;
 *   k_fr_recinit  the counts; a record per kept root of rank < max_clusters, emptied;
 *   k_fr_stats    integer atomics per stretch of lanes that share a root: sums, box;
 *   k_fr_rep      (the sums are complete) one 64-bit atomicMin per member on dist^2 << 32 | id;
 *   k_fr_finish   a lane per record: rep, centroid, box in global coordinates.
 * Every statistic is an integer atomic and every float is derived from the integers, so a result does not depend on scheduling.
 */

enum { GIE_FR_W_NCL = 0,        /* kept components */
       GIE_FR_W_NVOX = 1,       /* members in kept components */
       GIE_FR_NWORDS = 4 };

struct gie_fr_dev {
    int32_t *par, *size;
    uint64_t *mem, *kept;
    int32_t *cnt, *rank, *w;
    gie_frontier_cluster *rec;
    int W, nwords, max_clusters, min_size;
};

/* the root of x's tree, halving the path on the way: a link of a voxel that is not a root is only ever replaced by one to an
 * ancestor (here and in k_fr_flatten), a root's only by the compare-and-swap of gie_fr_unite */
GIE_DEV int gie_fr_find(int32_t *par, int x)
{
    for (;;) {
        const int p = gie_ld(&par[x]); if (p == x) return x;
        const int g = gie_ld(&par[p]); if (g == p) return p;
        gie_st(&par[x], g);
        x = g;
    }
}
/* the same without the halving: k_fr_flatten's, where a voxel's link is written by its own lane only (to the root, for good) */
GIE_DEV int gie_fr_root(const int32_t *par, int x)
{
    for (;;) { const int p = gie_ld(&par[x]); if (p == x) return x; x = p; }
}
/* a and b are members of one component: join their trees.  The larger root is hung below the smaller one, so a tree's root is
 * its smallest index at all times and the final root is the component's label whatever the schedule */
GIE_DEV void gie_fr_unite(int32_t *par, int a, int b)
{
    for (;;) {
        a = gie_fr_find(par, a); b = gie_fr_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expect = a;
        if (__hip_atomic_compare_exchange_strong(&par[a], &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = expect;                                             /* (a has been hung below another root meanwhile) */
    }
}

__global__ __launch_bounds__(256) void k_fr_prep(const gie_ctx c, const gie_fr_dev s, const float clearance)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const int row = wd / s.W, x0 = (wd - row * s.W) * 64, x = x0 + lane;
    const int id = row * c.X + x;
    bool mb = false;
    if (x < c.X) {
        mb = c.glb_type[id] == GIE_VOX_FNT;
        if (mb && clearance > 0.f) mb = gie_edt_value(c, id) >= clearance;    /* (edt >= 0 always) */
    }
    const uint64_t m = __ballot(mb);
    if (lane == 0) s.mem[wd] = m;
    if (mb) {
        const uint64_t gaps = ~m & ((1ull << lane) - 1ull);     /* non-members below this lane: the run starts above the highest */
        const int head = gaps ? 64 - __builtin_clzll(gaps) : 0;
        s.par[id] = row * c.X + x0 + head;
        s.size[id] = 0;
    }
}

__global__ __launch_bounds__(256) void k_fr_merge(const gie_ctx c, const gie_fr_dev s, const int conn26)
{
    const int wd = blockIdx.x * 256 + threadIdx.x;
    if (wd >= s.nwords) return;
    const uint64_t m = s.mem[wd];
    if (!m) return;
    const int W = s.W, X = c.X, Y = c.Y;
    const int row = wd / W, tx = wd - row * W, y = row % Y, z = row / Y;
    const int base = row * X + tx * 64;                         /* the voxel of bit 0 */
    if ((m & 1ull) && tx > 0 && (s.mem[wd - 1] >> 63)) gie_fr_unite(s.par, base, base - 1);
    const int nrows = conn26 ? 4 : 2;
#pragma unroll 1
    for (int k = 0; k < nrows; k++) {
        const int dy = k == 1 ? 0 : (k == 3 ? 1 : -1), dz = k == 0 ? 0 : -1;     /* (-1,0) (0,-1) (-1,-1) (+1,-1) */
        const int ny = y + dy, nz = z + dz;
        if (ny < 0 || ny >= Y || nz < 0) continue;
        const int drow = dz * Y + dy, nwd = wd + drow * W, nbase = base + drow * X;
        const uint64_t n = s.mem[nwd];
        const bool nl = conn26 && tx > 0 && (s.mem[nwd - 1] >> 63);
        const bool nr = conn26 && tx < W - 1 && (s.mem[nwd + 1] & 1ull);
        if (!n && !nl && !nr) continue;
        uint64_t mm = m;
        while (mm) {
            const int hb = __builtin_ctzll(mm);
            const uint64_t t = mm + (1ull << hb), r = mm & ~t;   /* the lowest run (t wraps to 0 when it ends at bit 63) */
            mm &= t;
            const uint64_t rd = conn26 ? (r | (r << 1) | (r >> 1)) : r;
            const uint64_t o = n & rd;
            for (uint64_t st = o & ~(o << 1); st; st &= st - 1) gie_fr_unite(s.par, base + hb, nbase + __builtin_ctzll(st));
            if (nl && (r & 1ull)) gie_fr_unite(s.par, base + hb, nbase - 1);
            if (nr && (r >> 63)) gie_fr_unite(s.par, base + hb, nbase + 64);
        }
    }
}

/* the stretch of lanes [lane, lane + n) that starts at this lane: consecutive active lanes with the same key.  Returns n for the
 * first lane of a stretch and 0 for every other lane (all lanes of the wave call it) */
GIE_DEV int gie_fr_stretch(const bool active, const int key)
{
    const int lane = __lane_id();
    const int pk = __shfl_up(key, 1);
    const uint64_t a = __ballot(active);
    const bool same = active && lane > 0 && ((a >> (lane - 1)) & 1ull) && pk == key;
    const uint64_t h = __ballot(active && !same);
    if (!active || same) return 0;
    const uint64_t above = a >> lane, hh = (h >> lane) & ~1ull;
    const int run = ~above ? __builtin_ctzll(~above) : 64 - lane;
    const int nh = hh ? __builtin_ctzll(hh) : 64;
    return run < nh ? run : nh;
}

__global__ __launch_bounds__(256) void k_fr_flatten(const gie_ctx c, const gie_fr_dev s)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const uint64_t m = s.mem[wd];
    if (!m) return;                                             /* wave-uniform */
    const int row = wd / s.W, id = row * c.X + (wd - row * s.W) * 64 + lane;
    const bool mb = (m >> lane) & 1ull;
    int root = -1;
    if (mb) {
        root = gie_fr_root(s.par, id);
        if (root != id) gie_st(&s.par[id], root);               /* (the forest is final: whoever reads this link meanwhile gets to the same root) */
    }
    const int n = gie_fr_stretch(mb, root);
    if (n) gie_aadd32(&s.size[root], n);
}

__global__ __launch_bounds__(256) void k_fr_kept(const gie_ctx c, const gie_fr_dev s)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const uint64_t m = s.mem[wd];
    if (!m) { if (lane == 0) { s.kept[wd] = 0; s.cnt[wd] = 0; } return; }
    const int row = wd / s.W, id = row * c.X + (wd - row * s.W) * 64 + lane;
    int sz = 0;
    if (((m >> lane) & 1ull) && s.par[id] == id) { sz = s.size[id]; if (sz < s.min_size) sz = 0; }
    const uint64_t k = __ballot(sz > 0);
    for (int i = 1; i < 64; i <<= 1) sz += __shfl_xor(sz, i);
    if (lane == 0) { s.kept[wd] = k; s.cnt[wd] = __popcll(k); if (sz) gie_aadd32(&s.w[GIE_FR_W_NVOX], sz); }
}

/* the record of root `root` (a member's label): -1 when its component is not kept or its rank is beyond the capacity */
GIE_DEV int gie_fr_rank(const gie_ctx &c, const gie_fr_dev &s, const int root)
{
    const int row = root / c.X, x = root - row * c.X, kwd = row * s.W + (x >> 6);
    const uint64_t kb = s.kept[kwd];
    if (!((kb >> (x & 63)) & 1ull)) return -1;
    const int r = s.rank[kwd] + __popcll(kb & ((1ull << (x & 63)) - 1ull));
    return r < s.max_clusters ? r : -1;
}

__global__ __launch_bounds__(256) void k_fr_recinit(const gie_ctx c, const gie_fr_dev s, int32_t *d_counts)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int n = s.rank[s.nwords - 1] + s.cnt[s.nwords - 1];
        s.w[GIE_FR_W_NCL] = n;
        if (d_counts) { d_counts[0] = n; d_counts[1] = s.w[GIE_FR_W_NVOX]; }
    }
    const int wd = blockIdx.x * 256 + threadIdx.x;
    if (wd >= s.nwords) return;
    const int n = s.cnt[wd];
    if (!n) return;
    int r = s.rank[wd];
    const int row = wd / s.W, base = row * c.X + (wd - row * s.W) * 64;
    for (uint64_t k = s.kept[wd]; k && r < s.max_clusters; k &= k - 1, r++) {
        const int id = base + __builtin_ctzll(k);
        gie_frontier_cluster q;
        q.label = id; q.size = s.size[id];
        for (int i = 0; i < 3; i++) { q.lo[i] = 0x7fffffff; q.hi[i] = -0x7fffffff - 1; q.rep[i] = -1; q.centroid[i] = 0.f; q.sum[i] = 0; }
        s.rec[r] = q;                                           /* (rep[0..1] = all ones: the largest key of k_fr_rep) */
    }
}

__global__ __launch_bounds__(256) void k_fr_stats(const gie_ctx c, const gie_fr_dev s)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const uint64_t m = s.mem[wd];
    if (!m) return;                                             /* wave-uniform */
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane, y = row % c.Y, z = row / c.Y;
    const bool mb = (m >> lane) & 1ull;
    const int r = mb ? gie_fr_rank(c, s, s.par[row * c.X + x]) : -1;
    const int n = gie_fr_stretch(r >= 0, r);
    if (!n) return;
    /* lanes x .. x + n - 1 of one row */
    gie_frontier_cluster *q = &s.rec[r];
    atomicAdd((unsigned long long *)&q->sum[0], (unsigned long long)n * (unsigned long long)x + (unsigned long long)(n * (n - 1) / 2));
    atomicAdd((unsigned long long *)&q->sum[1], (unsigned long long)n * (unsigned long long)y);
    atomicAdd((unsigned long long *)&q->sum[2], (unsigned long long)n * (unsigned long long)z);
    atomicMin(&q->lo[0], x); atomicMax(&q->hi[0], x + n - 1);
    atomicMin(&q->lo[1], y); atomicMax(&q->hi[1], y);
    atomicMin(&q->lo[2], z); atomicMax(&q->hi[2], z);
}

__global__ __launch_bounds__(256) void k_fr_rep(const gie_ctx c, const gie_fr_dev s)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const uint64_t m = s.mem[wd];
    if (!((m >> lane) & 1ull)) return;
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane, y = row % c.Y, z = row / c.Y, id = row * c.X + x;
    const int r = gie_fr_rank(c, s, s.par[id]);
    if (r < 0) return;
    gie_frontier_cluster *q = &s.rec[r];
    const long long sz = q->size;
    const long long dx = x - (2 * q->sum[0] + sz) / (2 * sz), dy = y - (2 * q->sum[1] + sz) / (2 * sz), dz = z - (2 * q->sum[2] + sz) / (2 * sz);
    const uint64_t key = ((uint64_t)(dx * dx + dy * dy + dz * dz) << 32) | (uint32_t)id;
    uint64_t *kp = reinterpret_cast<uint64_t *>(&q->rep[0]);
    if (key < gie_ld(kp)) gie_amin64(kp, key);
}

__global__ __launch_bounds__(256) void k_fr_finish(const gie_ctx c, const gie_fr_dev s)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    int n = s.w[GIE_FR_W_NCL]; if (n > s.max_clusters) n = s.max_clusters;
    if (r >= n) return;
    gie_frontier_cluster *q = &s.rec[r];
    const int id = (int)(uint32_t)(*reinterpret_cast<const uint64_t *>(&q->rep[0]) & 0xffffffffull);
    const int plane = c.X * c.Y, z = id / plane, y = (id - z * plane) / c.X, x = id - z * plane - y * c.X;
    const int v[3] = { x, y, z };
    for (int k = 0; k < 3; k++) {
        q->rep[k] = v[k] + c.pvt[k];
        q->lo[k] += c.pvt[k]; q->hi[k] += c.pvt[k];
        q->centroid[k] = ((float)((double)q->sum[k] / (double)q->size) + (float)c.pvt[k]) * c.voxel_width;
    }
}

/* the cluster reader: a lane per capacity entry */
__global__ __launch_bounds__(256) void k_fr_read(const gie_fr_dev s, const float w, gie_frontier_cluster *out, float *goal, int32_t *n_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = s.w[GIE_FR_W_NCL];
    if (i == 0 && n_out) *n_out = n;
    if (i >= s.max_clusters) return;
    const bool have = i < n;
    if (have && out) out[i] = s.rec[i];
    if (goal) for (int k = 0; k < 3; k++) goal[3 * i + k] = have ? (float)s.rec[i].rep[k] * w : __builtin_nanf("");
}

struct op_fr_labels {
    const int32_t *par, *size; const uint64_t *mem; int W, min_size; int32_t *out;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int row = i / c.X, x = i - row * c.X;
        int v = -1;
        if ((mem[(size_t)row * W + (x >> 6)] >> (x & 63)) & 1ull) { const int root = par[i]; v = size[root] >= min_size ? root : -2; }
        out[i] = v;
    }
};

/* ---- host side */
static gie_fr_dev gie_fr_view(const gie_mapper *m)
{
    const gie_ctx &c = m->c;
    gie_fr_dev s;
    s.W = (c.X + 63) / 64; s.nwords = s.W * c.Y * c.Z;
    s.par = m->fr.planes; s.size = s.par + (size_t)c.N;
    s.mem = m->fr.bits; s.kept = s.mem + s.nwords;
    s.cnt = m->fr.words; s.rank = s.cnt + s.nwords; s.w = s.rank + s.nwords;
    s.rec = (gie_frontier_cluster *)m->fr.rec;
    s.max_clusters = m->fr.max_clusters; s.min_size = m->fr.min_size;
    return s;
}
static int gie_fr_check(gie_mapper *m, const char *who, bool need_result)
{
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) { gie_set_err(std::string(who) + ": not for a tiled mapper (its components would stop at the tile's faces)"); return GIE_ERR_INVALID; }
    if (need_result && !m->fr.valid) { gie_set_err(std::string(who) + ": no frontier clusters yet (gie_frontier_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_frontier_compute_dev(gie_mapper *m, const gie_frontier_param *p, int32_t *d_counts)
{
    static_assert(sizeof(gie_frontier_cluster) == 80, "gie_frontier_cluster is 80 bytes");
    int rc = gie_fr_check(m, "gie_frontier_compute_dev", false); if (rc) return rc;
    if (!p) { gie_set_err("gie_frontier_compute_dev: null parameters"); return GIE_ERR_INVALID; }
    if (!(p->clearance >= 0.f && p->clearance <= 3.402823466e38f)) { gie_set_err("gie_frontier_compute_dev: clearance must be finite and >= 0"); return GIE_ERR_INVALID; }
    if (p->connectivity != 6 && p->connectivity != 26) { gie_set_err("gie_frontier_compute_dev: connectivity is 6 or 26"); return GIE_ERR_INVALID; }
    if (p->min_size < 1 || p->max_clusters < 0) { gie_set_err("gie_frontier_compute_dev: min_size >= 1 and max_clusters >= 0"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this stage) */
    const int W = (c.X + 63) / 64, nwords = W * c.Y * c.Z;
    if (!m->fr.planes) {
        int32_t *planes = gie_dalloc<int32_t>(m, 2 * (size_t)c.N, false);
        uint64_t *bits = planes ? gie_dalloc<uint64_t>(m, 2 * (size_t)nwords, false) : nullptr;
        int32_t *words = bits ? gie_dalloc<int32_t>(m, 2 * (size_t)nwords + GIE_FR_NWORDS, false) : nullptr;
        if (!words) { gie_set_err("gie_frontier_compute_dev: device allocation of the frontier planes failed"); return GIE_ERR_DEVICE; }
        m->fr.planes = planes; m->fr.bits = bits; m->fr.words = words;
    }
    if (p->max_clusters > m->fr.rec_cap) {                      /* the records grow with the largest capacity asked for */
        void *rec = be_alloc(&m->be, (size_t)p->max_clusters * sizeof(gie_frontier_cluster), false);
        if (!rec) { gie_set_err("gie_frontier_compute_dev: device allocation of the cluster records failed"); return GIE_ERR_DEVICE; }
        if (m->fr.rec) {
            for (void *&q : m->allocs) if (q == m->fr.rec) q = rec;
            be_free(&m->be, m->fr.rec);
        } else m->allocs.push_back(rec);
        m->fr.rec = rec; m->fr.rec_cap = p->max_clusters;
    }
    m->fr.max_clusters = p->max_clusters; m->fr.min_size = p->min_size;
    const gie_fr_dev s = gie_fr_view(m);
    const dim3 gw((nwords + 3) / 4), gl((nwords + 255) / 256), t(256);      /* a wave per word / a lane per word */
    be_memset(&m->be, s.w, 0, GIE_FR_NWORDS * sizeof(int32_t));
    GIE_LAUNCH(&m->be, k_fr_prep, gw, t, 0, c, s, p->clearance);
    GIE_LAUNCH(&m->be, k_fr_merge, gl, t, 0, c, s, p->connectivity == 26 ? 1 : 0);
    GIE_LAUNCH(&m->be, k_fr_flatten, gw, t, 0, c, s);
    GIE_LAUNCH(&m->be, k_fr_kept, gw, t, 0, c, s);
    be_exclusive_scan(&m->be, s.cnt, s.rank, nwords);
    GIE_LAUNCH(&m->be, k_fr_recinit, gl, t, 0, c, s, d_counts);
    if (p->max_clusters > 0) {
        GIE_LAUNCH(&m->be, k_fr_stats, gw, t, 0, c, s);
        GIE_LAUNCH(&m->be, k_fr_rep, gw, t, 0, c, s);
        GIE_LAUNCH(&m->be, k_fr_finish, dim3((p->max_clusters + 255) / 256), t, 0, c, s);
    }
    for (int i = 0; i < 3; i++) m->fr.pvt[i] = c.pvt[i];
    m->fr.valid = 1;
    return GIE_OK;
}
extern "C" int gie_frontier_compute(gie_mapper *m, const gie_frontier_param *p, int32_t *n_clusters, int32_t *n_voxels)
{
    int rc = gie_fr_check(m, "gie_frontier_compute", false); if (rc) return rc;
    rc = gie_frontier_compute_dev(m, p, nullptr); if (rc) return rc;
    int32_t w[2] = { 0, 0 };
    be_d2h(&m->be, w, m->fr.words + 2 * (size_t)gie_fr_view(m).nwords, sizeof(w));
    if (n_clusters) *n_clusters = w[GIE_FR_W_NCL];
    if (n_voxels) *n_voxels = w[GIE_FR_W_NVOX];
    return gie_sync(m);
}
extern "C" int gie_read_frontier_clusters_dev(gie_mapper *m, gie_frontier_cluster *d_out, float *d_goal_xyz, int32_t *d_n_clusters)
{
    int rc = gie_fr_check(m, "gie_read_frontier_clusters_dev", true); if (rc) return rc;
    const gie_fr_dev s = gie_fr_view(m);
    const int n = s.max_clusters > 0 ? s.max_clusters : 1;
    GIE_LAUNCH(&m->be, k_fr_read, dim3((n + 255) / 256), dim3(256), 0, s, m->c.voxel_width, d_out, d_goal_xyz, d_n_clusters);
    return GIE_OK;
}
extern "C" int gie_read_frontier_clusters(gie_mapper *m, gie_frontier_cluster *out, float *goal_xyz, int32_t *n_clusters)
{
    int rc = gie_fr_check(m, "gie_read_frontier_clusters", true); if (rc) return rc;
    const size_t cap = (size_t)m->fr.max_clusters;
    char *d = (char *)gie_scratch(m, 0, 16 + cap * (sizeof(gie_frontier_cluster) + 12), "gie_read_frontier_clusters");
    if (!d) return GIE_ERR_DEVICE;
    gie_frontier_cluster *dr = (gie_frontier_cluster *)(d + 16);
    float *dg = (float *)(d + 16 + cap * sizeof(gie_frontier_cluster));
    rc = gie_read_frontier_clusters_dev(m, out ? dr : nullptr, goal_xyz ? dg : nullptr, (int32_t *)d); if (rc) return rc;
    int32_t n = 0;
    be_d2h(&m->be, &n, d, sizeof(n));
    if (n_clusters) *n_clusters = n;
    const size_t have = (size_t)n < cap ? (size_t)n : cap;      /* (entries beyond the records produced are left as they are) */
    if (out && have) be_d2h(&m->be, out, dr, have * sizeof(gie_frontier_cluster));
    if (goal_xyz && cap) be_d2h(&m->be, goal_xyz, dg, cap * 12);
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_read_frontier_labels_dev(gie_mapper *m, int32_t *d_labels)
{
    int rc = gie_fr_check(m, "gie_read_frontier_labels_dev", true); if (rc) return rc;
    if (!d_labels) { gie_set_err("gie_read_frontier_labels_dev: null output"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;
    const gie_fr_dev s = gie_fr_view(m);
    op_fr_labels op; op.par = s.par; op.size = s.size; op.mem = s.mem; op.W = s.W; op.min_size = s.min_size; op.out = d_labels;
    be_lin(&m->be, c, op, c.N);
    return GIE_OK;
}
extern "C" int gie_read_frontier_labels(gie_mapper *m, int32_t *labels)
{
    int rc = gie_fr_check(m, "gie_read_frontier_labels", true); if (rc) return rc;
    if (labels) {
        const size_t N = (size_t)m->c.N;
        int32_t *d = (int32_t *)gie_scratch(m, 1, N * 4, "gie_read_frontier_labels");
        if (!d) return GIE_ERR_DEVICE;
        rc = gie_read_frontier_labels_dev(m, d); if (rc) return rc;
        be_d2h(&m->be, labels, d, N * 4);
        gie_scratch_trim(m);
    }
    return gie_sync(m);
}

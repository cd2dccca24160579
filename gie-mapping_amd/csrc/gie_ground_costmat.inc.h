/*
 * gie_ground_costmat.inc.h — the goal-to-goal cost matrix of the ground costmap: the 4-connected path lengths among up to 256 points
 * (include/gie.h "ground cost matrix").
 * HIP backend only: included by gie_hip.hip after gie_ground_frontier.inc.h.  It reads the ground field's type and dist_sq planes and
 * writes nothing of the map, of that field, of the ground navigation function or of the frontier clusters; its one plane is allocated
 * at the first call, the per-source planes of the global form when a field beyond the LDS budget first asks for them.
 *   k_glos_prep    (gie_ground_los.inc.h) on this section's own plane blk0 = ~traversable, padding bits beyond X SET: one launch in
 *                  front of the searches; no result is kept, a call sees the field as it stands where it is enqueued.  Ground NF1's
 *                  blk is not this one: after a propagation it means "blocked or visited", and the field of the robot's plan has to
 *                  survive the matrix.
 *   k_gcostmat     grid = n workgroups of 1024 threads: workgroup i is the whole search from point i, k_gnf1_bfs's level loop on
 *                  three bit planes without the field.  Threads t < n map point t to its cell (gie_ground_query's mapping) and test
 *                  its bit in blk0: word, bit and valid of every point lie in static LDS.  An invalid source writes its row of -1
 *                  and leaves (workgroup-uniform).  A valid one copies blk0 into B, sets its own bit in F and B, and runs
 *                    next = (F | F << 1 | F >> 1 | carries of the words left and right | the words of rows y - 1, y + 1) & ~B
 *                  into NX, B |= next by the word's owner, a wave vote into the s_any ring, ONE workgroup barrier, F and NX swap.
 *                  After the swap the new F is read-only until the next barrier: there thread t < n tests its target's bit, and a
 *                  target first seen in the frontier of level L + 1 gets cost[i][t] = L + 1.  "Some target is still missing" is a
 *                  wave vote of those threads into a second ring, s_left, read behind the NEXT level's barrier: the search stops
 *                  one level after its last valid target was found, with no barrier of its own.  It also stops when a level adds
 *                  nothing (the unreached targets stay at -1), and unconditionally after X * Y levels.
 *                  LDS = true: the three planes in dynamic LDS (GIE_GNF1_LDS_BYTES, 6144 words a plane: one workgroup per compute
 *                  unit, so 256 sources occupy the chip once; more would queue, nothing waits on another workgroup).
 *                  LDS = false (fields beyond that): F and B of source i in global memory, a pair of planes PER SOURCE; NX stays
 *                  in LDS and F <- NX is a copy behind a second barrier, as in k_gnf1_bfs<false>.  The host picks the form by the
 *                  size alone.
 * Only integers, no atomics, a row is written by one workgroup only: a result is bit-identical from run to run.  No grid barrier, no
 * cooperative residency: the launch is no member of the chain of grid-barrier launches and has no timeout path.
 * The compiler's figures and the times are in DESIGN.md 23.
 */

static_assert(GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE == GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE, "k_glos_prep takes this section's flag as it is");
static_assert(GIE_GROUND_COSTMAT_MAX_POINTS <= GIE_GNF1_THREADS, "a thread per point");

struct gie_gcm_dev {
    const uint64_t *blk0;   /* W words per row y: blocked */
    uint64_t *planes;       /* the global form: F, then B, of source i at 2 * nwords * i (nullptr in the LDS form) */
    int W, nwords;
    int pvt[2];
};

template <bool LDS>
__global__ __launch_bounds__(GIE_GNF1_THREADS) void k_gcostmat(const gie_ctx c, const gie_gcm_dev s, const float *xy, const int n, int32_t *cost, uint8_t *valid)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_planes[];     /* next; in the LDS form the frontier and B behind it */
    __shared__ int s_wd[GIE_GROUND_COSTMAT_MAX_POINTS];        /* the word of point t's cell */
    __shared__ uint8_t s_bit[GIE_GROUND_COSTMAT_MAX_POINTS], s_ok[GIE_GROUND_COSTMAT_MAX_POINTS];
    __shared__ int s_any[3], s_left[3];                        /* s_any[L % 3]: some wave found a new bit in level L; s_left[L % 3]: a target was missing before level L */
    const int src = blockIdx.x, tid = threadIdx.x, W = s.W, X = c.X, Y = c.Y, nwords = s.nwords;
    uint64_t *NX = s_planes, *F = LDS ? s_planes + nwords : s.planes + 2 * (size_t)nwords * src, *B = F + nwords;
    if (tid < n) {                                              /* gie_ground_query's mapping of point tid to its cell */
        const int S[2] = { X, Y };
        int v[2] = { 0, 0 };
        bool in = true;
#pragma unroll
        for (int k = 0; k < 2; k++) {                           /* (gie_ground_cell_of, written out: profiles/r28_ground_helpers_times.txt, second state) */
            const float u = floorf(xy[2 * (size_t)tid + k] / c.voxel_width + 0.5f);    /* gie_pos2coord */
            if (!(u >= -1.0e9f && u <= 1.0e9f)) { in = false; continue; }             /* (NaN, inf, and what no int32 coordinate holds) */
            v[k] = (int)u - s.pvt[k];
            in &= v[k] >= 0 && v[k] < S[k];
        }
        const int wd = in ? v[1] * W + (v[0] >> 6) : 0, bit = v[0] & 63;
        s_wd[tid] = wd; s_bit[tid] = (uint8_t)bit;
        s_ok[tid] = (uint8_t)(in && !((s.blk0[wd] >> bit) & 1ull));
    }
    if (tid < 3) s_any[tid] = s_left[tid] = 0;
    __syncthreads();
    if (!s_ok[src]) {                                           /* (workgroup-uniform) an invalid point: its row, and nothing else */
        if (tid < n) cost[(size_t)src * n + tid] = -1;
        if (tid == 0 && valid) valid[src] = 0;
        return;
    }
    for (int wd = tid; wd < nwords; wd += GIE_GNF1_THREADS) { F[wd] = 0ull; B[wd] = s.blk0[wd]; }
    const int swd = s_wd[src], sbit = s_bit[src];
    bool pending = false;                                       /* thread t < n: target t is valid and not reached yet */
    if (tid < n) {
        const bool own = s_ok[tid] && s_wd[tid] == swd && s_bit[tid] == sbit;
        pending = s_ok[tid] && !own;
        cost[(size_t)src * n + tid] = own ? 0 : -1;
    }
    if (__any(pending) && (tid & 63) == 0) s_left[0] = 1;
    if (tid == 0 && valid) valid[src] = 1;
    __syncthreads();                                            /* the planes are filled */
    if (tid == 0) { F[swd] = 1ull << sbit; B[swd] |= 1ull << sbit; }
    __syncthreads();
    if (!s_left[0]) return;                                     /* (workgroup-uniform) no valid point on another cell: the row is complete */
    /* a thread's words are tid + 1024 k: word column and row of the first, and the step between two, without a division per word
     * (gie_ground_words and gie_ground_dilate4, written out: with them the global form measured above the parent's range,
     * profiles/r28_ground_helpers_times.txt, first state) */
    const int y0 = tid / W, tx0 = tid - y0 * W, dy = GIE_GNF1_THREADS / W, dtx = GIE_GNF1_THREADS - dy * W;
    const int max_levels = X * Y;                               /* no path is longer: the loop ends here whatever the planes hold */
#pragma unroll 1
    for (int level = 0; level < max_levels; level++) {
        if (tid == 0) s_any[(level + 1) % 3] = s_left[(level + 1) % 3] = 0;       /* (last read after the barrier of level - 2, next set in level + 1 / after this level's barrier) */
        int any = 0;
#pragma unroll 1
        for (int wd = tid, y = y0, tx = tx0; wd < nwords; wd += GIE_GNF1_THREADS) {
            const uint64_t f = F[wd];
            uint64_t d = f | (f << 1) | (f >> 1);
            if (tx > 0) d |= F[wd - 1] >> 63;
            if (tx < W - 1) d |= F[wd + 1] << 63;
            if (y > 0) d |= F[wd - W];
            if (y < Y - 1) d |= F[wd + W];
            const uint64_t bl = B[wd], nx = d & ~bl;            /* (B holds the padding bits beyond X; only its owner touches a word of it) */
            NX[wd] = nx;
            if (nx) { any = 1; B[wd] = bl | nx; }
            y += dy; tx += dtx;
            if (tx >= W) { tx -= W; y++; }
        }
        if (__any(any) && (tid & 63) == 0) s_any[level % 3] = 1;
        __syncthreads();                                        /* every read of F is done, next is complete */
        if (!s_any[level % 3]) break;                           /* (workgroup-uniform) nothing new: what is not reached stays at -1 */
        if (!s_left[level % 3]) break;                          /* (workgroup-uniform; set before this barrier, after the one before) every valid target has its cost */
        if (LDS) { uint64_t *t = F; F = NX; NX = t; }           /* next is the frontier now; the old frontier is written after the next barrier only */
        else {
            for (int wd = tid; wd < nwords; wd += GIE_GNF1_THREADS) F[wd] = NX[wd];
            __syncthreads();
        }
        if (pending && ((F[s_wd[tid]] >> s_bit[tid]) & 1ull)) { /* the frontier of level + 1 is read-only here */
            cost[(size_t)src * n + tid] = level + 1;
            pending = false;
        }
        if (__any(pending) && (tid & 63) == 0) s_left[(level + 1) % 3] = 1;     /* read behind the next level's barrier: one level late */
    }
}

/* ---- host side */
static int gie_gcm_check(gie_mapper *m, const char *who, const float *xy, int n, const gie_ground_nf1_param *p, const int32_t *cost)
{
    const int rc = gie_gnf1_check(m, who, false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->clearance_sq < 0) bad = "clearance_sq must be >= 0";
    else if (p->flags & ~GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE) bad = "unknown flags (GIE_GROUND_NF1_FROM_FRONTIERS has no meaning here)";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3] || p->reserved[4] || p->reserved[5]) bad = "reserved must be 0";
    else if (n < 0 || n > GIE_GROUND_COSTMAT_MAX_POINTS) bad = "0 <= n <= 256 points";
    else if (n > 0 && (!xy || !cost)) bad = "n > 0 without points or without a matrix";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_ground_costmat_compute_dev(gie_mapper *m, const float *d_xy, int n, const gie_ground_nf1_param *p, int32_t *d_cost, uint8_t *d_valid)
{
    const int rc = gie_gcm_check(m, "gie_ground_costmat_compute_dev", d_xy, n, p, d_cost); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev g = gie_ground_view(m, &c);
    const int nwords = g.W * c.Y;
    const bool lds = nwords <= GIE_GNF1_LDS_WORDS;              /* by the size alone (sides <= 1024: one plane is 128 KiB at most, next always fits the LDS) */
    static bool attr_done = false;
    const int ra = gie_ground_lds_limit(&attr_done, "gie_ground_costmat_compute_dev", reinterpret_cast<const void *>(&k_gcostmat<true>),
                                        reinterpret_cast<const void *>(&k_gcostmat<false>), GIE_GNF1_LDS_BYTES);
    if (ra) return ra;
    if (!m->gcm.blk0) {
        m->gcm.blk0 = gie_dalloc<uint64_t>(m, (size_t)nwords, false);
        if (!m->gcm.blk0) { gie_set_err("gie_ground_costmat_compute_dev: device allocation of the blocked plane failed"); return GIE_ERR_DEVICE; }
    }
    if (!lds && n > m->gcm.planes_n) {                          /* the global form's planes grow with the largest n asked for */
        void *pl = be_alloc(&m->be, 2 * (size_t)nwords * n * sizeof(uint64_t), false);
        if (!pl) { gie_set_err("gie_ground_costmat_compute_dev: device allocation of the per-source planes failed"); return GIE_ERR_DEVICE; }
        if (m->gcm.planes) {
            for (void *&q : m->allocs) if (q == m->gcm.planes) q = pl;
            be_free(&m->be, m->gcm.planes);
        } else m->allocs.push_back(pl);
        m->gcm.planes = (uint64_t *)pl; m->gcm.planes_n = n;
    }
    gie_gcm_dev s;
    s.blk0 = m->gcm.blk0; s.planes = lds ? nullptr : m->gcm.planes; s.W = g.W; s.nwords = nwords; s.pvt[0] = g.pvt[0]; s.pvt[1] = g.pvt[1];
    be_prof(&m->be, GIE_K_GROUND_NF1, 0);
    GIE_LAUNCH(&m->be, k_glos_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, g, m->gcm.blk0, nwords, (int)p->clearance_sq, (int)p->flags);
    if (lds) GIE_LAUNCH(&m->be, k_gcostmat<true>, dim3(n), dim3(GIE_GNF1_THREADS), 3 * (size_t)nwords * sizeof(uint64_t), c, s, d_xy, n, d_cost, d_valid);
    else GIE_LAUNCH(&m->be, k_gcostmat<false>, dim3(n), dim3(GIE_GNF1_THREADS), (size_t)nwords * sizeof(uint64_t), c, s, d_xy, n, d_cost, d_valid);
    be_prof(&m->be, GIE_K_GROUND_NF1, 1);
    return GIE_OK;
}
extern "C" int gie_ground_costmat_compute(gie_mapper *m, const float *xy, int n, const gie_ground_nf1_param *p, int32_t *cost, uint8_t *valid)
{
    int rc = gie_gcm_check(m, "gie_ground_costmat_compute", xy, n, p, cost); if (rc) return rc;
    if (n == 0) return GIE_OK;
    const size_t cbytes = (size_t)n * n * 4;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_costmat_compute");
    char *dr = (char *)gie_scratch(m, 1, cbytes + (size_t)n, "gie_ground_costmat_compute");       /* the matrix, then valid */
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xy, (size_t)n * 8);
    rc = gie_ground_costmat_compute_dev(m, dx, n, p, (int32_t *)dr, (uint8_t *)(dr + cbytes)); if (rc) return rc;
    be_d2h(&m->be, cost, dr, cbytes);
    if (valid) be_d2h(&m->be, valid, dr + cbytes, (size_t)n);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_costmat.inc.h — the goal-to-goal cost matrix of the local volume (include/gie.h "cost matrix"): the BFS fields of up to 64
 * points in one bit-parallel pass.  HIP backend only: included by gie_hip.hip after gie_nf1.inc.h, whose traversable rule, point
 * mapping, tile lists with stamps and grid barrier it shares; nothing of the map update reads what is computed here.
 *
 * Scratch (gie_mapper::costmat), allocated at the first compute; no result is kept in it:
 *   m0, m1  one 64-bit mask per voxel each: bit i of seen_k(v) = "point i's search has reached v within k steps"; level k reads
 *           plane k & 1 and writes plane (k + 1) & 1;
 *   trav    one bit per voxel, NF1's layout (rows of W = ceil(X/64) words);
 *   stamp, list, w   NF1's tile stamps, two tile lists and control words (tiles of 64 x 8 x 8 voxels), in a gie_nf1_dev so that
 *           NF1's tile helpers serve as they are.
 * Prep: k_costmat_prep builds trav and zeroes both planes; k_costmat_points (one wave, a lane per point) maps and tests the points,
 * writes `valid`, sets bit i at voxel(i) in both planes, initialises the matrix and lists the points' tiles for level 0.
 * Propagation (k_costmat_bfs): one persistent launch, a grid barrier per level.  In level k a listed tile computes, a wave per
 * tile and a lane per voxel of a row (gie_costmat_tile: three z slices of the tile in registers),
 *   seen_{k+1}(v) = seen_k(v) | OR over the six neighbours u of seen_k(u)      for traversable v (0 elsewhere),
 * from plane k & 1 ONLY, and lists itself and its face neighbours for level k + 1 when a voxel changed.  The invariant that makes
 * two planes enough: at the start of level k, plane k & 1 holds seen_k and the other plane seen_{k-1} EVERYWHERE (seen_{-1} =
 * seen_0) — a tile that is not listed in level k had no change in itself or its face neighbours in level k - 1, so its
 * seen_{k+1} = seen_k = seen_{k-1}, which is what its words of plane (k + 1) & 1 hold already.
 * Recording: at the top of level k (after level k - 1's barrier) the first wave of every workgroup reads the <= 64 point voxels
 * from plane k & 1, a lane per point j, against the lane's copy of level k - 1's mask: bit i new at voxel(j) means
 * cost[i][j] = k (workgroup 0 writes it).  Every workgroup sees the same masks, so all take the same decision to leave early once
 * every valid point's voxel holds the mask of all valid points; otherwise the kernel leaves when a level's list is empty.  A
 * bit's level of arrival does not depend on when the kernel leaves, so the matrix is the same with and without the early exit.
 */

enum { GIE_CM_W_LEN = 0,        /* [0..2]: list lengths, level k's in w[k % 3] (NF1's scheme) */
       GIE_CM_W_BAR = 4,        /* grid-barrier word of k_costmat_bfs */
       GIE_CM_W_ALL = 6,        /* [6..7]: the 64-bit mask of the valid points (8-byte aligned) */
       GIE_CM_W_VOX = 8,        /* [8..71]: the local linear index of point j's voxel, -1 for an invalid point */
       GIE_CM_NWORDS = 72 };    /* (cleared with the stamps by one memset per compute) */
#define GIE_CM_BFS_THREADS 512         /* (three slices of a tile in registers: 166 VGPRs, two waves per SIMD) */

struct gie_costmat_dev {
    gie_nf1_dev t;              /* W, TY, TZ, ntiles, trav, stamp, list, w; the field and the other bit planes are not used */
    uint64_t *m0, *m1;
};

/* prep (a): one lane per voxel, a wave per 64-voxel word: the traversable plane; both mask planes at 0 */
__global__ __launch_bounds__(256) void k_costmat_prep(const gie_ctx c, const gie_costmat_dev s, const int nwords, const float clearance, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const int row = wd / s.t.W, x = (wd - row * s.t.W) * 64 + lane;
    bool tr = false;
    if (x < c.X) {
        const int id = row * c.X + x;
        tr = gie_nf1_traversable(c, id, c.glb_type[id], clearance, flags);
        s.m0[id] = 0; s.m1[id] = 0;
    }
    const uint64_t bt = __ballot(tr);
    if (lane == 0) s.t.trav[wd] = bt;
}

/* prep (b): ONE wave, a lane per point: voxel, validity, the point's bit in both planes; then the matrix at its initial values
 * (0 where two valid points share a voxel, the diagonal included; -1 elsewhere) and the tiles of level 0 */
__global__ __launch_bounds__(64) void k_costmat_points(const gie_ctx c, const gie_costmat_dev s, const float *xyz, const int n, int32_t *cost, uint8_t *valid)
{
    __shared__ int s_id[64];
    const int j = threadIdx.x;
    int id = -1;
    if (j < n) {
        int v[3];
        if (gie_nf1_voxel(c, c.pvt[0], c.pvt[1], c.pvt[2], xyz + 3 * (size_t)j, v)) {
            const size_t row = (size_t)v[2] * c.Y + v[1];
            if ((s.t.trav[row * s.t.W + (v[0] >> 6)] >> (v[0] & 63)) & 1ull) id = (int)(row * c.X + v[0]);
        }
        if (valid) valid[j] = id >= 0 ? 1 : 0;
    }
    s_id[j] = id;
    s.t.w[GIE_CM_W_VOX + j] = id;
    if (id >= 0) {
        atomicOr((unsigned long long *)&s.m0[id], 1ull << j);
        atomicOr((unsigned long long *)&s.m1[id], 1ull << j);
    }
    const uint64_t all = __ballot(id >= 0);
    if (j == 0) *(uint64_t *)&s.t.w[GIE_CM_W_ALL] = all;
    __syncthreads();
    for (int e = j; e < n * n; e += 64) {
        const int a = s_id[e / n], b = s_id[e % n];
        cost[e] = (a >= 0 && a == b) ? 0 : -1;
    }
    for (int p = 0; p < n; p++) {                               /* wave-uniform */
        const int q = s_id[p];
        if (q < 0) continue;
        const int x = q % c.X, r = q / c.X, y = r % c.Y, z = r / c.Y;
        gie_nf1_enqueue(s.t, ((z >> 3) * s.t.TY + (y >> 3)) * s.t.W + (x >> 6), 1, s.t.list, &s.t.w[GIE_CM_W_LEN]);
    }
}

/* slice z of tile column (tx, y0), in two phases so that the loads of a phase are in flight together (a load whose lanes depend
 * on a word loaded just before it would wait for that word, row after row):
 *   gie_costmat_slice_trav   the trav words T of its 8 rows, 0 for rows outside the volume;
 *   gie_costmat_slice_masks  the masks S, loaded only where the row's trav bit is set: the other voxels hold 0 in both planes
 *                            (trav has no bits beyond X, so no lane reads past a row's end). */
GIE_DEV void gie_costmat_slice_trav(const gie_ctx &c, const gie_costmat_dev &s, const int tx, const int y0, const int z, uint64_t (&T)[8])
{
#pragma unroll
    for (int r = 0; r < 8; r++) {
        T[r] = 0;
        if (z >= 0 && z < c.Z && y0 + r < c.Y) T[r] = s.t.trav[((size_t)z * c.Y + y0 + r) * s.t.W + tx];     /* wave-uniform */
    }
}
GIE_DEV void gie_costmat_slice_masks(const gie_ctx &c, const uint64_t *mk, const int tx, const int y0, const int z, const int lane,
                                     const uint64_t (&T)[8], uint64_t (&S)[8])
{
#pragma unroll
    for (int r = 0; r < 8; r++) {
        S[r] = 0;
        if ((T[r] >> lane) & 1ull) S[r] = gie_ld(&mk[((size_t)z * c.Y + y0 + r) * c.X + tx * 64 + lane]);
    }
}
/* one level of tile t, all lanes of a wave, lane = x within the word: slice after slice in z with the slices z - 1, z and z + 1 in
 * registers, so that every row of the tile and of its four face halos in y and z is loaded once (96 row loads for 64 rows; the x
 * neighbours come from the lanes beside, the two across the word's ends from a two-lane load per row).  Halo rows and end voxels
 * are loaded whatever their trav bits say (they hold 0 where it is clear).  true when a voxel changed. */
GIE_DEV bool gie_costmat_tile(const gie_ctx &c, const gie_costmat_dev &s, const uint64_t *mk, uint64_t *mn, const int t, const int lane)
{
    int tx, ty, tz;
    gie_nf1_tile(s.t, t, tx, ty, tz);
    const int X = c.X, Y = c.Y, Z = c.Z, y0 = ty * 8, z0 = tz * 8, x = tx * 64 + lane;
    const int nz = Z - z0 < 8 ? Z - z0 : 8;
    const bool inx = x < X;
    const bool edge = lane == 0 ? tx > 0 : (lane == 63 && x + 1 < X);      /* this lane fetches the voxel across the word's end */
    const int estep = lane == 0 ? -1 : 1;
    uint64_t A[8], B[8], Cn[8], tA[8], tB[8], tC[8];
    gie_costmat_slice_trav(c, s, tx, y0, z0 - 1, tA);
    gie_costmat_slice_trav(c, s, tx, y0, z0, tB);
    gie_costmat_slice_masks(c, mk, tx, y0, z0 - 1, lane, tA, A);
    gie_costmat_slice_masks(c, mk, tx, y0, z0, lane, tB, B);
    bool changed = false;
#pragma unroll 1
    for (int zi = 0; zi < nz; zi++) {
        const int z = z0 + zi;
        gie_costmat_slice_trav(c, s, tx, y0, z + 1, tC);
        uint64_t hm = 0, hp = 0, E[8];
        if (y0 > 0 && inx) hm = gie_ld(&mk[((size_t)z * Y + y0 - 1) * X + x]);
        if (y0 + 8 < Y && inx) hp = gie_ld(&mk[((size_t)z * Y + y0 + 8) * X + x]);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            E[r] = 0;
            if (tB[r] != 0 && edge) E[r] = gie_ld(&mk[((size_t)z * Y + y0 + r) * X + x + estep]);      /* (tB: 0 for rows outside the volume) */
        }
        gie_costmat_slice_masks(c, mk, tx, y0, z + 1, lane, tC, Cn);
        /* all eight rows are combined before the first store: a store between two rows would make the next row's first use of a
         * loaded register wait for that store's completion too (loads and stores share one in-order counter) */
        uint64_t U[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint64_t m = B[r];
            uint64_t u = m | A[r] | Cn[r] | (r > 0 ? B[r > 0 ? r - 1 : 0] : hm) | (r < 7 ? B[r < 7 ? r + 1 : 7] : hp) | E[r];
            const uint64_t lo = __shfl_up((unsigned long long)m, 1), hi = __shfl_down((unsigned long long)m, 1);
            if (lane > 0) u |= lo;
            if (lane < 63) u |= hi;
            U[r] = ((tB[r] >> lane) & 1ull) ? u : 0;           /* (the other voxels stay 0) */
            changed |= U[r] != m;
        }
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if ((tB[r] >> lane) & 1ull) gie_st(&mn[((size_t)z * Y + y0 + r) * X + x], U[r]);      /* (no lane of a row outside the volume) */
        }
#pragma unroll
        for (int r = 0; r < 8; r++) { A[r] = B[r]; B[r] = Cn[r]; tB[r] = tC[r]; }
    }
    return changed;
}

/* the propagation: one persistent launch, all workgroups co-resident (grid <= gie_config.wave_workgroups), a round per BFS level */
__global__ __launch_bounds__(GIE_CM_BFS_THREADS) void k_costmat_bfs(const gie_ctx c, const gie_costmat_dev s, const int n, int32_t *cost)
{
    __shared__ int s_fail, s_done;
    if (threadIdx.x == 0) { s_fail = 0; s_done = 0; }
    __syncthreads();
    constexpr int WAVES = GIE_CM_BFS_THREADS / 64;
    const int lane = threadIdx.x & 63, gw = blockIdx.x * WAVES + (int)(threadIdx.x >> 6), nw = gridDim.x * WAVES;
    /* the recording wave: lane j keeps voxel(j) and its mask of the level before */
    const bool rec = threadIdx.x < 64;
    int pv = -1;
    uint64_t prev = 0, all = 0;
    if (rec) {
        all = *(const uint64_t *)&s.t.w[GIE_CM_W_ALL];
        if (lane < n) pv = s.t.w[GIE_CM_W_VOX + lane];
        if (pv >= 0) prev = gie_ld(&s.m0[pv]);
    }
    uint32_t epoch = 0;
#pragma unroll 1
    for (int k = 0;; k++) {
        const uint64_t *mk = (k & 1) ? s.m1 : s.m0;
        uint64_t *mn = (k & 1) ? s.m0 : s.m1;
        if (rec) {                                              /* wave-uniform */
            const uint64_t cur = pv >= 0 ? gie_ld(&mk[pv]) : 0;
            if (blockIdx.x == 0)
                for (uint64_t b = cur & ~prev; b; b &= b - 1) cost[(size_t)__builtin_ctzll(b) * n + lane] = k;
            prev = cur;
            const bool done = __all(pv < 0 || cur == all);
            if (lane == 0) s_done = done ? 1 : 0;
        }
        __syncthreads();
        const int nt = gie_ld(&s.t.w[GIE_CM_W_LEN + k % 3]);  /* (the same in every workgroup: appended before the last barrier) */
        if (nt == 0 || s_done) break;
        if (blockIdx.x == 0 && threadIdx.x == 0) gie_st(&s.t.w[GIE_CM_W_LEN + (k + 2) % 3], 0);   /* (last read in round k - 1) */
        const int32_t *list = s.t.list + (size_t)(k & 1) * s.t.ntiles;
        int32_t *next = s.t.list + (size_t)((k + 1) & 1) * s.t.ntiles;
        int32_t *next_len = &s.t.w[GIE_CM_W_LEN + (k + 1) % 3];
#pragma unroll 1
        for (int i = gw; i < nt; i += nw) {                     /* wave-uniform */
            const int t = __builtin_amdgcn_readfirstlane(gie_ld(&list[i]));      /* (in scalar registers: the tile's trav words follow) */
            const bool changed = gie_costmat_tile(c, s, mk, mn, t, lane);
            if (__any(changed)) gie_nf1_enqueue(s.t, t, k + 2, next, next_len);
        }
        if (!gie_nf1_sync(c, &s.t.w[GIE_CM_W_BAR], epoch, &s_fail, GIE_ERRF_COSTMAT_BARRIER)) break;
    }
}

/* ---- host side */
static gie_costmat_dev gie_costmat_view(const gie_mapper *m)
{
    const gie_ctx &c = m->c;
    gie_costmat_dev s = {};
    s.t.W = (c.X + 63) / 64; s.t.TY = (c.Y + 7) / 8; s.t.TZ = (c.Z + 7) / 8; s.t.ntiles = s.t.W * s.t.TY * s.t.TZ;
    s.t.trav = m->costmat.trav;
    s.t.w = m->costmat.words; s.t.stamp = s.t.w + GIE_CM_NWORDS; s.t.list = s.t.stamp + s.t.ntiles;
    s.m0 = m->costmat.masks; s.m1 = s.m0 + (size_t)c.N;
    return s;
}

extern "C" int gie_costmat_compute_dev(gie_mapper *m, const float *d_xyz, int n, const gie_nf1_param *p, int32_t *d_cost, uint8_t *d_valid)
{
    int rc = gie_nf1_check(m, "gie_costmat_compute_dev", false); if (rc) return rc;
    if (!p || n < 0 || n > GIE_COSTMAT_MAX_POINTS || (n > 0 && (!d_xyz || !d_cost))) { gie_set_err("gie_costmat_compute_dev: bad arguments (0 <= n <= 64 points, a param and a matrix)"); return GIE_ERR_INVALID; }
    if (!(p->clearance >= 0.f && p->clearance <= 3.402823466e38f)) { gie_set_err("gie_costmat_compute_dev: clearance must be finite and >= 0"); return GIE_ERR_INVALID; }
    if (p->flags & ~GIE_NF1_UNKNOWN_TRAVERSABLE) { gie_set_err("gie_costmat_compute_dev: unknown flags (GIE_NF1_FROM_FRONTIERS has no meaning here)"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this matrix) */
    const int W = (c.X + 63) / 64, nwords = W * c.Y * c.Z, ntiles = W * ((c.Y + 7) / 8) * ((c.Z + 7) / 8);
    if (!m->costmat.masks) {
        uint64_t *masks = gie_dalloc<uint64_t>(m, 2 * (size_t)c.N, false);
        uint64_t *trav = masks ? gie_dalloc<uint64_t>(m, (size_t)nwords, false) : nullptr;
        int32_t *words = trav ? gie_dalloc<int32_t>(m, GIE_CM_NWORDS + 3 * (size_t)ntiles, false) : nullptr;
        if (!words) { gie_set_err("gie_costmat_compute_dev: device allocation of the cost matrix's scratch failed"); return GIE_ERR_DEVICE; }
        m->costmat.masks = masks; m->costmat.trav = trav; m->costmat.words = words;
    }
    const gie_costmat_dev s = gie_costmat_view(m);
    be_memset(&m->be, s.t.w, 0, (GIE_CM_NWORDS + (size_t)ntiles) * sizeof(int32_t));   /* control words and stamps */
    GIE_LAUNCH(&m->be, k_costmat_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, s, nwords, p->clearance, (int)p->flags);
    GIE_LAUNCH(&m->be, k_costmat_points, dim3(1), dim3(64), 0, c, s, d_xyz, n, d_cost, d_valid);
    /* a grid-barrier launch: it joins the device's chain of such launches (be_chained), as NF1's propagation does */
    be_chained(&m->be, [&]() { GIE_LAUNCH(&m->be, k_costmat_bfs, dim3(m->be.num_cu), dim3(GIE_CM_BFS_THREADS), 0, c, s, n, d_cost); });
    return GIE_OK;
}
extern "C" int gie_costmat_compute(gie_mapper *m, const float *xyz, int n, const gie_nf1_param *p, int32_t *cost, uint8_t *valid)
{
    int rc = gie_nf1_check(m, "gie_costmat_compute", false); if (rc) return rc;
    if (n < 0 || n > GIE_COSTMAT_MAX_POINTS || (n > 0 && (!xyz || !cost))) { gie_set_err("gie_costmat_compute: bad arguments (0 <= n <= 64 points and a matrix)"); return GIE_ERR_INVALID; }
    float *dx = nullptr;
    char *dr = nullptr;
    const size_t cbytes = (size_t)n * n * 4;
    if (n > 0) {
        dx = (float *)gie_scratch(m, 0, (size_t)n * 12, "gie_costmat_compute");
        dr = (char *)gie_scratch(m, 1, cbytes + (size_t)n, "gie_costmat_compute");     /* the matrix, then valid */
        if (!dx || !dr) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dx, xyz, (size_t)n * 12);
    }
    rc = gie_costmat_compute_dev(m, dx, n, p, (int32_t *)dr, dr ? (uint8_t *)(dr + cbytes) : nullptr); if (rc) return rc;
    if (n > 0) {
        be_d2h(&m->be, cost, dr, cbytes);
        if (valid) be_d2h(&m->be, valid, dr + cbytes, (size_t)n);
        gie_scratch_trim(m);
    }
    return gie_sync(m);
}

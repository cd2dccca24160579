/*
 * gie_ground.inc.h — the ground costmap: the footprint of a height band of the local volume and its exact 2-D distance transform
 * (include/gie.h "ground costmap").
 * HIP backend only: included by gie_hip.hip after gie_cloud.inc.h.  It reads the type plane and writes nothing of the map; its own
 * planes are per CELL (x, y) and are allocated at the first compute.
 *   k_ground_project   the only kernel that touches the volume: every cell's column over the band, reduced in registers (any
 *                      OCCUPIED, the number of known voxels, any FNT, the highest OCCUPIED z) into the cell's type, its top and
 *                      one bit row of obstacle columns per y (ceil(X/64) words, gie_sdf_pad's layout: padding bits are 0).  Lanes
 *                      run along x.  X % 16 == 0: a lane holds 16 cells behind one 16-byte load per layer, four lanes a word
 *                      (k_sdf_occ16's form), and the four waves of a workgroup take a quarter of the band each for the same 1024
 *                      cells and meet in LDS (OR, sum, max; 26 KB), no second pass over anything — with a lane's whole column in
 *                      one wave, 512 x 512 cells were 256 waves, one per compute unit with its loads one behind the other, and a
 *                      tall band ran at a sixth of the type plane's stream.  Otherwise a byte per lane, a wave
 *                      per word (k_sdf_occ's).  The four counts meet per
 *                      wave in one packed word, per workgroup in LDS: at most four atomics per workgroup.
 *   k_ground_line      pass X and pass Y of the separable transform, one wave per x.  A site of the line is a row y with an
 *                      obstacle column: its value the squared distance from x to the nearest set bit of that row (a scan of the
 *                      bit row, not stored), its closest x carried beside it; the lower envelope over the rows
 *                      (gie_row_compact_push, gie_row_argmin) gives dist_sq, the winning row coc_y, its carried x coc_x.  With no
 *                      obstacle column (the counts say so on the device) it returns at once and the readers write -1.
 *                      Keys of the envelope are ((u - i)² + a) << 10 | rank: a + Y² < X² + Y² < 2^22 for every size gie_create accepts.
 *   exports            one lane per cell (k_lin) or point (k_ground_query).
 * A compute is one memset of the counters and these two launches: no grid barrier, no loop whose trip count depends on device data
 * but the scans of a bit row.  The compiler's figures and the times are in DESIGN.md 18.
 */

#define GIE_GROUND_NONE INT32_MIN       /* top of a column that is not OCCUPIED */

struct gie_ground_dev {
    uint64_t *obs;          /* W words per row y: the obstacle columns */
    int8_t *type;           /* X * Y */
    int32_t *top, *dist;    /* X * Y: GLOBAL z; dist_sq (written only when there is an obstacle column) */
    int32_t *coc;           /* X * Y: local x | local y << 16 of the closest obstacle column (as dist) */
    int32_t *cnt;           /* the four counts, GIE_VOX_* order */
    int W, flags;
    int pvt[3];             /* the field's pivot */
};
/* the number of obstacle columns of the field (0: dist and coc hold nothing) */
GIE_DEV int gie_ground_nobs(const gie_ground_dev &s)
{
    const volatile int32_t *n = s.cnt;
    return n[GIE_VOX_OCCUPIED] + ((s.flags & GIE_GROUND_UNKNOWN_BLOCKS) ? n[GIE_VOX_UNKNOWN] : 0);
}
/* THE cell of a point (metres) for every ground entry: gie_pos2coord less the field's pivot; false outside the rectangle and for a
 * coordinate that is NaN, inf or beyond what an int32 holds (v[k] = 0 there; outside the rectangle v holds the cell all the same).
 * Five kernels spell the same loop out.  k_ground_query, k_gnf1_goals, k_gnf1_path, k_gnf1_query: the compiler makes the function
 * branch-free, which costs those four 3 to 5 registers (profiles/r28_ground_helpers_kernels.txt).  k_gcostmat: with the function one
 * of its times lay above the parent's range (profiles/r28_ground_helpers_times.txt).  tests/test_ground_gpu.py holds all of them and
 * the callers of this function to one table of points */
GIE_DEV bool gie_ground_cell_of(const float w, const int X, const int Y, const int *pvt, const float *xy, int v[2])
{
    const int S[2] = { X, Y };
    int r[2] = { 0, 0 };
    bool in = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float u = floorf(xy[k] / w + 0.5f);               /* gie_pos2coord */
        if (!(u >= -1.0e9f && u <= 1.0e9f)) { in = false; continue; }
        r[k] = (int)u - pvt[k];
        in &= r[k] >= 0 && r[k] < S[k];
    }
    v[0] = r[0]; v[1] = r[1];
    return in;
}
/* a robot may stand on cell id: FREE or FNT (UNKNOWN too with unknown_ok), and no obstacle column nearer than clearance_sq */
GIE_DEV bool gie_ground_traversable(const gie_ground_dev &g, const int id, const bool none, const int clearance_sq, const int unknown_ok)
{
    const int8_t ty = g.type[id];
    const bool open = ty == GIE_VOX_FREE || ty == GIE_VOX_FNT || (ty == GIE_VOX_UNKNOWN && unknown_ok);
    return open && (none || g.dist[id] >= clearance_sq);
}
/* the 4-neighbour dilation of word wd (word column tx, row y) of a bit plane of W words a row and Y rows */
GIE_DEV uint64_t gie_ground_dilate4(const uint64_t *F, const int wd, const int tx, const int y, const int W, const int Y)
{
    const uint64_t f = F[wd];
    uint64_t d = f | (f << 1) | (f >> 1);
    if (tx > 0) d |= F[wd - 1] >> 63;
    if (tx < W - 1) d |= F[wd + 1] << 63;
    if (y > 0) d |= F[wd - W];
    if (y < Y - 1) d |= F[wd + W];
    return d;
}
/* thread tid of T owns the words tid + T k of such a plane: word column and row of the first, and the step between two, without a
 * division per word */
struct gie_ground_words { int y, tx, dy, dtx; };
GIE_DEV gie_ground_words gie_ground_words_first(const int tid, const int T, const int W)
{
    gie_ground_words t;
    t.y = tid / W; t.tx = tid - t.y * W; t.dy = T / W; t.dtx = T - t.dy * W;
    return t;
}
GIE_DEV void gie_ground_words_next(gie_ground_words &t, const int W)
{
    t.y += t.dy; t.tx += t.dtx;
    if (t.tx >= W) { t.tx -= W; t.y++; }
}

/* one voxel of a column into its reduction: bit k of occ / fnt, the count of known voxels, the highest occupied layer */
GIE_DEV void gie_ground_voxel(const uint32_t ty, const int k, const int gz, uint32_t &occ, uint32_t &fnt, int &known, int &top)
{
    occ |= (uint32_t)(ty == GIE_VOX_OCCUPIED) << k;
    fnt |= (uint32_t)(ty == GIE_VOX_FNT) << k;
    known += (ty - 1u) < 3u;
    top = ty == GIE_VOX_OCCUPIED ? gz : top;                    /* (layers come in rising order) */
}
GIE_DEV int gie_ground_type(const bool occ, const bool fnt, const int known, const int min_known)
{
    return occ ? GIE_VOX_OCCUPIED : (known < min_known ? GIE_VOX_UNKNOWN : (fnt ? GIE_VOX_FNT : GIE_VOX_FREE));
}
/* a lane's counts (16-bit fields of `n`, type t in bits [16 t, 16 t + 16): a wave holds at most 1024 cells) into s.cnt: summed over
 * the wave, then over the workgroup's four waves in LDS; lane t adds type t's sum.  Called by all 256 lanes. */
GIE_DEV void gie_ground_count(unsigned long long n, int32_t *cnt)
{
    __shared__ unsigned long long s_n[4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x < 4) {
        const int sh = 16 * (int)threadIdx.x;
        const int v = (int)(((s_n[0] >> sh) & 0xffffu) + ((s_n[1] >> sh) & 0xffffu) + ((s_n[2] >> sh) & 0xffffu) + ((s_n[3] >> sh) & 0xffffu));
        if (v) atomicAdd(cnt + threadIdx.x, v);
    }
}

/* (a) the projection of the layers [z0, z1) (local z; the band, clipped by the host; z0 == z1: every column UNKNOWN) */
template <bool VEC>
__global__ __launch_bounds__(256) void k_ground_project(const gie_ctx c, const gie_ground_dev s, const int z0, const int z1, const int min_known, const int nwords)
{
    const size_t plane = (size_t)c.X * c.Y;
    const bool blocks = s.flags & GIE_GROUND_UNKNOWN_BLOCKS;
    unsigned long long n = 0;
    if (VEC) {                                                  /* 16 cells of one row per lane, four lanes per word; the band in four parts, one per wave */
        __shared__ int s_known[3][16][64], s_top[3][16][64];
        __shared__ uint32_t s_occ[3][64], s_fnt[3][64];
        const int part = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int g = blockIdx.x * 64 + lane, wd = g >> 2, q = g & 3;
        const int y = wd / s.W, x = (wd - y * s.W) * 64 + q * 16;
        const bool on = wd < nwords && x < c.X;
        const size_t cell = (size_t)y * c.X + x;
        const int per = (z1 - z0 + 3) >> 2, za = min(z0 + part * per, z1), zb = min(za + per, z1);
        uint32_t occ = 0, fnt = 0;
        int known[16], top[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { known[k] = 0; top[k] = GIE_GROUND_NONE; }
        if (on) {
            const int8_t *p = c.glb_type + za * plane + cell;
#pragma unroll 4
            for (int z = za; z < zb; z++, p += plane) {
                const uint4 t = *reinterpret_cast<const uint4 *>(p);
#pragma unroll
                for (int k = 0; k < 16; k++) gie_ground_voxel(gie_cloud_byte(t, k), k, z + s.pvt[2], occ, fnt, known[k], top[k]);
            }
        }
        if (part > 0) {
            s_occ[part - 1][lane] = occ; s_fnt[part - 1][lane] = fnt;
#pragma unroll
            for (int k = 0; k < 16; k++) { s_known[part - 1][k][lane] = known[k]; s_top[part - 1][k][lane] = top[k]; }
        }
        __syncthreads();
        if (part == 0) {                                        /* OR, sum and max over the parts (NONE is the least int) */
            uint64_t v = 0;
            if (on) {
#pragma unroll
                for (int w = 0; w < 3; w++) {
                    occ |= s_occ[w][lane]; fnt |= s_fnt[w][lane];
#pragma unroll
                    for (int k = 0; k < 16; k++) { known[k] += s_known[w][k][lane]; top[k] = max(top[k], s_top[w][k][lane]); }
                }
                uint32_t ty[4] = { 0, 0, 0, 0 }, m = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int t = gie_ground_type((occ >> k) & 1u, (fnt >> k) & 1u, known[k], min_known);
                    ty[k >> 2] |= (uint32_t)t << (8 * (k & 3));
                    m |= (uint32_t)(t == GIE_VOX_OCCUPIED || (blocks && t == GIE_VOX_UNKNOWN)) << k;
                    n += 1ull << (16 * t);
                }
                *reinterpret_cast<uint4 *>(s.type + cell) = make_uint4(ty[0], ty[1], ty[2], ty[3]);
#pragma unroll
                for (int k = 0; k < 16; k += 4) *reinterpret_cast<int4 *>(s.top + cell + k) = make_int4(top[k], top[k + 1], top[k + 2], top[k + 3]);
                v = (uint64_t)m << (16 * q);
            }
            v |= (uint64_t)__shfl_xor((unsigned long long)v, 1);
            v |= (uint64_t)__shfl_xor((unsigned long long)v, 2);
            if (q == 0 && wd < nwords) s.obs[wd] = v;
        }
    } else {                                                    /* a cell per lane, a wave per word */
        const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
        const int y = wd / s.W, x = (wd - y * s.W) * 64 + lane;
        const bool on = wd < nwords && x < c.X;
        bool obstacle = false;
        if (on) {
            uint32_t occ = 0, fnt = 0;
            int known = 0, top = GIE_GROUND_NONE;
            const size_t cell = (size_t)y * c.X + x;
            const int8_t *p = c.glb_type + z0 * plane + cell;
#pragma unroll 8
            for (int z = z0; z < z1; z++, p += plane) gie_ground_voxel((uint8_t)*p, 0, z + s.pvt[2], occ, fnt, known, top);
            const int t = gie_ground_type(occ, fnt, known, min_known);
            obstacle = t == GIE_VOX_OCCUPIED || (blocks && t == GIE_VOX_UNKNOWN);
            s.type[cell] = (int8_t)t;
            s.top[cell] = top;
            n = 1ull << (16 * t);
        }
        const unsigned long long b = __ballot(obstacle);
        if (lane == 0 && wd < nwords) s.obs[wd] = b;
    }
    gie_ground_count(n, s.cnt);
}

/* pass X: the x of the set bit of a bit row nearest to x (either of two equally near), -1 if the row has none */
GIE_DEV int gie_ground_near(const uint64_t *row, const int W, const int x)
{
    const int wx = x >> 6, b = x & 63;
    int r = -1, l = -1;
    uint64_t f = row[wx] & (~0ull << b);                        /* at or right of x */
    if (f) r = wx * 64 + __builtin_ctzll(f);
    else for (int k = wx + 1; k < W; k++) if ((f = row[k])) { r = k * 64 + __builtin_ctzll(f); break; }
    f = row[wx] & ((2ull << b) - 1ull);                         /* at or left of x (b = 63: 2 << 63 wraps to 0, all bits) */
    if (f) l = wx * 64 + 63 - __builtin_clzll(f);
    else for (int k = wx - 1; k >= 0; k--) if ((f = row[k])) { l = k * 64 + 63 - __builtin_clzll(f); break; }
    if (l < 0 || r < 0) return l < 0 ? r : l;
    return x - l <= r - x ? l : r;
}

/* (b) + (c): one wave per line along y at x; the first lanes of the grid hand the counts to a _dev caller */
template <int CP>
__global__ __launch_bounds__(64 * GIE_SDF_WAVES) void k_ground_line(const gie_ctx c, const gie_ground_dev s, int32_t *counts)
{
    if (counts && blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = s.cnt[threadIdx.x];
    if (gie_ground_nobs(s) == 0) return;                        /* no obstacle column: the readers write -1 */
    constexpr int LP = 64 * CP;
    __shared__ __attribute__((aligned(16))) uint2 s_ce[GIE_SDF_WAVES][LP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, W = s.W, X = c.X, Y = c.Y;
    uint2 *ce = s_ce[wave];
    const int u0 = lane * CP;
#pragma unroll 1
    for (int x = blockIdx.x * GIE_SDF_WAVES + wave; x < X; x += gridDim.x * GIE_SDF_WAVES) {
        gie_wave_sync();                                        /* (the wave's site list is reused line after line) */
        int K = 0;
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int i = 64 * m + lane;
            const int nx = i < Y ? gie_ground_near(s.obs + (size_t)i * W, W, x) : -1;
            const int dx = nx - x;
            if (64 * m < Y) K = gie_row_compact_push(ce, K, nx >= 0, (uint32_t)(dx * dx), i, (uint32_t)nx, lane);
        }
        gie_wave_sync();
        int sj[CP];
        gie_row_argmin<CP>(ce, K, Y, lane, sj);                 /* K > 0: some row holds an obstacle column, and every line sees it */
#pragma unroll
        for (int m = 0; m < CP; m++) {
            const int u = u0 + m;
            if (u >= Y) break;
            const uint2 e = ce[sj[m]];
            const int i = (int)((e.y & 0xffffu) >> 5), du = u - i;
            s.dist[(size_t)u * X + x] = du * du + (int)(e.x >> 10);
            s.coc[(size_t)u * X + x] = (int)(e.y >> 16) | (i << 16);
        }
    }
}

/* the record of cell i of the field */
GIE_DEV gie_ground_cell gie_ground_record(const gie_ground_dev &s, const int i, const bool none)
{
    gie_ground_cell r;
    r.dist_sq = none ? -1 : s.dist[i];
    r.coc_x = r.coc_y = GIE_EMPTY_VALUE;
    if (!none) { const int pc = s.coc[i]; r.coc_x = (pc & 0xffff) + s.pvt[0]; r.coc_y = (pc >> 16) + s.pvt[1]; }
    r.type = s.type[i]; r.inside = 1; r.pad[0] = r.pad[1] = 0;
    return r;
}
/* gie_read_ground: one lane per cell */
struct op_ground_export {
    gie_ground_dev s; int8_t *type; int32_t *dist, *coc_xy, *top;
    GIE_DEVM void operator()(const gie_ctx &, int i) const {
        const gie_ground_cell r = gie_ground_record(s, i, gie_ground_nobs(s) == 0);
        if (type) type[i] = r.type;
        if (dist) dist[i] = r.dist_sq;
        if (coc_xy) { coc_xy[2 * (size_t)i] = r.coc_x; coc_xy[2 * (size_t)i + 1] = r.coc_y; }
        if (top) top[i] = s.top[i];
    }
};
/* gie_read_costmap_ground: the one-layer TYPE_EDT payload */
struct op_ground_costmap {
    gie_ground_dev s; gie_seendist *out;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        gie_seendist sd;
        sd.d = gie_ground_nobs(s) == 0 ? (float)c.max_loc_dist_sq : sqrtf((float)s.dist[i]);
        sd.s = 0; sd.o = (uint8_t)(s.type[i] != GIE_VOX_UNKNOWN); sd.pad[0] = sd.pad[1] = 0;
        out[i] = sd;
    }
};
/* gie_ground_query: one lane per point */
__global__ __launch_bounds__(256) void k_ground_query(const gie_ctx c, const gie_ground_dev s, const float *xy, const int n, gie_ground_cell *out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int S[2] = { c.X, c.Y };
    int v[2];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {                               /* gie_ground_cell_of, written out: through the function the kernel takes 18 registers for 13 */
        const float u = floorf(xy[2 * (size_t)p + k] / c.voxel_width + 0.5f);
        v[k] = 0;
        if (!(u >= -1.0e9f && u <= 1.0e9f)) { in = false; continue; }
        v[k] = (int)u - s.pvt[k];
        in &= v[k] >= 0 && v[k] < S[k];
    }
    gie_ground_cell r;
    if (in) r = gie_ground_record(s, v[1] * c.X + v[0], gie_ground_nobs(s) == 0);
    else { r.dist_sq = -1; r.coc_x = r.coc_y = GIE_EMPTY_VALUE; r.type = GIE_VOX_UNKNOWN; r.inside = 0; r.pad[0] = r.pad[1] = 0; }
    out[p] = r;
}

/* ---- host side */
/* what every ground entry asks first; `what` is the stage's noun for that which a tile's faces would cut */
static int gie_ground_check(gie_mapper *m, const char *who, bool need_field, const char *what = "field")
{
    static_assert(sizeof(gie_ground_param) == 32 && sizeof(gie_ground_cell) == 16, "the sizes include/gie.h states");
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) { gie_set_err(std::string(who) + ": not for a tiled mapper (its " + what + " would stop at the tile's faces)"); return GIE_ERR_INVALID; }
    if (need_field && !m->ground.valid) { gie_set_err(std::string(who) + ": no ground field yet (gie_ground_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* a kernel pair's dynamic LDS limit raised once (k1 may be null); `done` is the call site's own flag */
static int gie_ground_lds_limit(bool *done, const char *who, const void *k0, const void *k1, int bytes)
{
    if (*done) return GIE_OK;
    hipError_t e = hipFuncSetAttribute(k0, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && k1) e = hipFuncSetAttribute(k1, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { gie_set_err(std::string(who) + ": hipFuncSetAttribute: " + hipGetErrorString(e)); return GIE_ERR_DEVICE; }
    *done = true;
    return GIE_OK;
}
/* the field's view, with the mapper's context free of a halo round's gate (no business of this section) */
static gie_ground_dev gie_ground_view(const gie_mapper *m, gie_ctx *c)
{
    *c = m->c;
    c->gate = nullptr;
    const size_t cells = (size_t)c->X * c->Y;
    gie_ground_dev s;
    s.obs = m->ground.obs; s.type = m->ground.type;
    s.top = m->ground.cells; s.dist = s.top + cells; s.coc = s.dist + cells; s.cnt = m->ground.cnt;
    s.W = (c->X + 63) / 64; s.flags = m->ground.flags;
    for (int i = 0; i < 3; i++) s.pvt[i] = m->ground.pvt[i];
    return s;
}
template <int CP> static void be_ground_lines(be_state *b, const gie_ctx &c, const gie_ground_dev &s, int32_t *d_counts)
{
    GIE_LAUNCH(b, k_ground_line<CP>, dim3(std::min((c.X + GIE_SDF_WAVES - 1) / GIE_SDF_WAVES, b->cu_total * 16)), dim3(64 * GIE_SDF_WAVES), 0, c, s, d_counts);
}

extern "C" int gie_ground_compute_dev(gie_mapper *m, const gie_ground_param *p, int32_t *d_counts)
{
    int rc = gie_ground_check(m, "gie_ground_compute_dev", false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->z_lo > p->z_hi) bad = "z_lo > z_hi";
    else if (p->min_known < 1) bad = "min_known must be >= 1";
    else if (p->flags & ~GIE_GROUND_UNKNOWN_BLOCKS) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) bad = "reserved must be 0";
    else if (!m->has_pose) bad = "gie_set_pose has not been called";
    if (bad) { gie_set_err(std::string("gie_ground_compute_dev: ") + bad); return GIE_ERR_INVALID; }
    const int X = m->c.X, Y = m->c.Y, Z = m->c.Z, W = (X + 63) / 64, nwords = W * Y;
    if (!m->ground.obs) {
        uint64_t *obs = gie_dalloc<uint64_t>(m, (size_t)nwords, false);
        int32_t *cells = obs ? gie_dalloc<int32_t>(m, 3 * (size_t)X * Y, false) : nullptr;
        int8_t *type = cells ? gie_dalloc<int8_t>(m, (size_t)X * Y, false) : nullptr;
        int32_t *cnt = type ? gie_dalloc<int32_t>(m, 4, false) : nullptr;
        if (!cnt) { gie_set_err("gie_ground_compute_dev: device allocation of the ground field failed"); return GIE_ERR_DEVICE; }
        m->ground.obs = obs; m->ground.cells = cells; m->ground.type = type; m->ground.cnt = cnt;
    }
    m->ground.flags = p->flags; m->ground.z_lo = p->z_lo;
    for (int i = 0; i < 3; i++) { m->ground.pvt[i] = m->c.pvt[i]; m->ground.origin[i] = m->msg_origin[i]; }
    gie_ctx c;
    const gie_ground_dev s = gie_ground_view(m, &c);
    const long long lo = (long long)p->z_lo - c.pvt[2], hi = (long long)p->z_hi - c.pvt[2];      /* the band in local layers */
    int z0 = lo < 0 ? 0 : (int)(lo < Z ? lo : Z), z1 = hi >= Z ? Z : (int)(hi < 0 ? 0 : hi + 1);
    if (z0 >= z1) z0 = z1 = 0;
    be_prof(&m->be, GIE_K_GROUND, 0);
    be_memset(&m->be, s.cnt, 0, 4 * sizeof(int32_t));
    if ((X & 15) == 0 && ((uintptr_t)c.glb_type & 15) == 0) GIE_LAUNCH(&m->be, k_ground_project<true>, dim3((nwords + 15) / 16), dim3(256), 0, c, s, z0, z1, (int)p->min_known, nwords);
    else GIE_LAUNCH(&m->be, k_ground_project<false>, dim3((nwords + 3) / 4), dim3(256), 0, c, s, z0, z1, (int)p->min_known, nwords);
    if (Y <= 64) be_ground_lines<1>(&m->be, c, s, d_counts);
    else if (Y <= 128) be_ground_lines<2>(&m->be, c, s, d_counts);
    else if (Y <= 256) be_ground_lines<4>(&m->be, c, s, d_counts);
    else if (Y <= 512) be_ground_lines<8>(&m->be, c, s, d_counts);
    else be_ground_lines<16>(&m->be, c, s, d_counts);
    be_prof(&m->be, GIE_K_GROUND, 1);
    m->ground.valid = 1;
    m->gnf1.valid = 0;                                          /* (gie_ground_nf1.inc.h: its field was of the planes just overwritten) */
    m->gfr.valid = 0;                                           /* (gie_ground_frontier.inc.h: so were its clusters) */
    m->gpose.valid = 0;                                         /* (gie_ground_pose_nf1.inc.h: and its field) */
    m->gsdf.valid = 0;                                          /* (gie_ground_sdf.inc.h: and its inside distances) */
    return GIE_OK;
}
extern "C" int gie_ground_compute(gie_mapper *m, const gie_ground_param *p, int32_t counts[4])
{
    const int rc = gie_ground_compute_dev(m, p, nullptr); if (rc) return rc;
    if (counts) be_d2h(&m->be, counts, m->ground.cnt, 4 * sizeof(int32_t));
    return gie_sync(m);
}
extern "C" int gie_read_ground_dev(gie_mapper *m, int8_t *d_type, int32_t *d_dist_sq, int32_t *d_coc_xy, int32_t *d_top)
{
    const int rc = gie_ground_check(m, "gie_read_ground_dev", true); if (rc) return rc;
    if (!d_type && !d_dist_sq && !d_coc_xy && !d_top) { gie_set_err("gie_read_ground_dev: all four outputs are null"); return GIE_ERR_INVALID; }
    gie_ctx c;
    op_ground_export op; op.s = gie_ground_view(m, &c); op.type = d_type; op.dist = d_dist_sq; op.coc_xy = d_coc_xy; op.top = d_top;
    be_prof(&m->be, GIE_K_GROUND, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND, 1);
    return GIE_OK;
}
extern "C" int gie_read_ground(gie_mapper *m, int8_t *type, int32_t *dist_sq, int32_t *coc_xy, int32_t *top)
{
    int rc = gie_ground_check(m, "gie_read_ground", true); if (rc) return rc;
    if (!type && !dist_sq && !coc_xy && !top) { gie_set_err("gie_read_ground: all four outputs are null"); return GIE_ERR_INVALID; }
    /* one export buffer: the closest columns (8 bytes a cell), dist_sq and top (4 each), the types (1) */
    const size_t n = (size_t)m->c.X * m->c.Y;
    char *d = (char *)gie_scratch(m, 1, n * 17, "gie_read_ground");
    if (!d) return GIE_ERR_DEVICE;
    int32_t *dc = (int32_t *)d, *dd = dc + 2 * n, *dt = dd + n;
    int8_t *dy = (int8_t *)(dt + n);
    rc = gie_read_ground_dev(m, type ? dy : nullptr, dist_sq ? dd : nullptr, coc_xy ? dc : nullptr, top ? dt : nullptr); if (rc) return rc;
    if (type) be_d2h(&m->be, type, dy, n);
    if (dist_sq) be_d2h(&m->be, dist_sq, dd, n * 4);
    if (coc_xy) be_d2h(&m->be, coc_xy, dc, n * 8);
    if (top) be_d2h(&m->be, top, dt, n * 4);
    return gie_sync(m);
}
/* gie_read_costmap's header at the field's pivot: one layer, whose origin is the band's lower end as the caller gave it */
static void gie_ground_costmap_hdr(const gie_mapper *m, gie_costmap_hdr *hdr)
{
    gie_fill_costmap_hdr(m, hdr);
    hdr->z_size = 1;
    hdr->x_origin = m->ground.origin[0]; hdr->y_origin = m->ground.origin[1]; hdr->z_origin = (float)m->ground.z_lo * m->c.voxel_width;
}
extern "C" int gie_read_costmap_ground_dev(gie_mapper *m, gie_seendist *d_payload, gie_costmap_hdr *hdr)
{
    const int rc = gie_ground_check(m, "gie_read_costmap_ground_dev", true); if (rc) return rc;
    if (!d_payload) { gie_set_err("gie_read_costmap_ground_dev: null payload"); return GIE_ERR_INVALID; }
    gie_ctx c;
    op_ground_costmap op; op.s = gie_ground_view(m, &c); op.out = d_payload;
    be_prof(&m->be, GIE_K_GROUND, 0);
    be_lin(&m->be, c, op, c.X * c.Y);
    be_prof(&m->be, GIE_K_GROUND, 1);
    if (hdr) gie_ground_costmap_hdr(m, hdr);
    return GIE_OK;
}
extern "C" int gie_read_costmap_ground(gie_mapper *m, gie_seendist *payload, gie_costmap_hdr *hdr)
{
    int rc = gie_ground_check(m, "gie_read_costmap_ground", true); if (rc) return rc;
    if (payload) {
        const size_t n = (size_t)m->c.X * m->c.Y;
        gie_seendist *d = (gie_seendist *)gie_scratch(m, 1, n * sizeof(gie_seendist), "gie_read_costmap_ground");
        if (!d) return GIE_ERR_DEVICE;
        rc = gie_read_costmap_ground_dev(m, d, nullptr); if (rc) return rc;
        be_d2h(&m->be, payload, d, n * sizeof(gie_seendist));
    }
    if (hdr) gie_ground_costmap_hdr(m, hdr);
    return gie_sync(m);
}
extern "C" int gie_ground_query_dev(gie_mapper *m, const float *d_xy, int n, gie_ground_cell *d_out)
{
    const int rc = gie_ground_check(m, "gie_ground_query_dev", true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_xy || !d_out))) { gie_set_err("gie_ground_query_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    gie_ctx c;
    const gie_ground_dev s = gie_ground_view(m, &c);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 0);
    GIE_LAUNCH(&m->be, k_ground_query, dim3((n + 255) / 256), dim3(256), 0, c, s, d_xy, n, d_out);
    be_prof(&m->be, GIE_K_GROUND_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_ground_query(gie_mapper *m, const float *xy, int n, gie_ground_cell *out)
{
    int rc = gie_ground_check(m, "gie_ground_query", true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!xy || !out))) { gie_set_err("gie_ground_query: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 8, "gie_ground_query");
    gie_ground_cell *dr = (gie_ground_cell *)gie_scratch(m, 1, (size_t)n * sizeof(gie_ground_cell), "gie_ground_query");
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xy, (size_t)n * 8);
    rc = gie_ground_query_dev(m, dx, n, dr); if (rc) return rc;
    be_d2h(&m->be, out, dr, (size_t)n * sizeof(gie_ground_cell));
    gie_scratch_trim(m);
    return gie_sync(m);
}

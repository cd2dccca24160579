/*
 * gie_nf1.inc.h — the NF1 navigation function of the local volume and its descent paths (include/gie.h "navigation function").
 * HIP backend only: included by gie_hip.hip after gie_sdf.inc.h; nothing of the map update reads what is computed here.
 *
 * The cache (gie_mapper::nf1), allocated at the first compute:
 *   f      int32 per voxel: the field;
 *   trav   one bit per voxel, traversable: rows of W = ceil(X/64) 64-bit words, bit x & 63 of word x >> 6 (as the SDF's occ plane);
 *   known  same layout, type != UNKNOWN (the costmap's `o`, taken at compute time like the field);
 *   vis    same layout, voxels with a value;
 *   fr[2]  same layout, the BFS frontier of level k in fr[k & 1];
 *   stamp  int32 per tile of 64 x 8 x 8 voxels (one word of x by 8 rows by 8 slices): the last level + 1 whose list holds it;
 *   list   two lists of tiles (level k reads list[k & 1], appends to list[(k + 1) & 1]);
 *   w      GIE_NF1_NWORDS control words (list lengths, source count, grid barrier).
 * Prep (k_nf1_prep, k_nf1_goals, k_nf1_seed) builds the bit planes and the level-0 list.  The propagation (k_nf1_bfs) is one
 * persistent launch of level-synchronous rounds: in round k every listed tile dilates the level-k frontier into its own words,
 *   next = (fr_k | fr_k << 1 | fr_k >> 1 | carries | rows y +- 1 | rows z +- 1) & trav & ~vis,
 * one lane per row word, writes k + 1 at the new bits and lists itself and its six neighbour tiles for round k + 1 when any bit
 * is new; a grid barrier ends the round; the kernel leaves when a round's list is empty.  Every voxel gets its value in the round
 * of its BFS level, so the field does not depend on scheduling.
 */

enum { GIE_NF1_W_LEN = 0,       /* [0..2]: list lengths, level k's in w[k % 3] */
       GIE_NF1_W_SRC = 3,       /* sources of the current field */
       GIE_NF1_W_BAR = 4,       /* grid-barrier word of k_nf1_bfs */
       GIE_NF1_NWORDS = 8 };    /* (32 bytes, cleared by one memset per compute) */
#define GIE_NF1_BFS_THREADS 1024

struct gie_nf1_dev {
    int32_t *f;
    uint64_t *trav, *known, *vis, *fr0, *fr1;
    int32_t *stamp, *list, *w;
    int W, TY, TZ, ntiles;
};

/* traversable(v) of include/gie.h for the voxel `id` of type ty (shared with the cost matrix, gie_costmat.inc.h) */
GIE_DEV bool gie_nf1_traversable(const gie_ctx &c, const int id, const int8_t ty, const float clearance, const int flags)
{
    const bool open = ty == GIE_VOX_FREE || ty == GIE_VOX_FNT || (ty == GIE_VOX_UNKNOWN && (flags & GIE_NF1_UNKNOWN_TRAVERSABLE));
    return open && gie_edt_value(c, id) >= clearance;
}

/* prep (a): one lane per voxel, a wave per 64-voxel word: the bit planes, the field at -1 and the FNT sources at 0 */
__global__ __launch_bounds__(256) void k_nf1_prep(const gie_ctx c, const gie_nf1_dev s, const int nwords, const float clearance, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= nwords) return;                                   /* wave-uniform */
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane;
    bool tr = false, kn = false, src = false;
    if (x < c.X) {
        const int id = row * c.X + x;
        const int8_t ty = c.glb_type[id];
        kn = ty != GIE_VOX_UNKNOWN;
        tr = gie_nf1_traversable(c, id, ty, clearance, flags);
        src = tr && ty == GIE_VOX_FNT && (flags & GIE_NF1_FROM_FRONTIERS);
        s.f[id] = src ? 0 : -1;
    }
    const uint64_t bt = __ballot(tr), bk = __ballot(kn), bs = __ballot(src);
    if (lane == 0) { s.trav[wd] = bt; s.known[wd] = bk; s.vis[wd] = bs; s.fr0[wd] = bs; s.fr1[wd] = 0; }
}

/* local voxel of a point (metres, world frame) at pivot pvt: gie_pos2coord(p_k, w) - pvt_k; false outside the volume */
GIE_DEV bool gie_nf1_voxel(const gie_ctx &c, const int pvt0, const int pvt1, const int pvt2, const float *p, int v[3])
{
    const int S[3] = { c.X, c.Y, c.Z }, P[3] = { pvt0, pvt1, pvt2 };
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float u = floorf(p[k] / c.voxel_width + 0.5f);
        if (!(u >= -1.0e9f && u <= 1.0e9f)) return false;       /* (NaN, inf, and what no int32 coordinate holds) */
        v[k] = (int)u - P[k];
        if (v[k] < 0 || v[k] >= S[k]) return false;
    }
    return true;
}

/* prep (b): one lane per goal point; traversable goals join the sources */
__global__ __launch_bounds__(256) void k_nf1_goals(const gie_ctx c, const gie_nf1_dev s, const float *xyz, const int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[3];
    if (!gie_nf1_voxel(c, c.pvt[0], c.pvt[1], c.pvt[2], xyz + 3 * (size_t)p, v)) return;
    const size_t row = (size_t)v[2] * c.Y + v[1], wd = row * s.W + (v[0] >> 6);
    const uint64_t bit = 1ull << (v[0] & 63);
    if (!(s.trav[wd] & bit)) return;
    atomicOr((unsigned long long *)&s.fr0[wd], (unsigned long long)bit);
    atomicOr((unsigned long long *)&s.vis[wd], (unsigned long long)bit);
    s.f[row * c.X + v[0]] = 0;
}

/* tile t -> (word column tx, row block ty, slice block tz) */
GIE_DEV void gie_nf1_tile(const gie_nf1_dev &s, const int t, int &tx, int &ty, int &tz)
{
    tx = t % s.W;
    const int r = t / s.W;
    ty = r % s.TY; tz = r / s.TY;
}
/* list tile t and its six face neighbours for the level whose stamp is `stamp` (each tile once per list); all lanes of the wave */
GIE_DEV void gie_nf1_enqueue(const gie_nf1_dev &s, const int t, const int stamp, int32_t *list, int32_t *len)
{
    const int lane = __lane_id();
    int tx, ty, tz;
    gie_nf1_tile(s, t, tx, ty, tz);
    bool first = false;
    int nt = t;
    if (lane < 7) {
        const int a = lane == 0 ? -1 : (lane - 1) >> 1, d = (lane & 1) ? -1 : 1;   /* lane 0: t itself; 1..6: -x +x -y +y -z +z */
        int q[3] = { tx, ty, tz };
        const int S[3] = { s.W, s.TY, s.TZ };
        bool in = true;
        if (a >= 0) { q[a] += d; in = q[a] >= 0 && q[a] < S[a]; }
        if (in) {
            nt = (q[2] * s.TY + q[1]) * s.W + q[0];
            first = __hip_atomic_fetch_max(&s.stamp[nt], stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < stamp;
        }
    }
    gie_list_append_wave(list, len, first, nt);
}

/* prep (c): one wave per tile: the sources are counted and the tiles around them make up the list of level 0 */
__global__ __launch_bounds__(256) void k_nf1_seed(const gie_ctx c, const gie_nf1_dev s)
{
    const int t = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= s.ntiles) return;                                  /* wave-uniform */
    int tx, ty, tz;
    gie_nf1_tile(s, t, tx, ty, tz);
    const int y = ty * 8 + (lane & 7), z = tz * 8 + (lane >> 3);
    int n = (y < c.Y && z < c.Z) ? __popcll(s.fr0[((size_t)z * c.Y + y) * s.W + tx]) : 0;
    for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
    if (n == 0) return;                                         /* wave-uniform */
    if (lane == 0) gie_aadd32(&s.w[GIE_NF1_W_SRC], n);
    gie_nf1_enqueue(s, t, 1, s.list, &s.w[GIE_NF1_W_LEN]);
}

/* the grid barrier of k_nf1_bfs: gie_grid_sync's protocol (every shared word is read and written with agent-scope accesses), but
 * a timeout sets only its own bit of the error word (GIE_ERRF_NF1_BARRIER, reported as GIE_ERR_TIMEOUT by the next sync): the map
 * update's barrier-failure word is left alone.  The arrival count wraps (one round per BFS level: a winding 512^3 field has tens of
 * millions): it is compared by the sign of the 32-bit difference, exact while fewer than 2^31 arrivals separate count and target.
 * errf: the caller's bit (the cost matrix's propagation, gie_costmat.inc.h, has its own). */
GIE_DEV bool gie_nf1_sync(const gie_ctx &c, int32_t *word, uint32_t &epoch, int *s_fail, const int errf = GIE_ERRF_NF1_BARRIER)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    epoch += 1;
    if (threadIdx.x == 0 && gridDim.x > 1) {
        const uint32_t target = epoch * gridDim.x;
        __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while ((int32_t)((uint32_t)__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > GIE_BAR_SPIN_LIMIT) { gie_aor32(&c.cnt[GIE_CNT_ERR], errf); *s_fail = 1; break; }
        }
    }
    __syncthreads();
    return *s_fail == 0;
}

/* the propagation: one persistent launch, all workgroups co-resident (grid <= gie_config.wave_workgroups), a round per BFS level */
__global__ __launch_bounds__(GIE_NF1_BFS_THREADS) void k_nf1_bfs(const gie_ctx c, const gie_nf1_dev s, int32_t *n_sources)
{
    __shared__ int s_fail;
    if (threadIdx.x == 0) s_fail = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_sources) *n_sources = s.w[GIE_NF1_W_SRC];
    __syncthreads();
    constexpr int WAVES = GIE_NF1_BFS_THREADS / 64;
    const int lane = threadIdx.x & 63, gw = blockIdx.x * WAVES + (int)(threadIdx.x >> 6), nw = gridDim.x * WAVES;
    const int W = s.W, X = c.X, Y = c.Y, Z = c.Z;
    const size_t slice = (size_t)Y * W;
    uint32_t epoch = 0;
#pragma unroll 1
    for (int k = 0;; k++) {
        const int n = gie_ld(&s.w[GIE_NF1_W_LEN + k % 3]);    /* (the same in every workgroup: appended before the last barrier) */
        if (n == 0) break;
        if (blockIdx.x == 0 && threadIdx.x == 0) gie_st(&s.w[GIE_NF1_W_LEN + (k + 2) % 3], 0);   /* (last read in round k - 1) */
        const int32_t *list = s.list + (size_t)(k & 1) * s.ntiles;
        int32_t *next = s.list + (size_t)((k + 1) & 1) * s.ntiles;
        int32_t *next_len = &s.w[GIE_NF1_W_LEN + (k + 1) % 3];
        const uint64_t *fk = (k & 1) ? s.fr1 : s.fr0;
        uint64_t *fn = (k & 1) ? s.fr0 : s.fr1;
#pragma unroll 1
        for (int i = gw; i < n; i += nw) {                      /* wave-uniform */
            const int t = gie_ld(&list[i]);
            int tx, ty, tz;
            gie_nf1_tile(s, t, tx, ty, tz);
            const int y = ty * 8 + (lane & 7), z = tz * 8 + (lane >> 3);
            uint64_t nb = 0;
            if (y < Y && z < Z) {
                /* a neighbour's word may still hold an older frontier of the same parity (its tile was not listed since): its
                 * voxels' neighbours are all visited by now, so the stale bits add nothing */
                const size_t row = (size_t)z * Y + y, wd = row * W + tx;
                const uint64_t f = gie_ld(&fk[wd]);
                uint64_t d = f | (f << 1) | (f >> 1);
                if (tx > 0) d |= gie_ld(&fk[wd - 1]) >> 63;
                if (tx < W - 1) d |= gie_ld(&fk[wd + 1]) << 63;
                if (y > 0) d |= gie_ld(&fk[wd - W]);
                if (y < Y - 1) d |= gie_ld(&fk[wd + W]);
                if (z > 0) d |= gie_ld(&fk[wd - slice]);
                if (z < Z - 1) d |= gie_ld(&fk[wd + slice]);
                const uint64_t v = gie_ld(&s.vis[wd]);
                nb = d & s.trav[wd] & ~v;                       /* (trav has no bits beyond X) */
                gie_st(&fn[wd], nb);
                if (nb) {
                    gie_st(&s.vis[wd], v | nb);
                    int32_t *fr = s.f + row * X + tx * 64;
                    for (uint64_t b = nb; b; b &= b - 1) fr[__builtin_ctzll(b)] = k + 1;
                }
            }
            if (__any(nb != 0)) gie_nf1_enqueue(s, t, k + 2, next, next_len);
        }
        if (!gie_nf1_sync(c, &s.w[GIE_NF1_W_BAR], epoch, &s_fail)) break;
    }
}

/* gie_nf1_path: one lane per start point, a descent of nf1(s) steps; the six neighbours of a step are loaded together */
__global__ __launch_bounds__(256) void k_nf1_path(const gie_ctx c, const int32_t *f, const int pvt0, const int pvt1, const int pvt2,
                                                  const float *xyz, const int n, const int max_len, int32_t *path, int32_t *len)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[3];
    const bool in = gie_nf1_voxel(c, pvt0, pvt1, pvt2, xyz + 3 * (size_t)p, v);
    const int X = c.X, Y = c.Y, Z = c.Z, plane = X * Y;
    int id = in ? gie_lid(c, v[0], v[1], v[2]) : 0;
    int cur = in ? f[id] : -1;
    len[p] = cur + 1;                                           /* (0 outside the volume and where nf1 < 0) */
    if (cur < 0) return;
    int32_t *out = path + (size_t)p * max_len * 3;
    int x = v[0], y = v[1], z = v[2];
    for (int i = 0; i < max_len; i++) {
        out[3 * i] = x + pvt0; out[3 * i + 1] = y + pvt1; out[3 * i + 2] = z + pvt2;
        if (cur == 0 || i + 1 == max_len) break;
        const int nb[6] = { x > 0 ? f[id - 1] : -1, x < X - 1 ? f[id + 1] : -1, y > 0 ? f[id - X] : -1,
                            y < Y - 1 ? f[id + X] : -1, z > 0 ? f[id - plane] : -1, z < Z - 1 ? f[id + plane] : -1 };
        const int want = cur - 1;
        if (nb[0] == want) { x--; id--; }
        else if (nb[1] == want) { x++; id++; }
        else if (nb[2] == want) { y--; id -= X; }
        else if (nb[3] == want) { y++; id += X; }
        else if (nb[4] == want) { z--; id -= plane; }
        else if (nb[5] == want) { z++; id += plane; }
        else break;                                             /* (never in a complete field; one cut short by a barrier timeout) */
        cur = want;
    }
}

/* the TYPE_NF1 CostMap payload */
struct op_nf1_costmap {
    const int32_t *f; const uint64_t *known; int W; gie_seendist *out;
    GIE_DEVM void operator()(const gie_ctx &c, int i) const {
        const int row = i / c.X, x = i - row * c.X;
        const int v = f[i];
        gie_seendist sd; sd.d = v >= 0 ? (float)v : -1.0f; sd.s = 0;
        sd.o = (uint8_t)((known[(size_t)row * W + (x >> 6)] >> (x & 63)) & 1ull); sd.pad[0] = sd.pad[1] = 0;
        out[i] = sd;
    }
};
struct op_nf1_copy { const int32_t *f; int32_t *out; GIE_DEVM void operator()(const gie_ctx &, int i) const { out[i] = f[i]; } };

/* ---- host side */
static gie_nf1_dev gie_nf1_view(const gie_mapper *m)
{
    const gie_ctx &c = m->c;
    gie_nf1_dev s;
    s.W = (c.X + 63) / 64; s.TY = (c.Y + 7) / 8; s.TZ = (c.Z + 7) / 8; s.ntiles = s.W * s.TY * s.TZ;
    const size_t nwords = (size_t)s.W * c.Y * c.Z;
    s.f = m->nf1.f;
    s.trav = m->nf1.bits; s.known = s.trav + nwords; s.vis = s.known + nwords; s.fr0 = s.vis + nwords; s.fr1 = s.fr0 + nwords;
    s.w = m->nf1.words; s.stamp = s.w + GIE_NF1_NWORDS; s.list = s.stamp + s.ntiles;
    return s;
}
static int gie_nf1_check(gie_mapper *m, const char *who, bool need_field)
{
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) { gie_set_err(std::string(who) + ": not for a tiled mapper (its field would stop at the tile's faces)"); return GIE_ERR_INVALID; }
    if (need_field && !m->nf1.valid) { gie_set_err(std::string(who) + ": no navigation function yet (gie_nf1_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}

extern "C" int gie_nf1_compute_dev(gie_mapper *m, const float *d_goal_xyz, int n, const gie_nf1_param *p, int32_t *d_n_sources)
{
    int rc = gie_nf1_check(m, "gie_nf1_compute_dev", false); if (rc) return rc;
    if (!p || n < 0 || (n > 0 && !d_goal_xyz)) { gie_set_err("gie_nf1_compute_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (!(p->clearance >= 0.f && p->clearance <= 3.402823466e38f)) { gie_set_err("gie_nf1_compute_dev: clearance must be finite and >= 0"); return GIE_ERR_INVALID; }
    if (p->flags & ~(GIE_NF1_UNKNOWN_TRAVERSABLE | GIE_NF1_FROM_FRONTIERS)) { gie_set_err("gie_nf1_compute_dev: unknown flags"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this field) */
    const int W = (c.X + 63) / 64, nwords = W * c.Y * c.Z, ntiles = W * ((c.Y + 7) / 8) * ((c.Z + 7) / 8);
    if (!m->nf1.f) {
        int32_t *f = gie_dalloc<int32_t>(m, (size_t)c.N, false);
        uint64_t *bits = f ? gie_dalloc<uint64_t>(m, 5 * (size_t)nwords, false) : nullptr;
        int32_t *words = bits ? gie_dalloc<int32_t>(m, GIE_NF1_NWORDS + 3 * (size_t)ntiles, false) : nullptr;
        if (!words) { gie_set_err("gie_nf1_compute_dev: device allocation of the navigation function failed"); return GIE_ERR_DEVICE; }
        m->nf1.f = f; m->nf1.bits = bits; m->nf1.words = words;
    }
    const gie_nf1_dev s = gie_nf1_view(m);
    be_memset(&m->be, s.w, 0, (GIE_NF1_NWORDS + (size_t)ntiles) * sizeof(int32_t));   /* control words and stamps */
    GIE_LAUNCH(&m->be, k_nf1_prep, dim3((nwords + 3) / 4), dim3(256), 0, c, s, nwords, p->clearance, (int)p->flags);
    if (n > 0) GIE_LAUNCH(&m->be, k_nf1_goals, dim3((n + 255) / 256), dim3(256), 0, c, s, d_goal_xyz, n);
    GIE_LAUNCH(&m->be, k_nf1_seed, dim3((ntiles + 3) / 4), dim3(256), 0, c, s);
    /* a grid-barrier launch: it joins the device's chain of such launches (be_chained), so that it is never resident together
     * with another mapper's waves launch */
    be_chained(&m->be, [&]() { GIE_LAUNCH(&m->be, k_nf1_bfs, dim3(m->be.num_cu), dim3(GIE_NF1_BFS_THREADS), 0, c, s, d_n_sources); });
    for (int i = 0; i < 3; i++) { m->nf1.pvt[i] = c.pvt[i]; m->nf1.origin[i] = m->msg_origin[i]; }
    m->nf1.valid = 1;
    return GIE_OK;
}
extern "C" int gie_nf1_compute(gie_mapper *m, const float *goal_xyz, int n, const gie_nf1_param *p, int32_t *n_sources)
{
    int rc = gie_nf1_check(m, "gie_nf1_compute", false); if (rc) return rc;
    if (n < 0 || (n > 0 && !goal_xyz)) { gie_set_err("gie_nf1_compute: bad arguments"); return GIE_ERR_INVALID; }
    float *dg = nullptr;
    if (n > 0) {
        dg = (float *)gie_scratch(m, 0, (size_t)n * 12, "gie_nf1_compute");
        if (!dg) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dg, goal_xyz, (size_t)n * 12);
    }
    rc = gie_nf1_compute_dev(m, dg, n, p, nullptr); if (rc) return rc;
    if (n_sources) be_d2h(&m->be, n_sources, m->nf1.words + GIE_NF1_W_SRC, sizeof(int32_t));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_read_nf1_dev(gie_mapper *m, int32_t *d_nf1)
{
    int rc = gie_nf1_check(m, "gie_read_nf1_dev", true); if (rc) return rc;
    if (!d_nf1) { gie_set_err("gie_read_nf1_dev: null output"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this reader) */
    op_nf1_copy op; op.f = m->nf1.f; op.out = d_nf1;
    be_lin(&m->be, c, op, c.N);
    return GIE_OK;
}
extern "C" int gie_read_nf1(gie_mapper *m, int32_t *nf1)
{
    int rc = gie_nf1_check(m, "gie_read_nf1", true); if (rc) return rc;
    if (nf1) be_d2h(&m->be, nf1, m->nf1.f, (size_t)m->c.N * 4);
    return gie_sync(m);
}
extern "C" int gie_nf1_path_dev(gie_mapper *m, const float *d_start_xyz, int n, int max_len, int32_t *d_path_xyz, int32_t *d_len)
{
    int rc = gie_nf1_check(m, "gie_nf1_path_dev", true); if (rc) return rc;
    if (n < 0 || max_len < 0 || (n > 0 && (!d_start_xyz || !d_len || (max_len > 0 && !d_path_xyz)))) { gie_set_err("gie_nf1_path_dev: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    gie_ctx c = m->c;
    c.gate = nullptr;
    GIE_LAUNCH(&m->be, k_nf1_path, dim3((n + 255) / 256), dim3(256), 0, c, m->nf1.f, m->nf1.pvt[0], m->nf1.pvt[1], m->nf1.pvt[2],
               d_start_xyz, n, max_len, d_path_xyz, d_len);
    return GIE_OK;
}
extern "C" int gie_nf1_path(gie_mapper *m, const float *start_xyz, int n, int max_len, int32_t *path_xyz, int32_t *len)
{
    int rc = gie_nf1_check(m, "gie_nf1_path", true); if (rc) return rc;
    if (n < 0 || max_len < 0 || (n > 0 && (!start_xyz || !len || (max_len > 0 && !path_xyz)))) { gie_set_err("gie_nf1_path: bad arguments"); return GIE_ERR_INVALID; }
    if (n == 0) return GIE_OK;
    const size_t pbytes = (size_t)n * max_len * 12;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 12, "gie_nf1_path");
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 4 + pbytes, "gie_nf1_path");     /* lengths, then the points */
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, start_xyz, (size_t)n * 12);
    rc = gie_nf1_path_dev(m, dx, n, max_len, (int32_t *)(dr + (size_t)n * 4), (int32_t *)dr); if (rc) return rc;
    be_d2h(&m->be, len, dr, (size_t)n * 4);
    if (pbytes) be_d2h(&m->be, path_xyz, dr + (size_t)n * 4, pbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}
static void gie_nf1_costmap_hdr(const gie_mapper *m, gie_costmap_hdr *hdr)
{
    gie_fill_costmap_hdr(m, hdr);
    hdr->x_origin = m->nf1.origin[0]; hdr->y_origin = m->nf1.origin[1]; hdr->z_origin = m->nf1.origin[2];
    hdr->type = 2;
}
extern "C" int gie_read_costmap_nf1_dev(gie_mapper *m, gie_seendist *d_payload, gie_costmap_hdr *hdr)
{
    int rc = gie_nf1_check(m, "gie_read_costmap_nf1_dev", true); if (rc) return rc;
    if (!d_payload) { gie_set_err("gie_read_costmap_nf1_dev: null payload"); return GIE_ERR_INVALID; }
    gie_ctx c = m->c;
    c.gate = nullptr;
    op_nf1_costmap op; op.f = m->nf1.f; op.known = gie_nf1_view(m).known; op.W = (c.X + 63) / 64; op.out = d_payload;
    be_lin(&m->be, c, op, c.N);
    if (hdr) gie_nf1_costmap_hdr(m, hdr);
    return GIE_OK;
}
extern "C" int gie_read_costmap_nf1(gie_mapper *m, gie_seendist *payload, gie_costmap_hdr *hdr)
{
    int rc = gie_nf1_check(m, "gie_read_costmap_nf1", true); if (rc) return rc;
    if (payload) {
        const size_t N = (size_t)m->c.N;
        gie_seendist *d = (gie_seendist *)gie_scratch(m, 1, N * sizeof(gie_seendist), "gie_read_costmap_nf1");
        if (!d) return GIE_ERR_DEVICE;
        rc = gie_read_costmap_nf1_dev(m, d, nullptr); if (rc) return rc;
        be_d2h(&m->be, payload, d, N * sizeof(gie_seendist));
        gie_scratch_trim(m);
    }
    if (hdr) gie_nf1_costmap_hdr(m, hdr);
    return gie_sync(m);
}

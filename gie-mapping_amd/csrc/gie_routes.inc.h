/*
 * gie_routes.inc.h — global block routes: the graph of the 8x8x8 blocks of everything mapped so far — a node per block with enough
 * passable voxels, a link per block face with enough passable voxel pairs across it — and a BFS field on it, over a finite box of
 * blocks (include/gie.h "global block routes").  The global counterpart of gie_nf1_* and gie_ground_nf1_*.
 * HIP backend only: included by gie_hip.hip after gie_blocks.inc.h and the ground sections (whose word walk and LDS limit it
 * shares).  It reads the map and writes nothing of it; its own planes are per CELL (a block of the box) and are allocated at the
 * first compute, grown when a later box is larger.
 *   k_routes_links   k_blocks_summary's walk of the pool: half a wave a slot, 16 consecutive bytes of the block's types per lane
 *                    (voxel j of lane `part` at x = j & 7, y = 2 (part & 3) + (j >> 3), z = part >> 2), 1 to 16 units of eight slots
 *                    per workgroup (gie_cloud_iters).  Lanes 0 .. 2 of the slot look up the blocks k + e_x / e_y / e_z
 *                    (gie_hash_find, only where that block lies in the box) and hand the slot to the others by shuffle.  The
 *                    neighbour's opposite face: x = 0 is 64 single bytes at stride 8 (two per lane), y = 0 eight 8-byte runs (the
 *                    lanes with part & 3 == 3), z = 0 64 contiguous bytes (lanes 28 .. 31, 16 bytes each).  A lane counts passable
 *                    and FNT voxels into one word (two 10-bit fields) and its open pairs into another (three 8-bit fields); five
 *                    __shfl_xor steps add both.  The slot's first lane stores ONE raw byte for its cell: node, pairs >= min_open
 *                    per axis, frontier.  A block lies in one cell: no atomics; the host has zeroed the raw plane on the stream.
 *   k_routes_prep    one wave per 64-cell word (k_gnf1_prep's form): a raw open bit survives iff the cell beyond it is a node
 *                    inside the box; the final byte, the field at -1 (frontier sources at 0) and by ballot the bit planes OX / OY /
 *                    OZ (bit x of a word: the link from cell x towards +x / +y / +z), blk = ~node | source (padding bits beyond
 *                    nx SET) and the level-0 frontier (padding clear).  The final bytes go to a plane of their own, so no lane
 *                    reads a byte another lane rewrites.
 *   k_routes_goals   one lane per goal point (k_gnf1_goals' form): ONE atomic OR on blk decides.
 *   k_routes_bfs     ONE workgroup of 1024 threads (k_gnf1_bfs's structure); a thread owns the words tid + 1024 j.  Per level
 *                      next = ((F & OX) << 1 | (F >> 1) & OX, with the carries of the words left and right
 *                             | (F & OY)[row y - 1] | F[row y + 1] & OY | (F & OZ)[plane z - 1] | F[plane z + 1] & OZ) & ~blk
 *                    then blk |= next, level + 1 to the field at each new bit, "any new" ORed in LDS, one workgroup barrier.  No
 *                    link leaves the box, so OX is clear in a row's last cell, OY in a plane's last row, OZ in the last plane:
 *                    the terms of the neighbouring words need guards against the ends of the planes only.  LDS = true: all six
 *                    planes in dynamic LDS (at most GIE_ROUTES_LDS_WORDS words each, within ground NF1's 144 KiB); otherwise F,
 *                    blk, OX, OY, OZ stay where they lie, next stays in LDS (at most GIE_ROUTES_MAX_WORDS words = 128 KiB) and a
 *                    second barrier follows each level.  The host picks the form by the size alone.  The level loop is bounded
 *                    by the number of cells whatever the planes hold.  No grid barrier, no cooperative launch, no timeout path.
 *                    The info record comes from popcounts of the planes here (n_frontier from k_routes_prep).
 *   k_routes_path / k_routes_query   one lane per start / point; the exports one lane per cell (k_lin).
 * No kernel uses scratch.  The compiler's figures and the times are in DESIGN.md 35.
 */

#define GIE_ROUTES_THREADS 1024
#define GIE_ROUTES_LDS_WORDS (GIE_GNF1_LDS_BYTES / 48)          /* words of ONE plane when six fit: 3072 */
#define GIE_ROUTES_MAX_WORDS 16384                               /* the "next" plane alone in LDS: 128 KiB */
enum { GIE_ROUTES_RAW_NODE = 1, GIE_ROUTES_RAW_FNT = 16, GIE_ROUTES_SOURCE = 32 };
enum { GIE_ROUTES_I_NODES = 0, GIE_ROUTES_I_LINKS, GIE_ROUTES_I_FRONTIER, GIE_ROUTES_I_SOURCES, GIE_ROUTES_I_REACHED, GIE_ROUTES_I_MAXSTEPS };

struct gie_routes_dev {
    int lo[3], nx, ny, nz, W, nwords;
    uint8_t *raw, *cells;                   /* a byte per cell: k_routes_links' and the final one */
    int32_t *f;                             /* the field */
    uint64_t *blk, *fr, *ox, *oy, *oz;      /* nwords each */
    int32_t *info;                          /* gie_routes_info */
};
struct gie_routes_sel { int min_free, min_open, min_fnt, iters; };

GIE_DEV uint32_t gie_routes_passable(uint32_t ty) { return (ty | 2u) == 3u ? 1u : 0u; }                 /* FREE (1) or FNT (3) */

__global__ __launch_bounds__(256) void k_routes_links(const gie_ctx c, const gie_routes_dev s, const gie_routes_sel q)
{
    int bound = c.pool_count[0];
    bound = bound < c.max_blocks ? bound : c.max_blocks;
    if ((int)blockIdx.x * GIE_CLOUD_SLOTS * q.iters >= bound) return;      /* workgroup-uniform */
    const int half = threadIdx.x >> 5, part = threadIdx.x & 31;
    const int slot0 = (int)blockIdx.x * GIE_CLOUD_SLOTS * q.iters + half;
    const int lane0 = (int)__lane_id() & 32;                               /* the slot's first lane in its wave */
#pragma unroll 1
    for (int r = 0; r < q.iters; r++) {
        const int slot = slot0 + r * GIE_CLOUD_SLOTS;
        const uint64_t key = slot < bound ? c.g_key[slot] : GIE_KEY_EMPTY;
        int k[3] = { 0, 0, 0 };
        uint32_t cell[3] = { 0u, 0u, 0u };                                 /* k - lo, unsigned: a block below lo wraps far beyond any side */
        bool in = key != GIE_KEY_EMPTY;                                    /* uniform over the half wave */
        if (in) {
            gie_unpack_crd(key, &k[0], &k[1], &k[2]);
#pragma unroll
            for (int a = 0; a < 3; a++) cell[a] = (uint32_t)k[a] - (uint32_t)s.lo[a];
            in = cell[0] < (uint32_t)s.nx && cell[1] < (uint32_t)s.ny && cell[2] < (uint32_t)s.nz;
        }
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        int nb = -1;
        if (in) {
            t = *reinterpret_cast<const uint4 *>(c.g_type + (gie_vaddr)slot * GIE_VBSZ + part * 16);
            if (part < 3) {                                                /* lane a: the block beyond the + face of axis a, if the box holds it */
                const uint32_t n[3] = { (uint32_t)s.nx, (uint32_t)s.ny, (uint32_t)s.nz };
                if (cell[part] + 1u < n[part]) nb = gie_hash_find(c, k[0] + (part == 0), k[1] + (part == 1), k[2] + (part == 2));
            }
        }
        const int nbx = __shfl(nb, lane0), nby = __shfl(nb, lane0 + 1), nbz = __shfl(nb, lane0 + 2);
        uint32_t cnt = 0u, pairs = 0u;                                     /* passable | FNT << 10;  pairs x | y << 8 | z << 16 */
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t ty = gie_cloud_byte(t, j);
            cnt += gie_routes_passable(ty) + (ty == (uint32_t)GIE_VOX_FNT ? 1u << 10 : 0u);
        }
        if (nbx >= 0) {                                                    /* own x = 7 (j = 7, 15) against the neighbour's x = 0 of the same rows */
            const uint8_t *f = reinterpret_cast<const uint8_t *>(c.g_type) + (gie_vaddr)nbx * GIE_VBSZ + part * 16;
            pairs += gie_routes_passable(gie_cloud_byte(t, 7)) & gie_routes_passable(f[0]);
            pairs += gie_routes_passable(gie_cloud_byte(t, 15)) & gie_routes_passable(f[8]);
        }
        if (nby >= 0 && (part & 3) == 3) {                                 /* own y = 7 (j = 8 .. 15) against the neighbour's y = 0 run of the same z */
            const uint2 f = *reinterpret_cast<const uint2 *>(c.g_type + (gie_vaddr)nby * GIE_VBSZ + (part >> 2) * 64);
#pragma unroll
            for (int j = 0; j < 8; j++)
                pairs += (gie_routes_passable(gie_cloud_byte(t, 8 + j)) & gie_routes_passable(((j < 4 ? f.x : f.y) >> (8 * (j & 3))) & 0xffu)) << 8;
        }
        if (nbz >= 0 && (part >> 2) == 7) {                                /* own z = 7 against the neighbour's z = 0 layer, the same 16 bytes of it */
            const uint4 f = *reinterpret_cast<const uint4 *>(c.g_type + (gie_vaddr)nbz * GIE_VBSZ + (part & 3) * 16);
#pragma unroll
            for (int j = 0; j < 16; j++) pairs += (gie_routes_passable(gie_cloud_byte(t, j)) & gie_routes_passable(gie_cloud_byte(f, j))) << 16;
        }
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) {
            cnt += (uint32_t)__shfl_xor((int)cnt, d);
            pairs += (uint32_t)__shfl_xor((int)pairs, d);
        }
        if (part == 0 && in && (int)(cnt & 0x3ffu) >= q.min_free) {        /* (a cell without a node stays 0) */
            const uint32_t b = GIE_ROUTES_RAW_NODE | ((int)(pairs & 0xffu) >= q.min_open ? 2u : 0u) | ((int)((pairs >> 8) & 0xffu) >= q.min_open ? 4u : 0u) |
                               ((int)(pairs >> 16) >= q.min_open ? 8u : 0u) | ((int)(cnt >> 10) >= q.min_fnt ? (uint32_t)GIE_ROUTES_RAW_FNT : 0u);
            s.raw[(cell[2] * (uint32_t)s.ny + cell[1]) * (uint32_t)s.nx + cell[0]] = (uint8_t)b;
        }
    }
}

__global__ __launch_bounds__(256) void k_routes_prep(const gie_routes_dev s, const int flags)
{
    const int wd = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wd >= s.nwords) return;                                 /* wave-uniform */
    const int row = wd / s.W, x = (wd - row * s.W) * 64 + lane, z = row / s.ny, y = row - z * s.ny;
    bool node = false, ox = false, oy = false, oz = false, fnt = false, src = false;
    if (x < s.nx) {
        const int id = row * s.nx + x, plane = s.nx * s.ny;
        const uint32_t b = s.raw[id];
        node = b & GIE_ROUTES_RAW_NODE;
        ox = (b & 2u) && x + 1 < s.nx && (s.raw[id + 1] & GIE_ROUTES_RAW_NODE);
        oy = (b & 4u) && y + 1 < s.ny && (s.raw[id + s.nx] & GIE_ROUTES_RAW_NODE);
        oz = (b & 8u) && z + 1 < s.nz && (s.raw[id + plane] & GIE_ROUTES_RAW_NODE);
        fnt = b & GIE_ROUTES_RAW_FNT;
        src = fnt && (flags & GIE_ROUTES_FROM_FRONTIERS);
        s.cells[id] = (uint8_t)(node ? 1u | (ox ? 2u : 0u) | (oy ? 4u : 0u) | (oz ? 8u : 0u) | (fnt ? 16u : 0u) | (src ? (uint32_t)GIE_ROUTES_SOURCE : 0u) : 0u);
        s.f[id] = src ? 0 : -1;
    }
    const uint64_t bn = __ballot(node), bx = __ballot(ox), by = __ballot(oy), bz = __ballot(oz), bf = __ballot(fnt), bs = __ballot(src);
    if (lane == 0) {
        s.blk[wd] = ~bn | bs; s.fr[wd] = bs; s.ox[wd] = bx; s.oy[wd] = by; s.oz[wd] = bz;
        if (bf) atomicAdd(&s.info[GIE_ROUTES_I_FRONTIER], __popcll(bf));
    }
}

/* the cell of a point (metres, world frame): gie_pos2coord per axis, >> 3, less the box's corner; false outside the box or not finite */
GIE_DEV bool gie_routes_cell(const gie_routes_dev &s, const float w, const float *p, int v[3])
{
    const int n[3] = { s.nx, s.ny, s.nz };
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float u = floorf(p[k] / w + 0.5f);
        if (!(u >= -1.0e9f && u <= 1.0e9f)) return false;       /* (NaN, inf, and what no int32 coordinate holds) */
        const long long b = (long long)((int)u >> 3) - s.lo[k];
        if (b < 0 || b >= n[k]) return false;
        v[k] = (int)b;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_routes_goals(const gie_routes_dev s, const float w, const float *xyz, const int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[3];
    if (!gie_routes_cell(s, w, xyz + 3 * (size_t)p, v)) return;
    const int row = v[2] * s.ny + v[1], wd = row * s.W + (v[0] >> 6), id = row * s.nx + v[0];
    const unsigned long long bit = 1ull << (v[0] & 63);
    if (atomicOr((unsigned long long *)&s.blk[wd], bit) & bit) return;       /* no node, or a source already */
    atomicOr((unsigned long long *)&s.fr[wd], bit);
    s.f[id] = 0;
    s.cells[id] = (uint8_t)(s.cells[id] | GIE_ROUTES_SOURCE);   /* (this lane alone won the cell) */
}

template <bool LDS>
__global__ __launch_bounds__(GIE_ROUTES_THREADS) void k_routes_bfs(const gie_routes_dev s, int32_t *info2)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_planes[];     /* next; in the LDS form F, blk, OX, OY, OZ behind it */
    __shared__ int s_cnt[GIE_ROUTES_THREADS / 64][4], s_any[3];
    const int nwords = s.nwords, tid = threadIdx.x, W = s.W, WP = s.W * s.ny, nx = s.nx;
    uint64_t *NX = s_planes, *F = LDS ? s_planes + nwords : s.fr, *B = LDS ? s_planes + 2 * (size_t)nwords : s.blk;
    const uint64_t *OX = LDS ? s_planes + 3 * (size_t)nwords : s.ox, *OY = LDS ? s_planes + 4 * (size_t)nwords : s.oy, *OZ = LDS ? s_planes + 5 * (size_t)nwords : s.oz;
    const gie_ground_words w0 = gie_ground_words_first(tid, GIE_ROUTES_THREADS, W);      /* (y: the row of all planes, z * ny + y) */
    int n_nodes = 0, n_links = 0, n_src = 0, n_reached = 0;
    for (int wd = tid; wd < nwords; wd += GIE_ROUTES_THREADS) {
        const uint64_t f = s.fr[wd], b = s.blk[wd], x = s.ox[wd], y = s.oy[wd], z = s.oz[wd];
        n_src += __popcll(f);
        n_nodes += __popcll(~b) + __popcll(f);
        n_links += __popcll(x) + __popcll(y) + __popcll(z);
        if (LDS) { s_planes[nwords + wd] = f; s_planes[2 * (size_t)nwords + wd] = b; s_planes[3 * (size_t)nwords + wd] = x; s_planes[4 * (size_t)nwords + wd] = y; s_planes[5 * (size_t)nwords + wd] = z; }
    }
    if (tid == 0) s_any[0] = s_any[1] = s_any[2] = 0;
    __syncthreads();
    const int max_levels = nx * s.ny * s.nz;                    /* no path is longer: the loop ends here whatever the planes hold */
    int levels = 0;
#pragma unroll 1
    for (int level = 0; level < max_levels; level++) {
        if (tid == 0) s_any[(level + 1) % 3] = 0;               /* (last read after the barrier of level - 2, next set in level + 1) */
        int any = 0;
        gie_ground_words w = w0;
#pragma unroll 1
        for (int wd = tid; wd < nwords; wd += GIE_ROUTES_THREADS) {
            const uint64_t f = F[wd], x = OX[wd];
            uint64_t d = ((f & x) << 1) | ((f >> 1) & x);
            if (wd > 0) d |= (F[wd - 1] & OX[wd - 1]) >> 63;
            if (wd + 1 < nwords) d |= (F[wd + 1] << 63) & x;
            if (wd >= W) d |= F[wd - W] & OY[wd - W];
            if (wd + W < nwords) d |= F[wd + W] & OY[wd];
            if (wd >= WP) d |= F[wd - WP] & OZ[wd - WP];
            if (wd + WP < nwords) d |= F[wd + WP] & OZ[wd];
            const uint64_t bl = B[wd], nw = d & ~bl;            /* (blk holds the padding bits beyond nx; only its owner touches a word of it) */
            NX[wd] = nw;
            if (nw) {
                any = 1;
                n_reached += __popcll(nw);
                B[wd] = bl | nw;
                int32_t *fr = s.f + (size_t)w.y * nx + w.tx * 64;
                for (uint64_t b = nw; b; b &= b - 1) fr[__builtin_ctzll(b)] = level + 1;
            }
            gie_ground_words_next(w, W);
        }
        if (__any(any) && (tid & 63) == 0) s_any[level % 3] = 1;
        __syncthreads();                                        /* every read of F is done, next is complete */
        if (!s_any[level % 3]) break;                           /* (workgroup-uniform) nothing new: the field is complete */
        levels = level + 1;
        if (LDS) { uint64_t *t = F; F = NX; NX = t; }
        else {
            for (int wd = tid; wd < nwords; wd += GIE_ROUTES_THREADS) F[wd] = NX[wd];
            __syncthreads();
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_nodes += __shfl_xor(n_nodes, d); n_links += __shfl_xor(n_links, d); n_src += __shfl_xor(n_src, d); n_reached += __shfl_xor(n_reached, d);
    }
    if ((tid & 63) == 0) { s_cnt[tid >> 6][0] = n_nodes; s_cnt[tid >> 6][1] = n_links; s_cnt[tid >> 6][2] = n_src; s_cnt[tid >> 6][3] = n_reached; }
    __syncthreads();
    if (tid == 0) {
        int t[4] = { 0, 0, 0, 0 };
        for (int i = 0; i < GIE_ROUTES_THREADS / 64; i++) for (int j = 0; j < 4; j++) t[j] += s_cnt[i][j];
        const int out[8] = { t[0], t[1], s.info[GIE_ROUTES_I_FRONTIER], t[2], t[2] + t[3], t[2] > 0 ? levels : -1, 0, 0 };
        for (int j = 0; j < 8; j++) { s.info[j] = out[j]; if (info2) info2[j] = out[j]; }
    }
}

/* gie_routes_path: one lane per start, a descent of steps(k_0) links; neighbours in the order -x +x -y +y -z +z */
__global__ __launch_bounds__(256) void k_routes_path(const gie_routes_dev s, const float w, const float *xyz, const int n, const int max_len, int32_t *path, int32_t *len)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[3] = { 0, 0, 0 };
    const bool in = gie_routes_cell(s, w, xyz + 3 * (size_t)p, v);
    const int nx = s.nx, plane = s.nx * s.ny;
    int id = in ? (v[2] * s.ny + v[1]) * nx + v[0] : 0;
    int cur = in ? s.f[id] : -1;
    len[p] = cur + 1;                                           /* (0 outside the box and where steps < 0) */
    if (cur < 0) return;
    int32_t *out = path + (size_t)p * max_len * 3;
    for (int i = 0; i < max_len; i++) {
        out[3 * i] = v[0] + s.lo[0]; out[3 * i + 1] = v[1] + s.lo[1]; out[3 * i + 2] = v[2] + s.lo[2];
        if (cur == 0 || i + 1 == max_len) break;
        const int want = cur - 1;
        const uint32_t b = s.cells[id];
        if (v[0] > 0 && (s.cells[id - 1] & 2u) && s.f[id - 1] == want) { v[0]--; id--; }
        else if ((b & 2u) && s.f[id + 1] == want) { v[0]++; id++; }
        else if (v[1] > 0 && (s.cells[id - nx] & 4u) && s.f[id - nx] == want) { v[1]--; id -= nx; }
        else if ((b & 4u) && s.f[id + nx] == want) { v[1]++; id += nx; }
        else if (v[2] > 0 && (s.cells[id - plane] & 8u) && s.f[id - plane] == want) { v[2]--; id -= plane; }
        else if ((b & 8u) && s.f[id + plane] == want) { v[2]++; id += plane; }
        else break;                                             /* (never in a complete field) */
        cur = want;
    }
}

/* gie_routes_query: one lane per point */
__global__ __launch_bounds__(256) void k_routes_query(const gie_routes_dev s, const float w, const float *xyz, const int n, int32_t *steps)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v[3];
    steps[p] = gie_routes_cell(s, w, xyz + 3 * (size_t)p, v) ? s.f[(v[2] * s.ny + v[1]) * s.nx + v[0]] : -1;
}

struct op_routes_copy_f { const int32_t *f; int32_t *out; GIE_DEVM void operator()(const gie_ctx &, int i) const { out[i] = f[i]; } };
struct op_routes_copy_b { const uint8_t *b; uint8_t *out; GIE_DEVM void operator()(const gie_ctx &, int i) const { out[i] = b[i]; } };

/* ---- host side */
static int gie_routes_check(gie_mapper *m, const char *who, bool need_field)
{
    static_assert(sizeof(gie_routes_param) == 48 && sizeof(gie_routes_info) == 32, "the sizes include/gie.h states");
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    if (gie_tiled(m)) { gie_set_err(std::string(who) + ": not for a tiled mapper (its pool holds ghost blocks of other tiles)"); return GIE_ERR_INVALID; }
    if (need_field && !m->routes.valid) { gie_set_err(std::string(who) + ": no routes yet (gie_routes_compute first)"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static int gie_routes_check_compute(gie_mapper *m, const char *who, const float *goal_xyz, int n, const gie_routes_param *p, int dim[3])
{
    const int rc = gie_routes_check(m, who, false); if (rc) return rc;
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->lo[0] > p->hi[0] || p->lo[1] > p->hi[1] || p->lo[2] > p->hi[2]) bad = "lo > hi";
    else if (p->min_free < 1 || p->min_free > GIE_VBSZ) bad = "min_free must be 1..512";
    else if (p->min_open < 1 || p->min_open > 64) bad = "min_open must be 1..64";
    else if (p->min_fnt < 1 || p->min_fnt > GIE_VBSZ) bad = "min_fnt must be 1..512";
    else if (p->flags & ~GIE_ROUTES_FROM_FRONTIERS) bad = "unknown flags";
    else if (p->reserved[0] || p->reserved[1]) bad = "reserved must be 0";
    else if (n < 0 || (n > 0 && !goal_xyz)) bad = "n < 0, or n > 0 without goals";
    else {
        long long side[3];
        for (int i = 0; i < 3 && !bad; i++) {
            if (p->lo[i] == INT32_MIN || p->hi[i] == INT32_MAX) bad = "the box must be finite";
            side[i] = (long long)p->hi[i] - p->lo[i] + 1;
            if (!bad && side[i] > 64ll * GIE_ROUTES_MAX_WORDS) bad = "the box is too large: at most 16384 64-cell words a plane";
        }
        if (!bad && ((side[0] + 63) / 64) * side[1] * side[2] > GIE_ROUTES_MAX_WORDS) bad = "the box is too large: at most 16384 64-cell words a plane";
        if (!bad) for (int i = 0; i < 3; i++) dim[i] = (int)side[i];
    }
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
static gie_routes_dev gie_routes_view(const gie_mapper *m)
{
    const gie_routes_cache &r = m->routes;
    gie_routes_dev s;
    for (int i = 0; i < 3; i++) s.lo[i] = r.lo[i];
    s.nx = r.dim[0]; s.ny = r.dim[1]; s.nz = r.dim[2];
    s.W = (s.nx + 63) / 64; s.nwords = s.W * s.ny * s.nz;
    s.raw = r.bytes; s.cells = r.bytes + r.cap_cells; s.f = r.f;
    s.blk = r.bits; s.fr = s.blk + r.cap_words; s.ox = s.fr + r.cap_words; s.oy = s.ox + r.cap_words; s.oz = s.oy + r.cap_words;
    s.info = r.info;
    return s;
}
/* a plane of the stage at a larger size: the old one goes back to the device (its place in the list gie_destroy frees is kept) */
template <class T> static bool gie_routes_grow(gie_mapper *m, T **p, size_t n)
{
    T *q = (T *)be_alloc(&m->be, n * sizeof(T), false);
    if (!q) return false;
    if (*p) {
        for (void *&a : m->allocs) if (a == (void *)*p) a = q;
        be_free(&m->be, *p);
    } else m->allocs.push_back(q);
    *p = q;
    return true;
}

extern "C" int gie_routes_compute_dev(gie_mapper *m, const float *d_goal_xyz, int n, const gie_routes_param *p, gie_routes_info *d_info)
{
    const char *who = "gie_routes_compute_dev";
    int dim[3];
    const int rc = gie_routes_check_compute(m, who, d_goal_xyz, n, p, dim); if (rc) return rc;
    const size_t cells = (size_t)dim[0] * dim[1] * dim[2], nwords = (size_t)((dim[0] + 63) / 64) * dim[1] * dim[2];
    static bool attr_done = false;
    const int ra = gie_ground_lds_limit(&attr_done, who, reinterpret_cast<const void *>(&k_routes_bfs<true>), reinterpret_cast<const void *>(&k_routes_bfs<false>), GIE_GNF1_LDS_BYTES);
    if (ra) return ra;
    gie_routes_cache &r = m->routes;
    bool ok = r.info || gie_routes_grow(m, &r.info, 8);
    if (ok && cells > r.cap_cells) {
        const size_t cap = (cells + 15) & ~(size_t)15;
        r.valid = 0;
        ok = gie_routes_grow(m, &r.bytes, 2 * cap) && gie_routes_grow(m, &r.f, cap);
        r.cap_cells = ok ? cap : 0;
    }
    if (ok && nwords > r.cap_words) {
        r.valid = 0;
        ok = gie_routes_grow(m, &r.bits, 5 * nwords);
        r.cap_words = ok ? nwords : 0;
    }
    if (!ok) { gie_set_err(std::string(who) + ": device allocation of the routes' planes failed"); return GIE_ERR_DEVICE; }
    for (int i = 0; i < 3; i++) { r.lo[i] = p->lo[i]; r.dim[i] = dim[i]; }
    const gie_routes_dev s = gie_routes_view(m);
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this stage) */
    gie_routes_sel q;
    q.min_free = p->min_free; q.min_open = p->min_open; q.min_fnt = p->min_fnt;
    const long long units = ((long long)c.max_blocks + GIE_CLOUD_SLOTS - 1) / GIE_CLOUD_SLOTS;
    q.iters = gie_cloud_iters(units);
    be_memset(&m->be, s.raw, 0, cells);
    be_memset(&m->be, s.info, 0, 8 * sizeof(int32_t));
    GIE_LAUNCH(&m->be, k_routes_links, dim3((unsigned)((units + q.iters - 1) / q.iters)), dim3(256), 0, c, s, q);
    GIE_LAUNCH(&m->be, k_routes_prep, dim3((unsigned)((nwords + 3) / 4)), dim3(256), 0, s, (int)p->flags);
    if (n > 0) GIE_LAUNCH(&m->be, k_routes_goals, dim3((n + 255) / 256), dim3(256), 0, s, c.voxel_width, d_goal_xyz, n);
    if (nwords <= GIE_ROUTES_LDS_WORDS)                         /* by the size alone */
        GIE_LAUNCH(&m->be, k_routes_bfs<true>, dim3(1), dim3(GIE_ROUTES_THREADS), 6 * nwords * sizeof(uint64_t), s, (int32_t *)d_info);
    else GIE_LAUNCH(&m->be, k_routes_bfs<false>, dim3(1), dim3(GIE_ROUTES_THREADS), nwords * sizeof(uint64_t), s, (int32_t *)d_info);
    r.valid = 1;
    return GIE_OK;
}
extern "C" int gie_routes_compute(gie_mapper *m, const float *goal_xyz, int n, const gie_routes_param *p, gie_routes_info *info)
{
    const char *who = "gie_routes_compute";
    int dim[3];
    int rc = gie_routes_check_compute(m, who, goal_xyz, n, p, dim); if (rc) return rc;
    float *dg = nullptr;
    if (n > 0) {
        dg = (float *)gie_scratch(m, 0, (size_t)n * 12, who);
        if (!dg) return GIE_ERR_DEVICE;
        be_h2d(&m->be, dg, goal_xyz, (size_t)n * 12);
    }
    rc = gie_routes_compute_dev(m, dg, n, p, nullptr); if (rc) return rc;
    if (info) be_d2h(&m->be, info, m->routes.info, sizeof(gie_routes_info));
    return gie_sync(m);
}
extern "C" int gie_read_routes_dev(gie_mapper *m, int32_t *d_steps, uint8_t *d_cells)
{
    const int rc = gie_routes_check(m, "gie_read_routes_dev", true); if (rc) return rc;
    if (!d_steps && !d_cells) { gie_set_err("gie_read_routes_dev: both outputs null"); return GIE_ERR_INVALID; }
    const gie_routes_dev s = gie_routes_view(m);
    const int cells = s.nx * s.ny * s.nz;
    if (d_steps) { op_routes_copy_f op; op.f = s.f; op.out = d_steps; be_lin(&m->be, m->c, op, cells); }
    if (d_cells) { op_routes_copy_b op; op.b = s.cells; op.out = d_cells; be_lin(&m->be, m->c, op, cells); }
    return GIE_OK;
}
extern "C" int gie_read_routes(gie_mapper *m, int32_t *steps, uint8_t *cells)
{
    const int rc = gie_routes_check(m, "gie_read_routes", true); if (rc) return rc;
    if (!steps && !cells) { gie_set_err("gie_read_routes: both outputs null"); return GIE_ERR_INVALID; }
    const gie_routes_dev s = gie_routes_view(m);
    const size_t n = (size_t)s.nx * s.ny * s.nz;
    if (steps) be_d2h(&m->be, steps, s.f, n * 4);
    if (cells) be_d2h(&m->be, cells, s.cells, n);
    return gie_sync(m);
}
static int gie_routes_check_query(gie_mapper *m, const char *who, const float *xyz, int n, const int32_t *steps)
{
    const int rc = gie_routes_check(m, who, true); if (rc) return rc;
    if (n < 0 || (n > 0 && (!xyz || !steps))) { gie_set_err(std::string(who) + ": n < 0, or n > 0 with a null array"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_routes_query_dev(gie_mapper *m, const float *d_xyz, int n, int32_t *d_steps)
{
    const int rc = gie_routes_check_query(m, "gie_routes_query_dev", d_xyz, n, d_steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    GIE_LAUNCH(&m->be, k_routes_query, dim3((n + 255) / 256), dim3(256), 0, gie_routes_view(m), m->c.voxel_width, d_xyz, n, d_steps);
    return GIE_OK;
}
extern "C" int gie_routes_query(gie_mapper *m, const float *xyz, int n, int32_t *steps)
{
    const char *who = "gie_routes_query";
    int rc = gie_routes_check_query(m, who, xyz, n, steps); if (rc) return rc;
    if (n == 0) return GIE_OK;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 12, who);
    int32_t *dr = (int32_t *)gie_scratch(m, 1, (size_t)n * 4, who);
    if (!dx || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, dx, xyz, (size_t)n * 12);
    rc = gie_routes_query_dev(m, dx, n, dr); if (rc) return rc;
    be_d2h(&m->be, steps, dr, (size_t)n * 4);
    gie_scratch_trim(m);
    return gie_sync(m);
}
static int gie_routes_check_path(gie_mapper *m, const char *who, const float *start_xyz, int n, int max_len, const int32_t *path_key, const int32_t *len)
{
    const int rc = gie_routes_check(m, who, true); if (rc) return rc;
    if (n < 0 || max_len < 1 || (n > 0 && (!start_xyz || !path_key || !len))) { gie_set_err(std::string(who) + ": bad arguments"); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_routes_path_dev(gie_mapper *m, const float *d_start_xyz, int n, int max_len, int32_t *d_path_key, int32_t *d_len)
{
    const int rc = gie_routes_check_path(m, "gie_routes_path_dev", d_start_xyz, n, max_len, d_path_key, d_len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    GIE_LAUNCH(&m->be, k_routes_path, dim3((n + 255) / 256), dim3(256), 0, gie_routes_view(m), m->c.voxel_width, d_start_xyz, n, max_len, d_path_key, d_len);
    return GIE_OK;
}
extern "C" int gie_routes_path(gie_mapper *m, const float *start_xyz, int n, int max_len, int32_t *path_key, int32_t *len)
{
    const char *who = "gie_routes_path";
    int rc = gie_routes_check_path(m, who, start_xyz, n, max_len, path_key, len); if (rc) return rc;
    if (n == 0) return GIE_OK;
    const size_t pbytes = (size_t)n * max_len * 12;
    float *dx = (float *)gie_scratch(m, 0, (size_t)n * 12, who);
    char *dr = (char *)gie_scratch(m, 1, (size_t)n * 4 + pbytes, who);      /* lengths, then the keys */
    if (!dx || !dr) return GIE_ERR_DEVICE;
    /* only the keys the descent writes reach the caller: the device buffer takes the caller's bytes first */
    be_h2d(&m->be, dx, start_xyz, (size_t)n * 12);
    be_h2d(&m->be, dr + (size_t)n * 4, path_key, pbytes);
    rc = gie_routes_path_dev(m, dx, n, max_len, (int32_t *)(dr + (size_t)n * 4), (int32_t *)dr); if (rc) return rc;
    be_d2h(&m->be, len, dr, (size_t)n * 4);
    be_d2h(&m->be, path_key, dr + (size_t)n * 4, pbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}

/*
 * gie_blocks.inc.h — global block summaries: one record per live 8x8x8 block of the pool — how many of its voxels are FREE, OCCUPIED
 * and FNT, where its first FNT / first free voxel lies, how close the nearest obstacle comes — as a compacted list and, optionally,
 * as a dense grid of the counts over a box of blocks (include/gie.h "global block summaries").  gie_cloud_global's definition at
 * block resolution: what an exploration planner asks of the map beyond the local volume.
 * HIP backend only: included by gie_hip.hip after gie_cloud.inc.h.  It reads the map and writes nothing of it; it keeps no memory
 * of its own (a _dev call with records but no count uses the display clouds' counter word).
 *   layout           k_cloud_global's: a UNIT is eight slots of the pool, 32 lanes (half a wave) a slot, 16 consecutive bytes of the
 *                    block's types per lane (one 16-byte load: voxel j of lane `part` at x = j & 7, y = 2 (part & 3) + (j >> 3),
 *                    z = part >> 2).  A workgroup takes a fixed run of 1 to 16 units, chosen by the host from the size of the pool
 *                    (gie_cloud_iters: one unit while that leaves a workgroup for each compute unit, more beyond).  Slots at or
 *                    above min(pool_count[0], max_blocks) end at that comparison, erased slots at the key.
 *   reduction        a lane counts its 16 voxels into ONE word (three 10-bit fields: FREE, OCCUPIED, FNT — at most 16 each per lane,
 *                    at most 512 each per block, which ten bits hold) and keeps its two least stream-order indices
 *                    (x * 64 + y * 8 + z, gie_stream_changed's order) as the two 16-bit halves of another; five __shfl_xor steps
 *                    (16 .. 1: they stay inside the half wave) add the first and take the packed 16-bit minimum of the second.
 *                    GIE_BLOCKS_DIST reads the closest obstacle of FREE / FNT voxels only (gie_cloud_dist: the pair plane's for a
 *                    voxel of a tskip tile) and reduces the least valid distance the same way.
 *   grid             the slot's first lane stores its cell (every block lies in at most one cell: no atomics); the host has zeroed
 *                    the grid on the stream.
 *   compaction       the slot's first lane leaves its record (32 bytes) and a flag in LDS; after the run, lanes 0 .. 8 iters - 1
 *                    ballot the flags, the two waves' counts meet in LDS, ONE returning atomic per workgroup on the counter, none
 *                    from a workgroup without a record (a device word takes about 88 returning atomics per microsecond, DESIGN.md
 *                    17); a record is two 16-byte stores from one lane, written only while rank < max_records.
 * No grid barrier, no loop whose trip count depends on device data, no scratch.  Compiler's figures (hipcc --offload-arch=gfx950 -O3,
 * -Rpass-analysis=kernel-resource-usage) are in DESIGN.md 34.
 */

#define GIE_BLOCKS_ENTRIES (GIE_CLOUD_ITERS * GIE_CLOUD_SLOTS)      /* records of a workgroup at most */

struct gie_blocks_sel { int lo[3], hi[3], nx, ny, flags, min_fnt, max_records, iters; };

typedef unsigned short gie_blocks_us2 __attribute__((ext_vector_type(2)));
/* the minimum of both 16-bit halves at once */
GIE_DEV uint32_t gie_blocks_min2(uint32_t a, uint32_t b)
{ return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(gie_blocks_us2, a), __builtin_bit_cast(gie_blocks_us2, b))); }

template <bool DIST>
__global__ __launch_bounds__(256) void k_blocks_summary(const gie_ctx c, const gie_blocks_sel s, gie_block_summary *out, int32_t *count, uint32_t *grid)
{
    __shared__ uint4 s_rec[GIE_BLOCKS_ENTRIES][2];
    __shared__ uint8_t s_has[GIE_BLOCKS_ENTRIES];
    __shared__ int s_cnt[2], s_base;
    int bound = c.pool_count[0];
    bound = bound < c.max_blocks ? bound : c.max_blocks;
    if ((int)blockIdx.x * GIE_CLOUD_SLOTS * s.iters >= bound) return;      /* workgroup-uniform */
    const int half = threadIdx.x >> 5, part = threadIdx.x & 31;
    const int slot0 = (int)blockIdx.x * GIE_CLOUD_SLOTS * s.iters + half;
#pragma unroll 1
    for (int r = 0; r < s.iters; r++) {
        const int slot = slot0 + r * GIE_CLOUD_SLOTS;
        const uint64_t key = slot < bound ? c.g_key[slot] : GIE_KEY_EMPTY;
        const bool live = key != GIE_KEY_EMPTY;                            /* uniform over the half wave */
        int k[3] = { 0, 0, 0 };
        uint4 t = make_uint4(0u, 0u, 0u, 0u);                              /* (UNKNOWN everywhere: counts nothing) */
        const gie_vaddr a0 = (gie_vaddr)slot * GIE_VBSZ + part * 16;
        if (live) {
            gie_unpack_crd(key, &k[0], &k[1], &k[2]);
            t = *reinterpret_cast<const uint4 *>(c.g_type + a0);
        }
        uint32_t cnt = 0u, least = 0xffffffffu;                            /* FREE | OCCUPIED << 10 | FNT << 20; free_voxel | fnt_voxel << 16 */
        int dmin = 0x7fffffff;
        const int y0 = (part & 3) * 2, z = part >> 2;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t ty = gie_cloud_byte(t, j);
            const uint32_t idx = (uint32_t)((j & 7) * 64 + (y0 + (j >> 3)) * 8 + z);
            cnt += (ty == (uint32_t)GIE_VOX_FREE ? 1u : 0u) + (ty == (uint32_t)GIE_VOX_OCCUPIED ? 1u << 10 : 0u) + (ty == (uint32_t)GIE_VOX_FNT ? 1u << 20 : 0u);
            if (ty == (uint32_t)GIE_VOX_FNT) least = gie_blocks_min2(least, idx | (idx << 16));
            else if (ty == (uint32_t)GIE_VOX_FREE) least = gie_blocks_min2(least, idx | 0xffff0000u);
            if (DIST && (ty == (uint32_t)GIE_VOX_FREE || ty == (uint32_t)GIE_VOX_FNT)) {
                const int d = gie_cloud_dist(c, a0 + j, k[0] * 8 + (j & 7), k[1] * 8 + y0 + (j >> 3), k[2] * 8 + z);
                if (d >= 0 && d < GIE_CLOUD_DIST_END) dmin = d < dmin ? d : dmin;
            }
        }
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) {
            cnt += (uint32_t)__shfl_xor((int)cnt, d);
            least = gie_blocks_min2(least, (uint32_t)__shfl_xor((int)least, d));
            if (DIST) { const int o = __shfl_xor(dmin, d); dmin = o < dmin ? o : dmin; }
        }
        if (part == 0) {
            const uint32_t n_free = cnt & 0x3ffu, n_occ = (cnt >> 10) & 0x3ffu, n_fnt = cnt >> 20;
            /* a block without a known voxel is not there (its existence is not observable), a block outside the box not asked for */
            const bool in = live && cnt != 0u && k[0] >= s.lo[0] && k[0] <= s.hi[0] && k[1] >= s.lo[1] && k[1] <= s.hi[1] && k[2] >= s.lo[2] && k[2] <= s.hi[2];
            if (in && grid) grid[((k[2] - s.lo[2]) * s.ny + (k[1] - s.lo[1])) * s.nx + (k[0] - s.lo[0])] = (1u << 31) | (n_fnt << 20) | (n_occ << 10) | n_free;
            const bool rec = in && count && (int)n_fnt >= s.min_fnt;
            if (rec) {
                s_rec[r * GIE_CLOUD_SLOTS + half][0] = make_uint4((uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], n_free | (n_occ << 16));
                s_rec[r * GIE_CLOUD_SLOTS + half][1] = make_uint4(n_fnt | (least & 0xffff0000u), (least & 0xffffu) | ((uint32_t)s.flags << 16),
                                                                  (uint32_t)(DIST && dmin != 0x7fffffff ? dmin : GIE_EMPTY_VALUE), 0u);
            }
            s_has[r * GIE_CLOUD_SLOTS + half] = rec ? 1 : 0;
        }
    }
    if (!count) return;                                                    /* (the grid alone: a kernel argument) */
    __syncthreads();
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const bool has = (int)threadIdx.x < s.iters * GIE_CLOUD_SLOTS && s_has[threadIdx.x];
    const unsigned long long b = __ballot(has);
    if (lane == 0 && wave < 2) s_cnt[wave] = __popcll(b);
    __syncthreads();
    const int c0 = s_cnt[0], c1 = s_cnt[1];
    if (c0 + c1 == 0) return;                                              /* workgroup-uniform */
    if (threadIdx.x == 0) s_base = atomicAdd(count, c0 + c1);
    __syncthreads();
    if (!has) return;
    const int rank = s_base + (wave > 0 ? c0 : 0) + __popcll(b & ((1ull << lane) - 1ull));
    if (rank < s.max_records) {
        uint4 *o = reinterpret_cast<uint4 *>(out + rank);
        o[0] = s_rec[threadIdx.x][0];
        o[1] = s_rec[threadIdx.x][1];
    }
}

/* ---- host side */
static int gie_blocks_args(gie_mapper *m, const char *who, bool dev, const gie_blocks_param *p, const gie_block_summary *out, const int32_t *count, const uint32_t *grid,
                           long long *cells)
{
    static_assert(sizeof(gie_blocks_param) == 48 && sizeof(gie_block_summary) == 32, "the sizes include/gie.h states");
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    const char *bad = nullptr;
    *cells = 0;
    if (gie_tiled(m)) bad = "not for a tiled mapper (its pool holds ghost blocks of other tiles)";
    else if (!p) bad = "null parameters";
    else if (p->lo[0] > p->hi[0] || p->lo[1] > p->hi[1] || p->lo[2] > p->hi[2]) bad = "lo > hi";
    else if (p->flags != 0 && p->flags != GIE_BLOCKS_DIST) bad = "flags must be 0 or 1 (reduce the distances too)";
    else if (p->min_fnt < 0 || p->min_fnt > GIE_VBSZ) bad = "min_fnt must be 0..512";
    else if (p->max_records < 0) bad = "max_records must be >= 0";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2]) bad = "reserved must be 0";
    else if (!out && p->max_records > 0) bad = "null record buffer with max_records > 0";
    else if (!out && !count && !grid) bad = "nothing to write: all outputs null";
    else if (dev && ((uintptr_t)out & 15)) bad = "the device record buffer must be 16-byte aligned";
    else if (grid) {
        long long n = 1;
        for (int i = 0; i < 3 && !bad; i++) {
            const long long side = (long long)p->hi[i] - p->lo[i] + 1;
            if (p->lo[i] == INT32_MIN || p->hi[i] == INT32_MAX) bad = "a grid needs a finite box";
            else if (side > 1024) bad = "a grid's box has at most 1024 blocks a side";
            n *= side;
        }
        if (!bad && n > (1ll << 24)) bad = "a grid has at most 2^24 cells";
        *cells = n;
    }
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* the launch: d_count and d_grid zeroed on the stream, then written in place (arguments are checked; d_count null: no list) */
static int gie_blocks_enqueue(gie_mapper *m, const gie_blocks_param *p, gie_block_summary *d_out, int32_t *d_count, uint32_t *d_grid, long long cells)
{
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this stage) */
    gie_blocks_sel s;
    for (int i = 0; i < 3; i++) { s.lo[i] = p->lo[i]; s.hi[i] = p->hi[i]; }
    s.nx = d_grid ? p->hi[0] - p->lo[0] + 1 : 0; s.ny = d_grid ? p->hi[1] - p->lo[1] + 1 : 0;
    s.flags = p->flags; s.min_fnt = p->min_fnt; s.max_records = p->max_records;
    const long long units = ((long long)c.max_blocks + GIE_CLOUD_SLOTS - 1) / GIE_CLOUD_SLOTS;
    s.iters = gie_cloud_iters(units);
    if (d_count) be_memset(&m->be, d_count, 0, sizeof(int32_t));
    if (d_grid) be_memset(&m->be, d_grid, 0, (size_t)cells * sizeof(uint32_t));
    const dim3 g((unsigned)((units + s.iters - 1) / s.iters)), t(256);
    if (p->flags & GIE_BLOCKS_DIST) GIE_LAUNCH(&m->be, k_blocks_summary<true>, g, t, 0, c, s, d_out, d_count, d_grid);
    else GIE_LAUNCH(&m->be, k_blocks_summary<false>, g, t, 0, c, s, d_out, d_count, d_grid);
    return GIE_OK;
}
/* the host form: the counter and, 16 bytes behind it, the grid in scratch slot 0, the records in slot 1; only the written records
 * travel back, so the entries beyond them are the caller's as they were */
extern "C" int gie_blocks_summary(gie_mapper *m, const gie_blocks_param *p, gie_block_summary *out, int32_t *count, uint32_t *grid)
{
    const char *who = "gie_blocks_summary";
    long long cells = 0;
    int rc = gie_blocks_args(m, who, false, p, out, count, grid, &cells); if (rc) return rc;
    const bool list = out || count;
    char *d0 = (char *)gie_scratch(m, 0, 16 + (size_t)cells * sizeof(uint32_t), who);
    gie_block_summary *dr = p->max_records > 0 ? (gie_block_summary *)gie_scratch(m, 1, (size_t)p->max_records * sizeof(gie_block_summary), who) : nullptr;
    if (!d0 || (p->max_records > 0 && !dr)) return GIE_ERR_DEVICE;
    int32_t *dn = list ? (int32_t *)d0 : nullptr;
    uint32_t *dg = grid ? (uint32_t *)(d0 + 16) : nullptr;
    rc = gie_blocks_enqueue(m, p, dr, dn, dg, cells); if (rc) return rc;
    if (list) {
        int32_t n = 0;
        be_d2h(&m->be, &n, dn, sizeof(int32_t));
        if (count) *count = n;
        const int32_t nw = n < p->max_records ? n : p->max_records;
        if (nw > 0) be_d2h(&m->be, out, dr, (size_t)nw * sizeof(gie_block_summary));
    }
    if (grid) be_d2h(&m->be, grid, dg, (size_t)cells * sizeof(uint32_t));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_blocks_summary_dev(gie_mapper *m, const gie_blocks_param *p, gie_block_summary *d_out, int32_t *d_count, uint32_t *d_grid)
{
    const char *who = "gie_blocks_summary_dev";
    long long cells = 0;
    const int rc = gie_blocks_args(m, who, true, p, d_out, d_count, d_grid, &cells); if (rc) return rc;
    if (!d_count && d_out) {                                    /* records without a count: the ranks still need a counter */
        if (!m->cloud_count) m->cloud_count = gie_dalloc<int32_t>(m, 4, false);
        if (!m->cloud_count) { gie_set_err(std::string(who) + ": device allocation of the counter failed"); return GIE_ERR_DEVICE; }
        d_count = m->cloud_count;
    }
    return gie_blocks_enqueue(m, p, d_out, d_count, d_grid, cells);
}

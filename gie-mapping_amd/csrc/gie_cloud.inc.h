/*
 * gie_cloud.inc.h — display clouds: the selected voxels of the local volume, or of every live block of the pool, compacted into
 * (x, y, z, intensity) records on the device (include/gie.h "display clouds"): VOLMAPNODE::visualize's four loops
 * (include/volumetric_mapper.h:181-357) without the CPU mirror.
 * HIP backend only: included by gie_hip.hip after gie_path.inc.h.  It reads the map and writes nothing of it; the only memory it
 * keeps is one counter word, allocated at the first _dev call that passes no count.
 *   layout           a UNIT is 4096 voxels: 16 that lie next to each other in memory for each of a workgroup's 256 lanes (one
 *                    16-byte load of types) — eight slots of the pool (32 lanes a slot, 4 lanes = 64 bytes a z layer of a block), or
 *                    4096 consecutive voxels of the local type plane.  A workgroup takes a fixed run of 1 to 16 units, chosen by
 *                    the host from the size of the pool / of the band: one unit while that leaves a workgroup for each of the 256
 *                    compute units, more beyond — because of the counter, below.  Two cases stay at one: the global form with a
 *                    band of at most eight layers (few of its workgroups have points) and the local distance cloud (every
 *                    workgroup has points, and their stores hide the atomics).
 *   k_cloud_global   slots at or above min(pool_count[0], max_blocks) end at that comparison, erased slots at the key, a z layer
 *                    outside the band before its types are loaded: a one-layer slice reads one key and 64 bytes per block.
 *                    GIE_CLOUD_TYPE reads nothing else; GIE_CLOUD_DIST reads the closest obstacle (the pair plane's for a voxel of a
 *                    tskip tile: gie_deferred_coc, gie_query_voxel's two cases) of the voxels that passed mask and band.
 *   k_cloud_local    the host clips the band to z planes, the launch covers those planes only.  X a multiple of 16 and an aligned
 *                    plane: 16-byte loads, a lane's voxels share a row; otherwise byte loads, voxel j of a lane at 256 j + lane
 *                    (coalesced).  gie_edt_value for written records only.
 *   compaction       two passes over the workgroup's units.  The first leaves every lane's 16-bit selection mask of every unit in
 *                    LDS (8 KB) and counts; the four waves' counts meet in LDS; ONE returning atomic per workgroup on the counter,
 *                    none from a workgroup without points.  The second pass ballots the masks, bit by bit: voxel j of consecutive
 *                    lanes goes to consecutive records (coalesced 16-byte stores), each written only while rank < max_points, its
 *                    position and intensity computed then (the bytes it looks at again were read by the same workgroup a moment
 *                    before).  A device word takes about 88 returning atomics per microsecond: the OCCUPIED cloud of a 512^3
 *                    map has points in nearly every unit, 40 k atomics (450 us) at a unit per workgroup, 2 500 (28 us) at 16;
 *                    against that, a unit's loads depend on each other (key, types, obstacles) and the units of a run pay those
 *                    latencies one after the other.
 * No grid barrier, no loop whose trip count depends on device data.  Compiler's figures (hipcc --offload-arch=gfx950 -O3,
 * -Rpass-analysis=kernel-resource-usage) are in DESIGN.md 17.
 */

#define GIE_CLOUD_SLOTS 8               /* slots per unit of k_cloud_global */
#define GIE_CLOUD_UNIT 4096             /* voxels of a unit: 16 for each of a workgroup's 256 lanes (both kernels) */
#define GIE_CLOUD_ITERS 16              /* units per workgroup at most */
#define GIE_CLOUD_DIST_END 900000       /* the reference's invalid_dist_glb (voxmap_utils.cuh:162-165): its literal, not GIE_EMPTY_VALUE */

struct gie_cloud_sel { uint32_t mask; int z_lo, z_hi, max_points, iters; float w; };
/* units per workgroup: one while that leaves a workgroup for every compute unit, then more — the counter takes one atomic per workgroup */
static int gie_cloud_iters(long long units) { const long long i = (units + 255) / 256; return i < 1 ? 1 : (i > GIE_CLOUD_ITERS ? GIE_CLOUD_ITERS : (int)i); }

GIE_DEV bool gie_cloud_type_on(const gie_cloud_sel &s, uint32_t ty) { return ty < 4u && ((s.mask >> ty) & 1u); }
GIE_DEV uint32_t gie_cloud_byte(const uint4 &t, int j)
{
    const uint32_t wd = (j >> 2) == 0 ? t.x : ((j >> 2) == 1 ? t.y : ((j >> 2) == 2 ? t.z : t.w));
    return (wd >> (8 * (j & 3))) & 0xffu;
}
/* the intensity of a type cloud: a mask of one type needs no second look at the voxel */
GIE_DEV float gie_cloud_type_value(const gie_cloud_sel &s, const int8_t *ty) { return (s.mask & (s.mask - 1u)) ? (float)*ty : (float)(__ffs((int)s.mask) - 1); }

/* A workgroup's units into out / count, called by all 256 lanes.  select(r): bit j = voxel j of the lane in unit r is selected;
 * record(r, j, g, v): its global voxel and intensity (called for records that are written only).  First pass: the masks into LDS
 * and the wave's count; one returning atomic for the workgroup; second pass: the ballots of the same masks give every record its
 * rank, voxel j of consecutive lanes consecutive records. */
template <class SEL, class REC>
GIE_DEV void gie_cloud_workgroup(const gie_cloud_sel &s, const SEL &select, const REC &record, gie_cloud_point *out, int32_t *count)
{
    __shared__ uint16_t s_sel[GIE_CLOUD_ITERS][256];
    __shared__ int s_cnt[4], s_base;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    int total = 0;
#pragma unroll 1
    for (int r = 0; r < s.iters; r++) {
        const uint32_t sel = select(r);
        s_sel[r][threadIdx.x] = (uint16_t)sel;
        total += __popc(sel);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d);
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], c3 = s_cnt[3];
    if (c0 + c1 + c2 + c3 == 0) return;                       /* workgroup-uniform */
    if (threadIdx.x == 0) s_base = atomicAdd(count, c0 + c1 + c2 + c3);
    __syncthreads();
    if (total == 0) return;                                    /* wave-uniform */
    int rank = s_base + (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
    if (rank >= s.max_points) return;                          /* wave-uniform: nothing of this wave fits any more */
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (int r = 0; r < s.iters; r++) {
        const uint32_t sel = s_sel[r][threadIdx.x];
        if (!__ballot(sel != 0u)) continue;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const bool on = (sel >> j) & 1u;
            const unsigned long long b = __ballot(on);
            if (on) {
                const int q = rank + __popcll(b & below);
                if (q < s.max_points) {
                    int g[3];
                    float v;
                    record(r, j, g, &v);
                    *reinterpret_cast<float4 *>(&out[q]) = make_float4((float)g[0] * s.w, (float)g[1] * s.w, (float)g[2] * s.w, v);
                }
            }
            rank += __popcll(b);
        }
    }
}

/* the closest obstacle's distance^2 as gie_query_voxel reports it: the pair plane's for a voxel of a tskip tile */
GIE_DEV int gie_cloud_dist(const gie_ctx &c, gie_vaddr a, int gx, int gy, int gz)
{
    uint64_t cc;
    if (!gie_deferred_coc(c, gx, gy, gz, &cc)) cc = c.g_coc[a];
    return gie_gdist(c, cc, gx, gy, gz);
}

template <bool DIST>
__global__ __launch_bounds__(256) void k_cloud_global(const gie_ctx c, const gie_cloud_sel s, gie_cloud_point *out, int32_t *count)
{
    int bound = c.pool_count[0];
    bound = bound < c.max_blocks ? bound : c.max_blocks;
    const int slot0 = (int)blockIdx.x * GIE_CLOUD_SLOTS * s.iters + (int)(threadIdx.x >> 5), part = threadIdx.x & 31;
    if ((int)blockIdx.x * GIE_CLOUD_SLOTS * s.iters >= bound) return;      /* workgroup-uniform */
    /* unit r: slot slot0 + 8 r; the lane's 16 voxels are bytes [16 part, 16 part + 16) of the block: voxel j at (j & 7, 2 (part & 3) + (j >> 3), part >> 2) */
    const auto first = [&](int slot, int *g0) -> bool {
        const uint64_t key = slot < bound ? c.g_key[slot] : GIE_KEY_EMPTY;
        if (key == GIE_KEY_EMPTY) return false;
        int k[3];
        gie_unpack_crd(key, &k[0], &k[1], &k[2]);
        g0[0] = k[0] * 8; g0[1] = k[1] * 8 + (part & 3) * 2; g0[2] = k[2] * 8 + (part >> 2);
        return g0[2] >= s.z_lo && g0[2] <= s.z_hi;
    };
    gie_cloud_workgroup(s, [&](int r) -> uint32_t {
        const int slot = slot0 + r * GIE_CLOUD_SLOTS;
        int g0[3];
        if (!first(slot, g0)) return 0u;
        const gie_vaddr a0 = (gie_vaddr)slot * GIE_VBSZ + part * 16;
        const uint4 t = *reinterpret_cast<const uint4 *>(c.g_type + a0);
        uint32_t sel = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (!gie_cloud_type_on(s, gie_cloud_byte(t, j))) continue;
            if (DIST) {
                const int d = gie_cloud_dist(c, a0 + j, g0[0] + (j & 7), g0[1] + (j >> 3), g0[2]);
                if (d < 0 || d >= GIE_CLOUD_DIST_END) continue;
            }
            sel |= 1u << j;
        }
        return sel;
    }, [&](int r, int j, int *g, float *v) {
        const int slot = slot0 + r * GIE_CLOUD_SLOTS;
        int g0[3];
        (void)first(slot, g0);
        g[0] = g0[0] + (j & 7); g[1] = g0[1] + (j >> 3); g[2] = g0[2];
        const gie_vaddr a = (gie_vaddr)slot * GIE_VBSZ + part * 16 + j;
        *v = DIST ? sqrtf((float)gie_cloud_dist(c, a, g[0], g[1], g[2])) * s.w : gie_cloud_type_value(s, c.g_type + a);
    }, out, count);
}

/* ids [id0, id1) of the local volume: whole z planes (the band, clipped by the host) */
template <bool DIST, bool VEC>
__global__ __launch_bounds__(256) void k_cloud_local(const gie_ctx c, const gie_cloud_sel s, const int id0, const int id1, gie_cloud_point *out, int32_t *count)
{
    const int base = id0 + (int)blockIdx.x * GIE_CLOUD_UNIT * s.iters, plane = c.X * c.Y;
    /* voxel j of the lane in unit r.  VEC (X % 16 == 0: id0, id1 and every lane's first id are multiples of 16): 16 voxels of one
     * row behind one 16-byte load; otherwise byte loads, voxel j at 256 j + lane (coalesced) */
    const auto vid = [&](int r, int j) { return base + r * GIE_CLOUD_UNIT + (VEC ? (int)threadIdx.x * 16 + j : j * 256 + (int)threadIdx.x); };
    gie_cloud_workgroup(s, [&](int r) -> uint32_t {
        uint32_t sel = 0;
        if (VEC) {
            const int id = vid(r, 0);
            if (id >= id1) return 0u;
            const uint4 t = *reinterpret_cast<const uint4 *>(c.glb_type + id);
#pragma unroll
            for (int j = 0; j < 16; j++) if (gie_cloud_type_on(s, gie_cloud_byte(t, j))) sel |= 1u << j;
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int id = vid(r, j);
                if (id < id1 && gie_cloud_type_on(s, (uint8_t)c.glb_type[id])) sel |= 1u << j;
            }
        }
        return sel;
    }, [&](int r, int j, int *g, float *v) {
        const int id = vid(r, j), z = id / plane, q = id - z * plane, y = q / c.X;
        g[0] = q - y * c.X + c.pvt[0]; g[1] = y + c.pvt[1]; g[2] = z + c.pvt[2];
        *v = DIST ? gie_edt_value(c, id) * s.w : gie_cloud_type_value(s, c.glb_type + id);
    }, out, count);
}

/* ---- host side */
static int gie_cloud_args(gie_mapper *m, const char *who, bool local, bool dev, const gie_cloud_param *p, const gie_cloud_point *out, const int32_t *count)
{
    static_assert(sizeof(gie_cloud_param) == 32 && sizeof(gie_cloud_point) == 16, "the sizes include/gie.h states");
    if (!m) { gie_set_err(std::string(who) + ": null handle"); return GIE_ERR_INVALID; }
    const char *bad = nullptr;
    if (gie_tiled(m)) bad = "not for a tiled mapper (its pool holds ghost blocks of other tiles)";
    else if (!p) bad = "null parameters";
    else if (p->type_mask == 0 || (p->type_mask & ~((1u << GIE_VOX_FREE) | (1u << GIE_VOX_OCCUPIED) | (1u << GIE_VOX_FNT)))) bad = "type_mask must select FREE, OCCUPIED or FNT and nothing else";
    else if (p->intensity != GIE_CLOUD_TYPE && p->intensity != GIE_CLOUD_DIST) bad = "intensity must be 0 (the type) or 1 (the distance)";
    else if (p->z_lo > p->z_hi) bad = "z_lo > z_hi";
    else if (p->max_points < 0) bad = "max_points must be >= 0";
    else if (p->reserved[0] || p->reserved[1] || p->reserved[2]) bad = "reserved must be 0";
    else if (!out && p->max_points > 0) bad = "null point buffer with max_points > 0";
    else if (!out && !count) bad = "nothing to write: both outputs null";
    else if (dev && ((uintptr_t)out & 15)) bad = "the device point buffer must be 16-byte aligned";
    else if (local && !m->has_pose) bad = "gie_set_pose has not been called";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
/* the launch: d_count zeroed on the stream, then accumulated in place (arguments are checked) */
static int gie_cloud_enqueue(gie_mapper *m, const char *who, bool local, const gie_cloud_param *p, gie_cloud_point *d_out, int32_t *d_count)
{
    if (!d_count) {
        if (!m->cloud_count) m->cloud_count = gie_dalloc<int32_t>(m, 4, false);
        if (!m->cloud_count) { gie_set_err(std::string(who) + ": device allocation of the counter failed"); return GIE_ERR_DEVICE; }
        d_count = m->cloud_count;
    }
    gie_ctx c = m->c;
    c.gate = nullptr;                                           /* (a halo round's gate is no business of this stage) */
    gie_cloud_sel s;
    s.mask = p->type_mask; s.z_lo = p->z_lo; s.z_hi = p->z_hi; s.max_points = p->max_points; s.iters = 1; s.w = c.voxel_width;
    const bool dist = p->intensity == GIE_CLOUD_DIST;
    be_prof(&m->be, GIE_K_CLOUD, 0);
    be_memset(&m->be, d_count, 0, sizeof(int32_t));
    if (!local) {
        const long long units = ((long long)c.max_blocks + GIE_CLOUD_SLOTS - 1) / GIE_CLOUD_SLOTS;
        /* a band of at most eight layers meets one or two block rows: few workgroups have points, so few atomics — and a unit's loads
         * depend on each other (key, types, obstacles), so units in a row cost their latencies in a row: the one-layer DIST slice of a
         * 512^3 map takes 56 us with a unit per workgroup, 520 us with 16 */
        s.iters = (long long)p->z_hi - p->z_lo < 8 ? 1 : gie_cloud_iters(units);
        const dim3 g((unsigned)((units + s.iters - 1) / s.iters)), t(256);
        if (dist) GIE_LAUNCH(&m->be, k_cloud_global<true>, g, t, 0, c, s, d_out, d_count);
        else GIE_LAUNCH(&m->be, k_cloud_global<false>, g, t, 0, c, s, d_out, d_count);
    } else {
        const long long lo = (long long)p->z_lo - c.pvt[2], hi = (long long)p->z_hi - c.pvt[2];      /* the band in local z planes */
        const int z0 = lo < 0 ? 0 : (int)(lo < c.Z ? lo : c.Z), z1 = hi >= c.Z ? c.Z : (int)(hi < 0 ? 0 : hi + 1);
        if (z0 < z1) {
            const int plane = c.X * c.Y, id0 = z0 * plane, id1 = z1 * plane;
            const int units = (id1 - id0 + GIE_CLOUD_UNIT - 1) / GIE_CLOUD_UNIT;
            /* the distance cloud of a local volume is nearly the volume (every known voxel): every workgroup has points and 16 bytes
             * a voxel to store, which hide the atomics that longer runs would save (all of a 512^3 volume: 1.09 ms with a unit
             * per workgroup, 1.47 ms with 16) */
            s.iters = dist ? 1 : gie_cloud_iters(units);
            const dim3 g((unsigned)((units + s.iters - 1) / s.iters)), t(256);
            const bool vec = (c.X & 15) == 0 && ((uintptr_t)c.glb_type & 15) == 0;
            if (dist && vec) GIE_LAUNCH(&m->be, (k_cloud_local<true, true>), g, t, 0, c, s, id0, id1, d_out, d_count);
            else if (dist) GIE_LAUNCH(&m->be, (k_cloud_local<true, false>), g, t, 0, c, s, id0, id1, d_out, d_count);
            else if (vec) GIE_LAUNCH(&m->be, (k_cloud_local<false, true>), g, t, 0, c, s, id0, id1, d_out, d_count);
            else GIE_LAUNCH(&m->be, (k_cloud_local<false, false>), g, t, 0, c, s, id0, id1, d_out, d_count);
        }
    }
    be_prof(&m->be, GIE_K_CLOUD, 1);
    return GIE_OK;
}
/* the host forms: the counter in scratch slot 0, the records in slot 1; only the written records travel back, so the entries
 * beyond them are the caller's as they were */
static int gie_cloud_host(gie_mapper *m, const char *who, bool local, const gie_cloud_param *p, gie_cloud_point *out, int32_t *count)
{
    int rc = gie_cloud_args(m, who, local, false, p, out, count); if (rc) return rc;
    int32_t *dn = (int32_t *)gie_scratch(m, 0, 16, who);
    gie_cloud_point *dp = p->max_points > 0 ? (gie_cloud_point *)gie_scratch(m, 1, (size_t)p->max_points * sizeof(gie_cloud_point), who) : nullptr;
    if (!dn || (p->max_points > 0 && !dp)) return GIE_ERR_DEVICE;
    rc = gie_cloud_enqueue(m, who, local, p, dp, dn); if (rc) return rc;
    int32_t n = 0;
    be_d2h(&m->be, &n, dn, sizeof(int32_t));
    if (count) *count = n;
    const int32_t nw = n < p->max_points ? n : p->max_points;
    if (nw > 0) be_d2h(&m->be, out, dp, (size_t)nw * sizeof(gie_cloud_point));
    gie_scratch_trim(m);
    return gie_sync(m);
}
extern "C" int gie_cloud_local_dev(gie_mapper *m, const gie_cloud_param *p, gie_cloud_point *d_out, int32_t *d_count)
{
    const int rc = gie_cloud_args(m, "gie_cloud_local_dev", true, true, p, d_out, d_count);
    return rc ? rc : gie_cloud_enqueue(m, "gie_cloud_local_dev", true, p, d_out, d_count);
}
extern "C" int gie_cloud_global_dev(gie_mapper *m, const gie_cloud_param *p, gie_cloud_point *d_out, int32_t *d_count)
{
    const int rc = gie_cloud_args(m, "gie_cloud_global_dev", false, true, p, d_out, d_count);
    return rc ? rc : gie_cloud_enqueue(m, "gie_cloud_global_dev", false, p, d_out, d_count);
}
extern "C" int gie_cloud_local(gie_mapper *m, const gie_cloud_param *p, gie_cloud_point *out, int32_t *count)
{ return gie_cloud_host(m, "gie_cloud_local", true, p, out, count); }
extern "C" int gie_cloud_global(gie_mapper *m, const gie_cloud_param *p, gie_cloud_point *out, int32_t *count)
{ return gie_cloud_host(m, "gie_cloud_global", false, p, out, count); }

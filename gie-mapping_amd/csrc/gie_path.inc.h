/*
 * gie_path.inc.h — path shortcutting: any-angle waypoints from a polyline of voxels, over the opaque plane of the last prepare
 * (include/gie.h "path shortcutting").
 * HIP backend only: included by gie_hip.hip after gie_los.inc.h, whose plane, edt copy and walk it uses; it keeps no memory of its
 * own and nothing of the map update reads what is computed here.
 *   k_path_shortcut  a wave per path, four paths per workgroup.  The greedy step is serial, its window is parallel: with
 *                    top = min(k + K, m - 1), chunk c gives lane l the candidate j = top - 64 c - l; the lane walks L(v_k, v_j) and
 *                    leaves at its first opaque voxel; the first chunk with a clear lane decides, k' = top - 64 c - ctz(ballot),
 *                    and no later chunk is walked.  A v_k outside the volume or opaque has no clear line at all: the leg is forced
 *                    without a walk (a path that has left the volume, or lies in an inflated obstacle, costs m steps, not m * K walks).
 *                    The chosen leg's min_edt is a SECOND walk of that one line by the wave's first lane, with loads of the edt
 *                    copy.  The register count does not decide it — 54 VGPRs this way, 53 with the minimum carried in the
 *                    candidate walks, no scratch and 8 waves per SIMD either way — the loads do: carried, every step of every
 *                    lane is a scattered 4-byte load beside its bit test, for lines of which all but one are thrown away.
 *                    The first lane also keeps count, forced and length and writes the records.
 * Integers, exact float minima and one float sum in leg order: a result does not depend on scheduling.
 */

/* the local voxel of a path point (any int32: the difference in 64 bits); false outside the volume */
GIE_DEV bool gie_path_local(const gie_ctx &c, const gie_los_dev &s, const int32_t *g, int v[3])
{
    const long long x = (long long)g[0] - s.pvt[0], y = (long long)g[1] - s.pvt[1], z = (long long)g[2] - s.pvt[2];
    const bool in = x >= 0 && x < c.X && y >= 0 && y < c.Y && z >= 0 && z < c.Z;
    v[0] = in ? (int)x : 0; v[1] = in ? (int)y : 0; v[2] = in ? (int)z : 0;
    return in;
}

__global__ __launch_bounds__(256) void k_path_shortcut(const gie_ctx c, const gie_los_dev s, const int32_t *path, const int32_t *len, const int n,
                                                       const int max_len, const int K, const int max_wp, gie_waypoint *wp, gie_shortcut_info *info)
{
    const int p = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n) return;                                         /* wave-uniform */
    const int32_t *pts = path + (size_t)p * max_len * 3;
    gie_waypoint *out = wp + (size_t)p * max_wp;                /* (not touched when max_wp == 0) */
    int m = len[p];
    m = m < 0 ? 0 : (m > max_len ? max_len : m);
    int count = 0, forced = 0;
    float length = 0.f;
    if (m > 0) {
        int a[3], k = 0;
        bool ina = gie_path_local(c, s, pts, a);
        if (lane == 0 && max_wp > 0) {
            gie_waypoint r;
            r.xyz[0] = pts[0]; r.xyz[1] = pts[1]; r.xyz[2] = pts[2]; r.index = 0; r.forced = 0;
            r.min_edt = ina ? s.edt[gie_lid(c, a[0], a[1], a[2])] : -1.0f;
            out[0] = r;
        }
        count = 1;
        /* everything that steers the loops below is the same in all lanes of the wave: k, a, the ballots */
#pragma unroll 1
        while (k < m - 1) {
            int nk = -1;
            if (ina && !gie_los_opaque(c, s, a[0], a[1], a[2])) {
                const int top = m - 1 - k > K ? k + K : m - 1;
#pragma unroll 1
                for (int base = top; base > k; base -= 64) {
                    const int j = base - lane;
                    bool clear = false;
                    int b[3];
                    if (j > k && gie_path_local(c, s, pts + 3 * (size_t)j, b)) {
                        gie_los_walk w;
                        gie_los_walk_init(w, a, b);
                        int v[3] = { a[0], a[1], a[2] };
                        clear = true;
                        while (gie_los_walk_step(w, v))
                            if (gie_los_opaque(c, s, v[0], v[1], v[2])) { clear = false; break; }
                    }
                    const uint64_t bal = __ballot(clear);
                    if (bal) { nk = base - (int)__builtin_ctzll(bal); break; }
                }
            }
            const bool f = nk < 0;
            if (f) nk = k + 1;
            int b[3];
            const bool inb = gie_path_local(c, s, pts + 3 * (size_t)nk, b);
            if (lane == 0) {
                gie_waypoint r;
                r.xyz[0] = pts[3 * (size_t)nk]; r.xyz[1] = pts[3 * (size_t)nk + 1]; r.xyz[2] = pts[3 * (size_t)nk + 2];
                r.index = nk; r.forced = f ? 1 : 0; r.min_edt = -1.0f;
                if (f) forced++;
                else {
                    const int dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
                    length += sqrtf((float)(dx * dx + dy * dy + dz * dz));
                    if (count < max_wp) {                       /* (a record that is not written needs no minimum) */
                        gie_los_walk w;
                        gie_los_walk_init(w, a, b);
                        int v[3] = { a[0], a[1], a[2] };
                        float me = s.edt[gie_lid(c, v[0], v[1], v[2])];
                        while (gie_los_walk_step(w, v)) { const float e = s.edt[gie_lid(c, v[0], v[1], v[2])]; me = e < me ? e : me; }
                        r.min_edt = me;
                    }
                }
                if (count < max_wp) out[count] = r;
            }
            count++;
            k = nk; ina = inb; a[0] = b[0]; a[1] = b[1]; a[2] = b[2];
        }
    }
    if (lane == 0 && info) { gie_shortcut_info q; q.count = count; q.forced = forced; q.length = length; q.reserved = 0; info[p] = q; }
}

/* ---- host side */
static int gie_path_shortcut_args(const char *who, const int32_t *path_xyz, const int32_t *len, int n, int max_len, const gie_shortcut_param *p,
                                  const gie_waypoint *wp, const gie_shortcut_info *info)
{
    const char *bad = nullptr;
    if (!p) bad = "null parameters";
    else if (p->lookahead < 1 || p->lookahead > 4096) bad = "lookahead must be in 1..4096";
    else if (p->max_wp < 0) bad = "max_wp must be >= 0";
    else if (n < 0) bad = "n must be >= 0";
    else if (n > 0 && (max_len < 1 || !path_xyz || !len)) bad = "max_len must be >= 1 and the path buffers not null";
    else if (!wp && p->max_wp > 0) bad = "null waypoint buffer with max_wp > 0";
    else if (!wp && !info) bad = "nothing to write: both outputs null";
    if (bad) { gie_set_err(std::string(who) + ": " + bad); return GIE_ERR_INVALID; }
    return GIE_OK;
}
extern "C" int gie_path_shortcut_dev(gie_mapper *m, const int32_t *d_path_xyz, const int32_t *d_len, int n, int max_len, const gie_shortcut_param *p,
                                     gie_waypoint *d_wp, gie_shortcut_info *d_info)
{
    static_assert(sizeof(gie_shortcut_param) == 16 && sizeof(gie_waypoint) == 24 && sizeof(gie_shortcut_info) == 16, "the sizes include/gie.h states");
    int rc = gie_los_check(m, "gie_path_shortcut_dev", true); if (rc) return rc;
    rc = gie_path_shortcut_args("gie_path_shortcut_dev", d_path_xyz, d_len, n, max_len, p, d_wp, d_info); if (rc) return rc;
    if (n == 0) return GIE_OK;
    gie_ctx c = m->c;
    c.gate = nullptr;
    be_prof(&m->be, GIE_K_LOS_QUERY, 0);
    GIE_LAUNCH(&m->be, k_path_shortcut, dim3((n + 3) / 4), dim3(256), 0, c, gie_los_view(m), d_path_xyz, d_len, n, max_len, (int)p->lookahead,
               (int)p->max_wp, d_wp, d_info);
    be_prof(&m->be, GIE_K_LOS_QUERY, 1);
    return GIE_OK;
}
extern "C" int gie_path_shortcut(gie_mapper *m, const int32_t *path_xyz, const int32_t *len, int n, int max_len, const gie_shortcut_param *p,
                                 gie_waypoint *wp, gie_shortcut_info *info)
{
    int rc = gie_los_check(m, "gie_path_shortcut", true); if (rc) return rc;
    rc = gie_path_shortcut_args("gie_path_shortcut", path_xyz, len, n, max_len, p, wp, info); if (rc) return rc;
    if (n == 0) return GIE_OK;
    /* slot 0: the lengths, then the points.  Slot 1: the infos, then the waypoints — the caller's own bytes first, so that the
     * entries beyond a path's records come back as they were */
    const size_t lbytes = (size_t)n * 4, pbytes = (size_t)n * max_len * 12;
    const size_t ibytes = (size_t)n * sizeof(gie_shortcut_info), wbytes = (size_t)n * p->max_wp * sizeof(gie_waypoint);
    char *di = (char *)gie_scratch(m, 0, lbytes + pbytes, "gie_path_shortcut");
    char *dr = (char *)gie_scratch(m, 1, ibytes + wbytes, "gie_path_shortcut");
    if (!di || !dr) return GIE_ERR_DEVICE;
    be_h2d(&m->be, di, len, lbytes);
    be_h2d(&m->be, di + lbytes, path_xyz, pbytes);
    if (wbytes) be_h2d(&m->be, dr + ibytes, wp, wbytes);
    rc = gie_path_shortcut_dev(m, (const int32_t *)(di + lbytes), (const int32_t *)di, n, max_len, p, wbytes ? (gie_waypoint *)(dr + ibytes) : nullptr,
                               (gie_shortcut_info *)dr);
    if (rc) return rc;
    if (info) be_d2h(&m->be, info, dr, ibytes);
    if (wbytes) be_d2h(&m->be, wp, dr + ibytes, wbytes);
    gie_scratch_trim(m);
    return gie_sync(m);
}

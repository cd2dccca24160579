/*
 * gie_hip.hip — libgie_hip.so: the MI355X (gfx950) implementation of include/gie.h.
 *   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC gie_hip.hip -o libgie_hip.so
 * One HIP stream per mapper; a frame is a fixed sequence of kernel launches with no host
 * synchronisation inside (the reference syncs ≥12 times per frame through thrust scalars,
 * SURVEY.md §2.3).
 */
#include <cstdio>
#include <unistd.h>
#include <cstring>
#include <cstdlib>
#include <string>
#include <algorithm>
#include <vector>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rocprim/rocprim.hpp>
#include "gie_kernels.hip.h"
#include "gie_edt_plan.h"

#define GIE_NEV 8

struct be_state {
    int device;
    int num_cu;     /* workgroups of the persistent wave kernels */
    int cu_total;   /* CUs of the device */
    hipStream_t stream;
    hipEvent_t ev[GIE_NEV];
    int ev_set[GIE_NEV];
    void *scan_tmp; size_t scan_bytes;
    void *arena;                        /* GIE_ARENA_MB (placement experiments): be_arena */
    hipEvent_t copy_ev[2];              /* completion of the async D2H copies (changed-block streaming) */
    hipStream_t side;                   /* copy stream of gie_costmap_publish (created on first use) */
    hipEvent_t side_ready, side_done; int side_on, side_busy;
    /* per-kernel event profiling */
    int prof_on;
    std::vector<hipEvent_t> *pool;      /* event pool */
    std::vector<int> *pending;          /* triples (kernel id, start event idx, stop event idx) */
    int pool_used;
    int cur_id;                         /* bracket the launches currently belong to (-1: none) */
    double acc_ms[32]; int acc_n[32];
    /* the batch EDT's hint (GIE_EDT_HINT_*, gie_types.h): pinned, host-mapped words the streaming kernel of pass Z stores and be_edt
     * reads with a plain load before the next update's launches */
    volatile uint32_t *edt_hint;        /* the host's address (null: no such memory — no guess, every launch as before) */
    uint32_t *edt_hint_dev;             /* the device's */
    int edt_guess;                      /* what the last update was launched for: GIE_EDT_HINT_* */
    int edt_force;                      /* test hook: the next update's guess (GIE_EDT_HINT_*), -1: the word's */
};

struct be_arena { char *base; size_t size, top; int k; std::vector<long long> skew; };
static void gie_set_err(const std::string &s);

#define GIE_HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { gie_set_err(std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

#include <mutex>
static std::mutex g_waves_mutex;
static hipEvent_t g_waves_event[64];
static bool g_waves_event_set[64];
static int g_live_mappers[64];          /* mappers alive per device: waves launches are chained only when there is more than one */

static int be_init(be_state *b, int device, int wave_workgroups)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { gie_set_err("no HIP device visible (libgie_hip.so needs an AMD GPU; there is no CPU fallback)"); return 1; }
    if (device < 0 || device >= n) { gie_set_err("bad device_id"); return 1; }
    b->device = device;
    if (hipSetDevice(device) != hipSuccess) { gie_set_err("hipSetDevice failed"); return 1; }
    { hipDeviceProp_t pr; b->num_cu = (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 64; }
    b->cu_total = b->num_cu;
    /* the persistent wavefront grid: HALF the compute units by default, so that two mappers (or two processes) with default settings
     * fit one device side by side (160 + 160 did not, for 3 % — C5 waves 128: 0.270, 160: 0.261, 192: 0.266, 256: 0.271 ms);
     * gie_config.wave_workgroups asks for another size (bench.py: 160 on a device of its own; ranks that share a device: 192 / ranks) */
    b->num_cu = b->num_cu >= 64 ? b->num_cu / 2 : b->num_cu;
    if (wave_workgroups > 0) b->num_cu = wave_workgroups < b->cu_total ? wave_workgroups : b->cu_total;
    {   /* the waves kernel meets at a hand-rolled grid barrier: its grid must fit the device at once.  Checked here, once,
         * against the runtime's own occupancy answer (what hipLaunchCooperativeKernel would check at every launch, at
         * +15-19 us of host time each); what it cannot guard against — another PROCESS holding compute units — ends in a
         * bounded spin and GIE_ERR_TIMEOUT (include/gie.h). */
        int per_cu = 0, per_cu_c = 0;
        hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(&k_waves_ab), GIE_WAVE_THREADS, 0);
        if (oe == hipSuccess) oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_c, reinterpret_cast<const void *>(&k_waves_c), GIE_WAVE_THREADS, 0);
        if (per_cu_c < per_cu) per_cu = per_cu_c;
        if (oe != hipSuccess || per_cu < 1) {
            gie_set_err(std::string("the wavefront kernels cannot be resident on this device (occupancy query: ") + hipGetErrorString(oe) + ", " + std::to_string(per_cu) + " workgroups per compute unit)");
            (void)hipGetLastError();
            return 1;
        }
        if (b->num_cu > per_cu * b->cu_total) b->num_cu = per_cu * b->cu_total;
    }
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { gie_set_err("hipStreamCreate failed"); return 1; }
    for (int i = 0; i < GIE_NEV; i++) { GIE_HIP_OK(hipEventCreate(&b->ev[i])); b->ev_set[i] = 0; }
    b->scan_tmp = nullptr; b->scan_bytes = 0; b->arena = nullptr; b->side_on = 0; b->side_busy = 0;
    for (int i = 0; i < 2; i++) GIE_HIP_OK(hipEventCreateWithFlags(&b->copy_ev[i], hipEventDisableTiming));
    {   /* (coherent host memory: the word is visible to the host once the kernel that stored it has ended) */
        void *h = nullptr, *d = nullptr;
        b->edt_hint = nullptr; b->edt_hint_dev = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
            memset(h, 0, 64); b->edt_hint = (volatile uint32_t *)h; b->edt_hint_dev = (uint32_t *)d;
        } else { if (h) (void)hipHostFree(h); (void)hipGetLastError(); }
        b->edt_guess = GIE_EDT_HINT_NONE; b->edt_force = -1;
    }
    b->prof_on = 0; b->cur_id = -1; b->pool = new std::vector<hipEvent_t>(); b->pending = new std::vector<int>(); b->pool_used = 0;
    for (int i = 0; i < 32; i++) { b->acc_ms[i] = 0; b->acc_n[i] = 0; }
    {   /* a second mapper on this device: whatever the first one has in flight was launched unchained — let it finish once */
        std::lock_guard<std::mutex> lock(g_waves_mutex);
        if (++g_live_mappers[device & 63] == 2) (void)hipDeviceSynchronize();
    }
    return 0;
}
static void be_fini(be_state *b)
{
    { std::lock_guard<std::mutex> lock(g_waves_mutex); g_live_mappers[b->device & 63]--; }
    if (b->scan_tmp) (void)hipFree(b->scan_tmp);
    for (hipEvent_t e : *b->pool) (void)hipEventDestroy(e);
    delete b->pool; delete b->pending;
    for (int i = 0; i < GIE_NEV; i++) (void)hipEventDestroy(b->ev[i]);
    for (int i = 0; i < 2; i++) (void)hipEventDestroy(b->copy_ev[i]);
    (void)hipStreamSynchronize(b->stream);              /* (a streaming kernel still in flight stores the hint word) */
    (void)hipStreamDestroy(b->stream);
    if (b->edt_hint) { (void)hipHostFree((void *)b->edt_hint); b->edt_hint = nullptr; b->edt_hint_dev = nullptr; }
    if (b->side_on) { (void)hipStreamSynchronize(b->side); (void)hipEventDestroy(b->side_ready); (void)hipEventDestroy(b->side_done); (void)hipStreamDestroy(b->side); }
    if (b->arena) { be_arena *a = (be_arena *)b->arena; if (a->base) (void)hipFree(a->base); delete a; b->arena = nullptr; }
}
/* Placement experiments ("placement bands"): GIE_ARENA_MB=<MiB> takes ONE allocation of that size per mapper and
 * carves every plane of 64 MiB and more out of it, the k-th such plane GIE_ARENA_SKEW[k] MiB (comma list, default 0) behind the
 * 2 MiB-rounded end of the one before; smaller buffers and whatever does not fit go through hipMalloc as usual. */
static be_arena *be_arena_of(be_state *b)
{
#if !defined(GIE_TEST_HOOKS)
    (void)b; return nullptr;              /* (a measurement aid: test builds only) */
#else
    static const char *e = getenv("GIE_ARENA_MB");
    if (!e || atoll(e) <= 0) return nullptr;
    if (!b->arena) {
        be_arena *a = new be_arena();
        a->size = (size_t)atoll(e) << 20; a->top = 0; a->k = 0; a->base = nullptr;
        if (const char *sk = getenv("GIE_ARENA_SKEW")) { std::string t(sk); size_t i = 0; while (i < t.size()) { size_t j = t.find(',', i); if (j == std::string::npos) j = t.size(); a->skew.push_back(atoll(t.substr(i, j - i).c_str())); i = j + 1; } }
        if (hipMalloc((void **)&a->base, a->size) != hipSuccess) { a->base = nullptr; a->size = 0; }
        b->arena = a;
    }
    return (be_arena *)b->arena;
#endif
}
static void *be_alloc(be_state *b, size_t bytes, bool zero)
{
    void *p = nullptr;
    (void)hipSetDevice(b->device);
    be_arena *a = bytes >= ((size_t)64 << 20) ? be_arena_of(b) : nullptr;
    if (a && a->base) {
        const size_t sk = (size_t)((a->k < (int)a->skew.size() ? a->skew[a->k] : 0) << 20);
        const size_t at = ((a->top + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1)) + sk;
        if (at + bytes <= a->size) { p = a->base + at; a->top = at + bytes; a->k++; }
    }
    if (!p && hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    if (zero) GIE_HIP_OK(hipMemsetAsync(p, 0, bytes, b->stream));
    return p;
}
static void be_free(be_state *b, void *p)
{
    (void)hipStreamSynchronize(b->stream);
    be_arena *a = (be_arena *)b->arena;
    if (a && a->base && (char *)p >= a->base && (char *)p < a->base + a->size) return;      /* goes with the arena (be_fini) */
    (void)hipFree(p);
}
static void be_memset(be_state *b, void *p, int v, size_t bytes) { GIE_HIP_OK(hipMemsetAsync(p, v, bytes, b->stream)); }
static void be_h2d(be_state *b, void *d, const void *h, size_t bytes)
{   /* blocking like the reference's GPU_MEMCPY_H2D (cuda_macro.h:33): the caller may reuse h */
    GIE_HIP_OK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, b->stream));
    GIE_HIP_OK(hipStreamSynchronize(b->stream));
}
static void be_d2h(be_state *b, void *h, const void *d, size_t bytes)
{
    GIE_HIP_OK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, b->stream));
    GIE_HIP_OK(hipStreamSynchronize(b->stream));
}
/* pinned host memory + asynchronous D2H with a completion event per staging slot */
static void *be_host_alloc(be_state *b, size_t bytes) { void *p = nullptr; (void)hipSetDevice(b->device); return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
static void be_host_free(be_state *, void *p) { (void)hipHostFree(p); }
static void be_d2h_async(be_state *b, void *h, const void *d, size_t bytes, int slot)
{
    GIE_HIP_OK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, b->stream));
    GIE_HIP_OK(hipEventRecord(b->copy_ev[slot], b->stream));
}
static void be_wait(be_state *b, int slot) { GIE_HIP_OK(hipEventSynchronize(b->copy_ev[slot])); }
/* a copy that leaves the mapper's stream free: the side stream waits for what the mapper's stream has enqueued so far, copies into
 * pinned host memory and records its completion; be_side_copy_begin makes the mapper's stream wait for the copy before (its source
 * is about to be rewritten) */
static void be_side_on(be_state *b)
{
    if (b->side_on) return;
    (void)hipSetDevice(b->device);
    GIE_HIP_OK(hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking));
    GIE_HIP_OK(hipEventCreateWithFlags(&b->side_ready, hipEventDisableTiming));
    GIE_HIP_OK(hipEventCreateWithFlags(&b->side_done, hipEventDisableTiming));
    b->side_on = 1;
}
static void be_side_copy_begin(be_state *b) { be_side_on(b); if (b->side_busy) GIE_HIP_OK(hipStreamWaitEvent(b->stream, b->side_done, 0)); }
static void be_side_copy(be_state *b, void *h, const void *d, size_t bytes)
{
    be_side_on(b);
    GIE_HIP_OK(hipEventRecord(b->side_ready, b->stream));
    GIE_HIP_OK(hipStreamWaitEvent(b->side, b->side_ready, 0));
    GIE_HIP_OK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, b->side));
    GIE_HIP_OK(hipEventRecord(b->side_done, b->side));
    b->side_busy = 1;
}
static int be_side_copy_wait(be_state *b)
{
    if (!b->side_busy) return 0;
    const hipError_t e = hipEventSynchronize(b->side_done);
    if (e != hipSuccess) { gie_set_err(std::string("hipEventSynchronize: ") + hipGetErrorString(e)); return 1; }
    return 0;
}
static void *be_stream_handle(be_state *b) { return (void *)b->stream; }
static int be_sync(be_state *b)
{
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) { gie_set_err(std::string("hipStreamSynchronize: ") + hipGetErrorString(e)); return 1; }
    e = hipGetLastError();
    if (e != hipSuccess) { gie_set_err(std::string("HIP error: ") + hipGetErrorString(e)); return 1; }
    return 0;
}
/* stage boundaries (us_ogm .. us_merge of gie_frame_stats): recorded while profiling is on — every
 * event is a marker packet the next kernel has to wait for */
static void be_time(be_state *b, int i)
{
    if (!b->prof_on) { b->ev_set[i] = 0; return; }
    GIE_HIP_OK(hipEventRecord(b->ev[i], b->stream)); b->ev_set[i] = 1;
}
static void be_times(be_state *b, float *ogm, float *fuse, float *edt, float *merge)
{
    float *out[4] = { ogm, fuse, edt, merge };
    for (int k = 0; k < 4; k++) {
        float ms = 0.f;
        if (b->ev_set[2 * k] && b->ev_set[2 * k + 1] && hipEventElapsedTime(&ms, b->ev[2 * k], b->ev[2 * k + 1]) == hipSuccess) *out[k] = ms * 1000.f;
        else *out[k] = 0.f;
    }
}

/* Per-kernel timing: the start / stop events ride on the kernel's own dispatch packet
 * (hipExtLaunchKernelGGL), so a profiled map update has no marker packets between its kernels
 * (event records between the launches cost the map update +18 %) and a kernel's time is its
 * execution, as rocprofv3 reports it, without the dispatch gap. */
static int be_prof_event(be_state *b)
{
    if (b->pool_used == (int)b->pool->size()) { hipEvent_t e; GIE_HIP_OK(hipEventCreate(&e)); b->pool->push_back(e); }
    return b->pool_used++;
}
/* GIE_TRACE_LAUNCHES=1: every kernel launch is announced on stderr (process id, kernel) and waited for — the last line a
 * process prints before a device fault names the kernel */
static int be_trace_on() { static const int on = GIE_SWITCH("GIE_TRACE_LAUNCHES", 0); return on; }
#define GIE_LAUNCH(b, kern, grid, block, lds, ...) GIE_LAUNCH_AS(b, #kern, kern, grid, block, lds, __VA_ARGS__)
/* ... under the name given: the templated launchers name the instantiation (k_edt_x<8>), not the parameter (k_edt_x<CP>) */
#define GIE_LAUNCH_AS(b, name, kern, grid, block, lds, ...) do { \
        if (be_trace_on()) { fprintf(stderr, "[%d] launch %s\n", (int)getpid(), name); fflush(stderr); } \
        GIE_LAUNCH_(b, kern, grid, block, lds, __VA_ARGS__); \
        if (be_trace_on()) { hipError_t e_ = hipStreamSynchronize((b)->stream); if (e_ != hipSuccess) { fprintf(stderr, "[%d] %s: %s\n", (int)getpid(), name, hipGetErrorString(e_)); fflush(stderr); } } \
    } while (0)
/* the name of an instantiation, written only when the trace is on (a constant 0 in the product library) */
struct be_kname {
    char s[40];
    be_kname(const char *kern, int a) { s[0] = 0; if (be_trace_on()) snprintf(s, sizeof(s), "%s<%d>", kern, a); }
    be_kname(const char *kern, int a, int b, int c) { s[0] = 0; if (be_trace_on()) snprintf(s, sizeof(s), "%s<%d, %d, %d>", kern, a, b, c); }
};
#define GIE_LAUNCH_(b, kern, grid, block, lds, ...) do { \
        if ((b)->prof_on && (b)->cur_id >= 0) { \
            const int e0_ = be_prof_event(b), e1_ = be_prof_event(b); \
            hipExtLaunchKernelGGL(kern, grid, block, lds, (b)->stream, (*(b)->pool)[e0_], (*(b)->pool)[e1_], 0, __VA_ARGS__); \
            (b)->pending->push_back((b)->cur_id); (b)->pending->push_back(e0_); (b)->pending->push_back(e1_); \
        } else hipLaunchKernelGGL(kern, grid, block, lds, (b)->stream, __VA_ARGS__); \
    } while (0)
static void be_prof_resolve(be_state *b)
{
    if (b->pending->empty()) { b->pool_used = 0; return; }
    GIE_HIP_OK(hipStreamSynchronize(b->stream));
    for (size_t i = 0; i + 2 < b->pending->size(); i += 3) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, (*b->pool)[(*b->pending)[i + 1]], (*b->pool)[(*b->pending)[i + 2]]) == hipSuccess) {
            b->acc_ms[(*b->pending)[i]] += ms;
        }
    }
    b->pending->clear(); b->pool_used = 0;
}
static void be_prof(be_state *b, int id, int end)
{
    if (!b->prof_on) return;
    if (!end) {
        if (b->pool_used > 4000) be_prof_resolve(b);
        b->cur_id = id;
    } else { b->cur_id = -1; b->acc_n[id] += 1; }       /* acc_n counts brackets, acc_ms sums the kernels launched inside them */
}
static void be_prof_enable(be_state *b, int on) { be_prof_resolve(b); b->prof_on = on; b->cur_id = -1; }
static void be_prof_collect(be_state *b, float *ms, int *n, int num)
{
    be_prof_resolve(b);
    for (int i = 0; i < num; i++) { ms[i] = (float)b->acc_ms[i]; n[i] = b->acc_n[i]; b->acc_ms[i] = 0; b->acc_n[i] = 0; }
}

template <class F> static void be_vox(be_state *b, const gie_ctx &c, const F &f)
{
    dim3 blk(GIE_VOX_BX, GIE_VOX_BY, 1);
    dim3 grd((c.X + GIE_VOX_BX - 1) / GIE_VOX_BX, (c.Y + GIE_VOX_BY - 1) / GIE_VOX_BY, (c.Z + GIE_VOX_ZPER - 1) / GIE_VOX_ZPER);
    GIE_LAUNCH(b, k_voxz<F>, grd, blk, 0, c, f);
}
template <class F> static void be_lin(be_state *b, const gie_ctx &c, const F &f, int n)
{
    if (n <= 0) return;
    GIE_LAUNCH(b, k_lin<F>, dim3((n + 255) / 256), dim3(256), 0, c, f, n);
}
static void be_flush_clear(be_state *b, const gie_ctx &c, const op_pair_flush &f, int n, const gie_clear_list &l)
{
    const int nclr = gie_clear_total_wgs(l);
    GIE_LAUNCH(b, k_flush_clear, dim3(nclr + (n + 255) / 256), dim3(256), 0, c, f, n, l, nclr);
}
/* can the scan stay where it is (no be_labels: gie_fuse reads the plane itself, and k_cell_alloc where a block is missing)? */
static int be_labels_in_place_ok(const gie_ctx &c, const int8_t *labels)
{ return (c.X & 15) == 0 && !c.for_motion_planner && ((uintptr_t)labels & 15) == 0; }
static void be_labels(be_state *b, const gie_ctx &c, const int8_t *labels)
{
    if (be_labels_in_place_ok(c, labels)) {
        const int nvec = c.N >> 4;
        GIE_LAUNCH(b, k_labels16, dim3((nvec + 255) / 256), dim3(256), 0, c, labels, nvec);
    } else { op_classify_labels op; op.labels = labels; be_vox(b, c, op); }
}
static void be_clear(be_state *b, const gie_clear_list &l, const int32_t *gate = nullptr)
{
    if (l.n > 0) GIE_LAUNCH(b, k_clear, dim3(gie_clear_total_wgs(l)), dim3(256), 0, l, gate);
}
static void be_round_note(be_state *b, const gie_ctx &c, int32_t *changed, long long *stats, const int32_t *go, int end)
{
    GIE_LAUNCH(b, k_round_note, dim3(1), dim3(64), 0, c, changed, stats, go, end);
}
/* allocHashTB + block table (see k_cell_alloc) */
#define GIE_INIT_MULT 4         /* workgroups per compute unit of the block initialisation */
/* fuse_list_ntile > 0: the fuse tile list (op_fuse_list over that many tiles) is built in the block-initialisation launch */
static void be_block_alloc(be_state *b, const gie_ctx &c, int ncell, int32_t *, int clear_list, int fuse_list_ntile = 0)
{
    if (clear_list) GIE_HIP_OK(hipMemsetAsync(&c.cnt[GIE_CNT_NEWLIST], 0, sizeof(int32_t), b->stream));
    GIE_LAUNCH(b, k_cell_alloc, dim3((ncell + 255) / 256), dim3(256), 0, c, ncell);
    const int ninit = b->cu_total * GIE_INIT_MULT;
    int nfl = (fuse_list_ntile + 255) / 256; if (nfl > 2 * b->cu_total) nfl = 2 * b->cu_total;
    GIE_LAUNCH(b, k_block_init_list, dim3(ninit + nfl), dim3(256), 0, c, ninit, fuse_list_ntile);
}
static void be_free_rays(be_state *b, const gie_ctx &c, const float *g, int n)
{
    if (n <= 0) return;
    GIE_LAUNCH(b, k_free_rays, dim3((n + 63) / 64), dim3(64 * GIE_RAY_SEGS), 0, c, g, n, gie_ray_max_steps(c));
}
static void be_exclusive_scan(be_state *b, const int32_t *flag, int32_t *rank, int n)
{
    size_t bytes = 0;
    (void)hipSetDevice(b->device);
    GIE_HIP_OK(rocprim::exclusive_scan(nullptr, bytes, flag, rank, 0, (size_t)n, rocprim::plus<int32_t>(), b->stream));
    if (bytes > b->scan_bytes) {
        if (b->scan_tmp) { (void)hipStreamSynchronize(b->stream); (void)hipFree(b->scan_tmp); }
        GIE_HIP_OK(hipMalloc(&b->scan_tmp, bytes)); b->scan_bytes = bytes;
    }
    GIE_HIP_OK(rocprim::exclusive_scan(b->scan_tmp, bytes, flag, rank, 0, (size_t)n, rocprim::plus<int32_t>(), b->stream));
}

/* The batch EDT's launchers: what they launch, and whether, is gie_edt_plan_for's (gie_edt_plan.h).  A CP value of the plan to its instantiation: */
#define BE_EDT_CP(cp, fn, ...) do { switch (cp) { case 1: fn<1>(__VA_ARGS__); break; case 2: fn<2>(__VA_ARGS__); break; case 4: fn<4>(__VA_ARGS__); break; \
                                                  case 8: fn<8>(__VA_ARGS__); break; default: fn<16>(__VA_ARGS__); break; } } while (0)
/* pass X; p.x_zs: the fused streaming form of pass Z may take the volume — when it does the launch returns at once */
template <int CP> static void be_edt_x(be_state *b, const gie_ctx &c, const gie_edt_plan &p, int full)
{ GIE_LAUNCH_AS(b, be_kname("k_edt_x", CP).s, k_edt_x<CP>, dim3(p.x_grid[0], p.x_grid[1]), dim3(64 * GIE_EDTX_WAVES), 0, c, p.x_zs, full); }
/* ... only the rows of the slabs that form gave up */
template <int CP> static void be_edt_x_redo(be_state *b, const gie_ctx &c, const gie_edt_plan &p)
{ GIE_LAUNCH_AS(b, be_kname("k_edt_x_redo", CP).s, k_edt_x_redo<CP>, dim3(p.redo_grid), dim3(64 * GIE_EDTX_WAVES), 0, c); }
/* the column kernel of pass Z */
template <int CP> static void be_edt_column(be_state *b, const gie_ctx &c, const gie_edt_plan &p, int full)
{
    static bool attr_done = false;
    if (!attr_done) {
        GIE_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_edt_z<CP, GIE_EDTZ_TX, GIE_EDTZ_WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, GIE_LDS_BYTES));
        attr_done = true;
    }
    GIE_LAUNCH_AS(b, be_kname("k_edt_z", CP, GIE_EDTZ_TX, GIE_EDTZ_WAVES).s, (k_edt_z<CP, GIE_EDTZ_TX, GIE_EDTZ_WAVES>), dim3(p.col_grid), dim3(64 * GIE_EDTZ_WAVES), (size_t)p.col_lds, c, p.col_ntx, p.col_ntiles, full);
}
/* adaptive sweep (k_voxa): the kernel walks the list or sweeps the volume, whichever the list's
 * length calls for; staged = the functor's load1/load2/finish form; always_list = never sweep */
/* mode: 0 = the kernel walks its list or sweeps the volume (decided on the device), 1 = always the list,
 * 2 = the list or nothing (the dense form is a block-row kernel launched next to this one) */
/* workgroups per compute unit: 8 / 16 / 32 / 64 measured 0.33 / 0.27 / 0.25 / 0.25 ms for Mark on a densely known
 * volume (sweep side); the list side does not care */
#define GIE_VOXA_MULT 32
template <bool STAGED, class F> static void be_vox_list(be_state *b, const gie_ctx &c, const F &f, const int32_t *list, int count_idx, int always_list)
{
    GIE_LAUNCH(b, (k_voxa<F, STAGED>), dim3(b->cu_total * GIE_VOXA_MULT), dim3(256), 0, c, f, list, count_idx, always_list);
}
/* Mark + commit as one sweep: its own kernel (k_markc) */
#define GIE_MARKC_MULT 64       /* workgroups per compute unit of the dense sweep: 16 / 32 / 48 / 64 / 96 / 128 measured 1.00 / 0.80 / 0.78 / 0.76 / 0.78 / 0.79 ms at 512^3 (round 4; 64 = exactly four virtual workgroups each) */
#define GIE_MARKC_LAZY_MULT 40  /* ... of the lazy walk (5 / 10 / 20 / 40 / 64 / 96 per compute unit: 0.193 / 0.186 / 0.178 / 0.174 / 0.179 / 0.180 ms on the headline — a wave per swept tile, no second tile behind it) */
static void be_markc(be_state *b, const gie_ctx &c, const int32_t *list)
{
    /* with lazy tiles the kernel walks the swept tiles, a wave each (k_markc): a grid that is resident at once */
    const dim3 g(b->cu_total * ((c.coc_defer && c.lazy_ok) ? GIE_MARKC_LAZY_MULT : GIE_MARKC_MULT)), t(256);
    GIE_LAUNCH(b, k_markc, g, t, 0, c, list);
}
/* placement probe (k_place_probe) on the Mark + commit sweep's own grid: median of `reps` timed launches, ms */
static float be_place_probe(be_state *b, const gie_ctx &c, int reps, int streams = 15)
{
    const long long ntile = (long long)c.tfd[0] * c.tfd[1] * c.tfd[2];
    const int nslot = (int)(ntile < c.max_blocks ? ntile : c.max_blocks);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
    std::vector<float> ms;
    hipLaunchKernelGGL(k_place_probe, dim3(b->cu_total * GIE_MARKC_MULT), dim3(256), 0, b->stream, c, nslot, streams);      /* warm-up: page tables, clocks */
    for (int r = 0; r < reps; r++) {
        (void)hipEventRecord(e0, b->stream);
        hipLaunchKernelGGL(k_place_probe, dim3(b->cu_total * GIE_MARKC_MULT), dim3(256), 0, b->stream, c, nslot, streams);
        (void)hipEventRecord(e1, b->stream);
        (void)hipEventSynchronize(e1);
        float t = 0.f; (void)hipEventElapsedTime(&t, e0, e1); ms.push_back(t);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    std::sort(ms.begin(), ms.end());
    GIE_HIP_OK(hipMemsetAsync(c.pair, 0, (size_t)c.N * sizeof(uint64_t), b->stream));
    return ms.empty() ? -1.f : ms[ms.size() / 2];
}
/* fuse: one launch — the kernel walks its tile list (a wave per tile) or sweeps the volume by block rows, whichever the list's
 * length calls for */
#define GIE_ROWS_MULT 32        /* 8 / 16 / 32 / 48 workgroups per compute unit: 0.225 / 0.215 / 0.195 / 0.19 ms at 512^3 (round 4: with the byte-parallel filter the kernel is short enough for the tail of its last workgroups to show; 32 = one virtual wavefront per wavefront) */
static void be_fuse(be_state *b, const gie_ctx &c, const int32_t *list)
{
    if (c.pntcld_mode) GIE_LAUNCH(b, k_fuse_rows<true>, dim3(b->cu_total * GIE_ROWS_MULT), dim3(256), 0, c, op_fuse(), list);
    else GIE_LAUNCH(b, k_fuse_rows<false>, dim3(b->cu_total * GIE_ROWS_MULT), dim3(256), 0, c, op_fuse(), list);
}
/* obtainFrontiers: the voxels on the six faces of the volume one per lane (an 8x8 patch per wave) with the tile summary + tile
 * list in the first workgroups of the same launch, then a wave per listed tile for the voxels off the faces (tile + halo
 * staged in LDS) */
static void be_frontier_tiles(be_state *b, const gie_ctx &c, const int32_t *known, int known_idx, const int32_t *list, int count_idx)
{
    gie_face_patches fp;
    const int da[6] = { c.Y, c.Y, c.X, c.X, c.X, c.X }, db[6] = { c.Z, c.Z, c.Z, c.Z, c.Y, c.Y };
    fp.off[0] = 0;
    for (int f = 0; f < 6; f++) { fp.na[f] = (da[f] + 7) / 8; fp.off[f + 1] = fp.off[f] + fp.na[f] * ((db[f] + 7) / 8); }
    const long long ntile = (long long)c.tfd[0] * c.tfd[1] * c.tfd[2];
    int nsum = (int)((ntile + 64 * GIE_FF_WAVES - 1) / (64 * GIE_FF_WAVES));
    if (nsum > 2 * b->cu_total) nsum = 2 * b->cu_total;
    const int nface = (fp.off[6] + GIE_FF_WAVES - 1) / GIE_FF_WAVES;
    /* (tried in round 4: the face voxels on a side stream next to the tiles, forked and joined with events — 2.352 against 2.352 ms per
     * C5 update: what the overlap saves the two stream hand-overs cost) */
    GIE_LAUNCH(b, k_frontier_faces, dim3(nsum + nface), dim3(64 * GIE_FF_WAVES), 0, c, fp, known, known_idx, nsum);
    static int mult = 0;
    if (mult <= 0) {    /* as many workgroups as are resident at once: every wave walks the same share of the list (a second round of workgroups would start when the first is done) */
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&mult, reinterpret_cast<const void *>(&k_frontier_tiles), 64 * GIE_FR_WAVES, 0) != hipSuccess || mult < 1) mult = 2;
    }
    GIE_LAUNCH(b, k_frontier_tiles, dim3(b->cu_total * mult), dim3(64 * GIE_FR_WAVES), 0, c, list, count_idx);
}
/* tskip for this update; with c.catchup_fast the tiles whose deferred records have to be stored are listed and stored (pupvt: the
 * wave-range pivot of the update that left them) */
static void be_tile_oldskip(be_state *b, const gie_ctx &c, const int pupvt[3])
{
    const int ntile = c.tfd[0] * c.tfd[1] * c.tfd[2];
    /* the list lives in wave C's tile list (ntile words, not in use between two merges), its length in a spare counter */
    int32_t *const count = &c.cnt[GIE_CNT_STATE1];        /* (zero: the frame clear) */
    GIE_LAUNCH(b, k_tile_oldskip, dim3((ntile + 255) / 256), dim3(256), 0, c, ntile, c.wc_list[0], count);
    if (c.catchup_fast) GIE_LAUNCH(b, k_coc_catchup_new, dim3(b->cu_total * 8), dim3(256), 0, c, pupvt[0], pupvt[1], pupvt[2], c.wc_list[0], count);
}
/* "lazy pairs": the flagged tiles that will not stay flagged get their pairs into the plane (gie_fuse) */
static void be_pair_materialise(be_state *b, const gie_ctx &c, int stay)
{
    const int ntile = c.tfd[0] * c.tfd[1] * c.tfd[2];
    /* the list lives in wave C's second tile list (ntile words, not in use between two merges), its length in a spare counter (zero: the frame clear) */
    int32_t *const count = &c.cnt[GIE_CNT_STATE2];
    GIE_LAUNCH(b, k_pair_lazy_list, dim3((ntile + 255) / 256), dim3(256), 0, c, ntile, stay, c.wc_list[1], count);
    GIE_LAUNCH(b, k_pair_lazy_run, dim3(b->cu_total * 8), dim3(256), 0, c, c.wc_list[1], count);
}
static void be_coc_catchup(be_state *b, const gie_ctx &c, const gie_catchup &p)
{
    const int ntile = c.tfd[0] * c.tfd[1] * c.tfd[2];
    /* the list lives in wave C's tile list (ntile words, not in use between two merges), its length in a spare counter */
    int32_t *const count = &c.cnt[GIE_CNT_STATE1];
    GIE_HIP_OK(hipMemsetAsync(count, 0, sizeof(int32_t), b->stream));
    GIE_LAUNCH(b, k_coc_catchup_list, dim3((ntile + 255) / 256), dim3(256), 0, c, p, ntile, c.wc_list[0], count);
    GIE_LAUNCH(b, k_coc_catchup_run, dim3(b->cu_total * 4), dim3(256), 0, c, p, c.wc_list[0], count);
}
static void be_edt_prep(be_state *b, const gie_ctx &c)
{
    const int ncol = c.tfd[0] * c.tfd[1];
    GIE_LAUNCH(b, k_edt_prep, dim3((ncol + GIE_PREP_WAVES - 1) / GIE_PREP_WAVES), dim3(64 * GIE_PREP_WAVES), 0, c, ncol);
}
/* The guess for the update about to be launched: a plain load of the hint word — no copy, no event, no wait.  The word is the last
 * update's only if the host has waited for that update since; otherwise it is an older one's or 0, and the guess is that much
 * worse.  GIE_EDT_HINT=0 (test build): no guess, the launches of before. */
static int be_edt_hint_take(be_state *b)
{
    static const int on = GIE_SWITCH("GIE_EDT_HINT", 1);
    if (!b->edt_hint) return GIE_EDT_HINT_NONE;
    const int out = (int)(b->edt_hint[0] & 3u);
    int guess = (on && (out == GIE_EDT_HINT_LEFT || out == GIE_EDT_HINT_TOOK)) ? out : GIE_EDT_HINT_NONE;
    if (b->edt_force >= 0) { guess = b->edt_force; b->edt_force = -1; }
    b->edt_guess = guess;
    return guess;
}
#if defined(GIE_TEST_HOOKS)
/* gie_debug_edt_hint: the next update's guess (GIE_EDT_HINT_*; anything else: the word's again); info[4], if asked for: the word, the
 * two counts of wrong guesses, what the last update was launched for — current once the caller has waited for the stream */
static void be_edt_hint_debug(be_state *b, int force, int32_t *info)
{
    b->edt_force = (force >= GIE_EDT_HINT_NONE && force <= GIE_EDT_HINT_TOOK) ? force : -1;
    if (info) { for (int i = 0; i < 3; i++) info[i] = b->edt_hint ? (int32_t)b->edt_hint[i] : 0; info[3] = b->edt_guess; }
}
#endif
static int be_zs_fused_switch() { static const int on = GIE_SWITCH("GIE_ZS_FUSED", 1); return on; }
/* the launches the plan lists, in their order: pass Y, pass X, then pass Z — the streaming form (dense fields: it does the whole pass and flags what it could not
 * finish for the column kernel; few known tiles: the list form, in the same launch), the list form on its own, k_edt_x_redo, the column kernel (the rest, or the repair).
 * (no launch, no bracket: the profile lists a stage by the brackets it has counted; a completion is not part of the profile) */
static void be_edt_run(be_state *b, const gie_ctx &c, int full, int guess, int completion)
{
    const gie_edt_plan p = gie_edt_plan_for(c.X, c.Y, c.Z, b->cu_total, full, guess, completion, be_zs_fused_switch());
    const dim3 gy(p.y_grid), by(p.y_block[0], p.y_block[1]);
    if (p.y_kernel != GIE_EDT_Y_NONE) be_prof(b, GIE_K_EDT_Y, 0);
    switch (p.y_kernel) {
    case GIE_EDT_Y4_16: GIE_LAUNCH(b, k_edt_y4<16>, gy, by, 0, c); break;
    case GIE_EDT_Y4_32: GIE_LAUNCH(b, k_edt_y4<32>, gy, by, 0, c); break;
    case GIE_EDT_Y_8_8: GIE_LAUNCH(b, (k_edt_y<8, 8>), gy, by, 0, c); break;
    case GIE_EDT_Y_16_16: GIE_LAUNCH(b, (k_edt_y<16, 16>), gy, by, 0, c); break;
    case GIE_EDT_Y_32_16: GIE_LAUNCH(b, (k_edt_y<32, 16>), gy, by, 0, c); break;
    }
    if (p.y_kernel != GIE_EDT_Y_NONE) be_prof(b, GIE_K_EDT_Y, 1);
    if (p.x) { be_prof(b, GIE_K_EDT_X, 0); BE_EDT_CP(p.cp_x, be_edt_x, b, c, p, full); be_prof(b, GIE_K_EDT_X, 1); }
    if (!completion) be_prof(b, GIE_K_EDT_Z, 0);
    uint32_t *const hint = p.stream_note ? b->edt_hint_dev : nullptr;
    if (p.stream && p.stream_fused) GIE_LAUNCH(b, k_edt_z_stream<true>, dim3(p.stream_grid), dim3(256), 0, c, full, p.nseg, p.seg_len, p.zs, p.guess, hint);
    else if (p.stream) GIE_LAUNCH(b, k_edt_z_stream<false>, dim3(p.stream_grid), dim3(256), 0, c, full, p.nseg, p.seg_len, p.zs, p.guess, hint);
    if (p.direct) GIE_LAUNCH(b, k_edt_z_direct, dim3(p.direct_grid), dim3(256), 0, c);
    if (p.redo) BE_EDT_CP(p.cp_x, be_edt_x_redo, b, c, p);
    BE_EDT_CP(p.cp_z, be_edt_column, b, c, p, full);
    if (!completion) be_prof(b, GIE_K_EDT_Z, 1);
}
/* EDT_OCC::batchEDTUpdate, local_edt.cu:7-28.  full = 1: whole volume; 0: only where Mark reads.  The guess is taken where it counts */
static void be_edt(be_state *b, const gie_ctx &c, int full)
{
    const int guess = gie_edt_zs_host(c.X, c.Z, be_zs_fused_switch()) == 2 ? be_edt_hint_take(b) : GIE_EDT_HINT_NONE;
    be_edt_run(b, c, full, guess, 0);
}
/* pass Z again over the whole volume (pass Y is complete, pass X where the streaming form does not take the volume) */
static void be_edt_z(be_state *b, const gie_ctx &c, int full) { be_edt_run(b, c, full, GIE_EDT_HINT_NONE, 1); }
/* waves A, B and C in one launch; workgroups are co-resident by construction (512 threads and ≈ 151 KB of LDS each:
 * at most one per compute unit).  The frame clear has zeroed the barrier word and the per-level
 * arrays; a second launch inside the same map update (gie_refine) clears them itself. */
/* The waves kernel synchronises its workgroups with a grid barrier, so ALL of them have to be
 * resident at once.  One launch is (128 workgroups on 256 compute units); two launches from
 * different mappers on the same device at the same time need not be.  Waves launches of one
 * device are therefore chained through an event: a launch waits for the previous one, whichever
 * mapper (stream) it came from. */
/* every grid-barrier launch of the library joins that chain (the waves; the navigation function's propagation, gie_nf1.inc.h; the cost matrix's, gie_costmat.inc.h):
 * `enqueue` puts the chained work on b->stream */
template <class F> static void be_chained(be_state *b, const F &enqueue)
{
    std::lock_guard<std::mutex> lock(g_waves_mutex);
    const int dv = b->device & 63;
    (void)hipSetDevice(b->device);
    const bool chain = g_live_mappers[dv] > 1;       /* a lone mapper's launches follow each other on its stream anyway (an event is a marker packet the next kernel waits for) */
    if (chain) {
        if (g_waves_event_set[dv]) GIE_HIP_OK(hipStreamWaitEvent(b->stream, g_waves_event[dv], 0));
        else { GIE_HIP_OK(hipEventCreateWithFlags(&g_waves_event[dv], hipEventDisableTiming)); g_waves_event_set[dv] = true; }
    }
    enqueue();
    if (chain) GIE_HIP_OK(hipEventRecord(g_waves_event[dv], b->stream));
}
static void be_waves(be_state *b, const gie_ctx &c, int with_ab, int record_seeds, int clear_first)
{
    be_chained(b, [&]() {
        if (clear_first) {
            GIE_HIP_OK(hipMemsetAsync(&c.cnt[GIE_CNT_BAR_B], 0, 2 * sizeof(int32_t), b->stream));      /* (BAR_B, BAR_C: the barrier words of the two launches) */
            GIE_HIP_OK(hipMemsetAsync(c.lvl_next, 0, 2 * GIE_MAX_LEVELS * sizeof(int32_t), b->stream));
        }
        if (with_ab) GIE_LAUNCH(b, k_waves_ab, dim3(b->num_cu), dim3(GIE_WAVE_THREADS), 0, c);
        GIE_LAUNCH(b, k_waves_c, dim3(b->num_cu), dim3(GIE_WAVE_THREADS), 0, c, with_ab, record_seeds);
    });
}

#include "gie_api.inc.h"
#if defined(GIE_TEST_HOOKS)
/* test hook (not in gie.h; this backend's alone — the sequential one under tests/emu has no launches to guess for): the guess the
 * NEXT gie_batch_edt launches its passes for — 0 none (pass X and k_edt_x_redo both), 1 "the streaming form did not take the last
 * volume", 2 "the fused form took it" (GIE_EDT_HINT_*, be_edt); anything else: the device's word again, as the updates after the
 * next one do anyway.  A race makes the real hint harmless and untestable; this makes every guess meet every kind of update.
 * info (null, or 4 words): the hint word of the last update that has ended (bits 0-1 its outcome, the rest its planes with
 * obstacles), the updates launched for 1 / for 2 that had the other outcome, the last guess. */
extern "C" int gie_debug_edt_hint(gie_mapper *m, int force, int32_t *info)
{
    if (!m) { gie_set_err("gie_debug_edt_hint: null handle"); return GIE_ERR_INVALID; }
    if (be_sync(&m->be) != 0) return GIE_ERR_DEVICE;
    be_edt_hint_debug(&m->be, force, info);
    return GIE_OK;
}
#endif
#include "gie_sdf.inc.h"
#include "gie_nf1.inc.h"
#include "gie_costmat.inc.h"
#include "gie_frontier.inc.h"
#include "gie_los.inc.h"
#include "gie_path.inc.h"
#include "gie_cloud.inc.h"
#include "gie_blocks.inc.h"
#include "gie_ground.inc.h"
#include "gie_ground_nf1.inc.h"
#include "gie_ground_los.inc.h"
#include "gie_ground_frontier.inc.h"
#include "gie_ground_costmat.inc.h"
#include "gie_ground_view.inc.h"
#include "gie_ground_rollout.inc.h"
#include "gie_ground_footprint.inc.h"
#include "gie_ground_pose_nf1.inc.h"
#include "gie_ground_sdf.inc.h"
#include "gie_routes.inc.h"

// Host side of libmavflow.so: the C-ABI of include/mavflow.h over the gfx950 kernels.
// Owns the context (stream, pyramid tables, workspace), schedules the per-layer launches in groups of pairs that
// keep the iteration working set cache-sized, and maps every failure to an error code + message.
#include <assert.h>
#include <dlfcn.h>
#include <math.h>
#include <float.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mavflow_internal.h"
#include "../../include/mavflow_truth.h"
#include "../../include/mavflow_validation.h"

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(call)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? MAV_ERR_OOM : MAV_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                         \
    } while (0)
#define CHK(call)              \
    do {                       \
        int rc_ = (call);      \
        if (rc_ != MAV_OK) return rc_; \
    } while (0)

extern "C" const char* mav_last_error(void) { return g_err.c_str(); }

extern "C" void mav_fb_defaults(mav_fb_params* p) { *p = mav_fb_params{0.4, 1, 12, 10, 8, 1.2, 0}; }
extern "C" void mav_foe_defaults(mav_foe_params* p) { *p = mav_foe_params{1000, 2.5, 30.0}; }
extern "C" void mav_thr_defaults(mav_thr_params* p) { *p = mav_thr_params{15.0, 1.0, 0.5, 0.25, 0.5, 8.0}; }

extern "C" int mav_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- small host math ------------------------------------------------------------------------------------
static int cv_round(double v) { return (int)nearbyint(v); }
static int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}
// smallest double T with fl(sqrt(T)) >= t, so that  sqrt(v) < t  <=>  v < T  for every double v (sqrt is monotone
// and correctly rounded on both sides).  Lets the kernels compare squared magnitudes without changing a single result.
static double sq_threshold(double t)
{
    if (!(t > 0)) return 0.0;
    double T = t * t;
    while (sqrt(nextafter(T, -INFINITY)) >= t) T = nextafter(T, -INFINITY);
    while (sqrt(T) < t) T = nextafter(T, INFINITY);
    return T;
}

// float32 twin for frame-0 pairs: numpy compares sqrt_f32(m2) with the threshold rounded to float32 (a Python float next to a
// float32 scalar is "weak"), so  sqrtf(v) < (float)t  <=>  v < T32  with T32 the smallest float whose rounded root is >= (float)t.
static float sq_threshold_f32(double t)
{
    const float tf = (float)t;
    if (!(tf > 0)) return 0.f;
    float T = tf * tf;
    while (sqrtf(nextafterf(T, -INFINITY)) >= tf) T = nextafterf(T, -INFINITY);
    while (sqrtf(T) < tf) T = nextafterf(T, INFINITY);
    return T;
}

static void gaussian_kernel(int n, double sigma, std::vector<float>& k)  // getGaussianKernel(n, sigma, CV_32F)
{
    static const float small_tab[4][7] = {{1.f},
                                          {0.25f, 0.5f, 0.25f},
                                          {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                          {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    const float* fixed = (n % 2 == 1 && n <= 7 && sigma <= 0) ? small_tab[n >> 1] : nullptr;
    const double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double s2 = -0.5 / (sx * sx);
    k.resize(n);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        const double t = fixed ? (double)fixed[i] : exp(s2 * x * x);
        k[i] = (float)t;
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) k[i] = (float)(k[i] * sum);
}

static bool inv6_cholesky(const double G[36], double inv[36])
{
    double L[36];
    memset(L, 0, sizeof(L));
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = G[i * 6 + j];
            for (int k = 0; k < j; k++) s -= L[i * 6 + k] * L[j * 6 + k];
            if (i == j) {
                if (!(s > 0)) return false;
                L[i * 6 + j] = sqrt(s);
            } else
                L[i * 6 + j] = s / L[j * 6 + j];
        }
    for (int c = 0; c < 6; c++) {
        double y[6], x[6];
        for (int i = 0; i < 6; i++) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) s -= L[i * 6 + k] * y[k];
            y[i] = s / L[i * 6 + i];
        }
        for (int i = 5; i >= 0; i--) {
            double s = y[i];
            for (int k = i + 1; k < 6; k++) s -= L[k * 6 + i] * x[k];
            x[i] = s / L[i * 6 + i];
        }
        for (int i = 0; i < 6; i++) inv[i * 6 + c] = x[i];
    }
    return true;
}

static bool prepare_poly(int n, double sigma, PolyCoef* pc)  // FarnebackPrepareGaussian
{
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    std::vector<float> gb(2 * n + 1), xgb(2 * n + 1), xxgb(2 * n + 1);
    float *g = gb.data() + n, *xg = xgb.data() + n, *xxg = xxgb.data() + n;
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        xg[x] = (float)(x * g[x]);
        xxg[x] = (float)(x * x * g[x]);
    }
    double G[36];
    memset(G, 0, sizeof(G));
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0] += g[y] * g[x];
            G[7] += g[y] * g[x] * x * x;
            G[21] += g[y] * g[x] * x * x * x * x;
            G[35] += g[y] * g[x] * x * x * y * y;
        }
    G[14] = G[3] = G[4] = G[18] = G[24] = G[7];
    G[28] = G[21];
    G[22] = G[27] = G[35];
    double inv[36];
    if (!inv6_cholesky(G, inv)) return false;
    pc->n = n;
    for (int k = 0; k <= n; k++) { pc->g[k] = g[k]; pc->xg[k] = xg[k]; pc->xxg[k] = xxg[k]; }
    pc->ig11 = (float)inv[7]; pc->ig03 = (float)inv[3]; pc->ig33 = (float)inv[21]; pc->ig55 = (float)inv[35];
    return true;
}

// resize(INTER_LINEAR): source index and weight for destination index o of d along an axis of S source pixels -- the host twin of the
// kernels' resize_coord (same expression, same roundings: this file is compiled without FMA contraction): (o + 0.5) * scale - 0.5 in
// double, rounded to float, floor, clamp.
static void resize_coord_host(int o, int S, int d, double scale, int* s0, float* f)
{
    if (d == S) { *s0 = o; *f = 0.f; return; }
    const double p = (o + 0.5) * scale;
    float t = (float)(p - 0.5);
    int s = (int)floorf(t);
    t -= (float)s;
    if (s < 0) { t = 0.f; s = 0; }
    if (s >= S - 1) { t = 0.f; s = S - 1; }
    *s0 = s; *f = t;
}

// ---- device memory: the ledger of what a context owns ----------------------------------------------------------------------------
// Every device allocation of a context is recorded (pointer, size, tag) where it is taken, so that mav_destroy frees and mav_mem_info
// counts whatever exists.  A vector searched linearly: a context holds a few dozen allocations, and only alloc / release / total look
// at it -- a call whose buffers exist already never comes here.  No lock: a context is single-threaded (include/mavflow.h).
enum MemTag { MEM_WORKSPACE, MEM_OTHER };       // the Farneback workspace (group slots, deep set, initial-flow snapshot) | everything else
struct DevMem {
    struct Out { void** pp; template <typename T> Out(T** p) : pp((void**)p) {} };     // the address of a device pointer of any type
    struct Want { Out out; size_t bytes; };
    struct Rec { void* p; size_t bytes; MemTag tag; };
    std::vector<Rec> recs;

    int alloc(Out out, size_t bytes, MemTag tag, const char* what)
    {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);     // (never NULL: a record is a live allocation)
        if (e != hipSuccess) {
            (void)hipGetLastError();           // reported here: it must not surface again at the next launch check
            return fail(e == hipErrorOutOfMemory ? MAV_ERR_OOM : MAV_ERR_HIP, "%s (%zu bytes): %s", what, bytes, hipGetErrorString(e));
        }
        recs.push_back({p, bytes, tag});
        *out.pp = p;
        return MAV_OK;
    }
    // all or nothing: either every destination is set, or none is touched and nothing stays allocated (the set's records are the
    // ledger's last ones until the destinations are written: nothing else allocates meanwhile, a context being single-threaded)
    int alloc_set(std::initializer_list<Want> set, MemTag tag, const char* what)
    {
        const size_t mark = recs.size();
        void* p = nullptr;
        for (const Want& w : set)
            if (const int rc = alloc(&p, w.bytes, tag, what); rc != MAV_OK) {
                while (recs.size() > mark) release(recs.back().p);
                return rc;
            }
        size_t i = mark;
        for (const Want& w : set) *w.out.pp = recs[i++].p;
        return MAV_OK;
    }
    void release(void* p)          // NULL, or a pointer this ledger gave out: anything else is a bookkeeping mistake of the caller
    {
        for (size_t i = recs.size(); p && i-- > 0;)
            if (recs[i].p == p) { recs.erase(recs.begin() + i); hipFree(p); return; }
        assert(!p && "DevMem::release: a pointer the ledger has no record of");
    }
    void release_all() { while (!recs.empty()) release(recs.back().p); }
    size_t total(MemTag tag) const
    {
        size_t n = 0;
        for (const Rec& r : recs) if (r.tag == tag) n += r.bytes;
        return n;
    }
};

// ---- context -------------------------------------------------------------------------------------------
struct Layer {
    int w, h, ksize;
    double sigma;
    float* g = nullptr;      // device copy of the Gaussian taps (getGaussianKernel(ksize, sigma, CV_32F))
    int* coord = nullptr;    // device: xs[w] | xf[w] | ys[h] | yf[h] -- the resize coordinates of the layer's columns and rows (coarse layers)
};

// ---- gather uploads: many host arrays -> one contiguous device buffer ----------------------------------------------------------
// The reference's loop is handed one numpy array per frame (Dataset.get_frame / get_flow_uv, src/datasets/dataset.py:205-230); a batch
// of 64 pairs is 128 separate pageable 2 MB arrays.  hipMemcpy from pageable memory stages through the runtime's own bounce buffer on
// the calling thread (~6 GB/s here); np.stack + one copy touches every byte twice.  The stager copies the sources into a ring of
// page-locked chunks on a few worker threads (memcpy at DRAM rate) and issues one H2D per chunk on the copy stream while the next
// chunk is being filled, so the PCIe transfer hides behind the staging.  A source that is already page-locked (mav_host_alloc, the
// Python layer's pinned pool) is copied straight from where it is.
struct Stager {
    enum { NCHUNK = 4 };
    static constexpr size_t CHUNK = (size_t)16 << 20, PIECE = (size_t)512 << 10;
    struct Seg { char* dst; const char* src; size_t n; };
    void* chunk[NCHUNK] = {nullptr};
    hipEvent_t sent[NCHUNK] = {nullptr};
    bool in_flight[NCHUNK] = {false};
    unsigned next_chunk = 0;
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    std::vector<Seg> segs;
    std::atomic<size_t> next_seg{0};
    unsigned long long generation = 0;
    int busy = 0;
    bool stop = false;

    void run_segments()
    {
        for (;;) {
            const size_t i = next_seg.fetch_add(1);
            if (i >= segs.size()) return;
            memcpy(segs[i].dst, segs[i].src, segs[i].n);
        }
    }
    void worker()
    {
        unsigned long long seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_job.wait(lk, [&] { return stop || generation != seen; });
            if (stop) return;
            seen = generation;
            lk.unlock();
            run_segments();
            lk.lock();
            if (--busy == 0) cv_done.notify_one();
        }
    }
    // copy every segment of `segs` (the calling thread takes part), return when all are done
    void copy_all()
    {
        next_seg.store(0);
        if (workers.empty() || segs.size() < 2) { run_segments(); return; }
        {
            std::lock_guard<std::mutex> lk(m);
            busy = (int)workers.size();
            generation++;
        }
        cv_job.notify_all();
        run_segments();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return busy == 0; });
    }
    void shutdown()
    {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv_job.notify_all();
        for (auto& t : workers) t.join();
        workers.clear();
        for (int i = 0; i < NCHUNK; i++) {
            if (sent[i]) { hipEventSynchronize(sent[i]); hipEventDestroy(sent[i]); }
            if (chunk[i]) hipHostFree(chunk[i]);
        }
    }
};
enum KernelId { K_BLUR_RESIZE, K_POLYEXP, K_UPDATE, K_ITER, K_ITER_COARSE, K_FOE, K_PHI, K_MISC, K_LK_CORNERS, K_LK_PYRAMID, K_LK_TRACK, K_LK_PICK, K_COMPONENTS, K_HISTORY_PUT, K_HISTORY_TRACE, K_GTS_MAX, K_GTS_COUNT, K_GTS_LIST, K_GTS_SUM, K_JPEG_INTERVALS, K_JPEG_ENTROPY, K_JPEG_IDCT, K_JPEG_FINISH, K_COUNT };
static const char* const kKernelNames[K_COUNT] = {"blur_resize", "polyexp", "update_matrices", "blur_iter", "blur_iter_coarse",
                                                  "foe_ransac", "phi_mask_box", "misc", "lk_corners", "lk_pyramid", "lk_track", "lk_pick", "components", "history_put", "history_trace",
                                                  "gt_stats_max", "gt_stats_count", "gt_stats_list", "gt_stats_sum", "jpeg_intervals", "jpeg_entropy", "jpeg_idct", "jpeg_finish"};
struct ProfRec { int kid; hipEvent_t a, b; int stream; };
struct ProfInterval { int kid; float t0, t1; int stream; };      // ms since the profile was switched on

// Sparse optical flow (mav_good_features / mav_lk_track): everything it owns, allocated by the first such call (ensure_lk).
enum { LK_CNT_PICKED = 2 + MAV_LK_HIST, LK_CNT_STATS, LK_CNT_N = LK_CNT_STATS + 2 };   // corner count of the host forms; chunks, rounds
struct LkState {
    LkLevels dims{};                 // every level the frame size allows (MAV_LK_MAX_LEVEL + 1 at most), whatever the window
    size_t pyr_elems = 0;            // elements of one pyramid block
    uint8_t* pyr[2] = {nullptr, nullptr};   // two frame slots: the resident frame and the one before / after it
    int built[2] = {0, 0};           // levels of the slot's pyramid that are valid (0: the slot holds no frame)
    int cur = -1;                    // slot of the resident frame, -1: none
    short2* deriv = nullptr;         // Scharr pairs of ONE slot's levels
    int deriv_slot = -1, deriv_levels = 0;
    float* eig = nullptr;            // (H, W) min-eigenvalue map; dead once the candidates are out: the pick's grid of accepted corners
    size_t eig_words = 0;            // W * H, or the largest grid where a one-pixel-wide frame makes that larger
    uint2* cand = nullptr;           // MAV_GFTT_MAX_CANDIDATES x (value bits, linear index)
    unsigned* counters = nullptr;    // [0] max key, [1] candidate count, [2 ..] iteration histogram (MAV_LK_HIST), then LK_CNT_*
    float *pts = nullptr, *out = nullptr;   // MAV_LK_MAX_POINTS x 2 each
    uint8_t* status = nullptr;       // MAV_LK_MAX_POINTS
    bool hist_valid = false;
    std::vector<float> fetch;        // host staging of the host forms' corners: kept, so a call allocates nothing
};

// A flow history (include/mavflow.h: mav_history_*): the ring and where the next field goes.
struct mav_history {
    int length = 0, depth = 0, flags = 0, index = 0;
    long pushes = 0;
    void* ring = nullptr;            // length slots of W * H pairs of `depth`, from the owning context's ledger
    size_t ring_bytes = 0;
};

struct mav_ctx {
    int device = 0, W = 0, H = 0, max_batch = 0, group = 0, group_fine = 1;
    mav_fb_params fb;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // uploads that overlap the compute stream (mav_upload_async / mav_upload_fence)
    hipEvent_t copy_done = nullptr, compute_mark = nullptr;
    hipEvent_t gather_done = nullptr;    // mav_upload_gather: "the page-locked sources sent from where they are have been read"
    struct Stager* stager = nullptr;     // mav_upload_gather: page-locked ring + worker threads (created by its first call)
    struct Worker* worker = nullptr;     // mav_frame_step_post: the thread that enqueues posted steps (created by the first post)
    int upload_threads = 4;              // option "upload_threads"
    bool inline_uploads = false;         // option "inline_uploads": uploads go on the compute stream (no copy stream, no cross-stream events)
    int stream_priority = 0;             // option "stream_priority": the compute stream's priority class (the runtime keeps a queue pool per class)
    const float* last_flow = nullptr;    // where the latest farneback / process_batch call wrote its flow (mav_last_flow_dev)
    const uint8_t *last_mf = nullptr, *last_md = nullptr;   // masks of the latest host-pointer detection call, still in their
    int last_mask_batch = 0;                                // staging blocks (mav_last_masks_tpr_fpr)
    std::vector<Layer> layers;
    PolyCoef pc;
    // workspace (group slots)
    size_t n0 = 0, n1 = 0;
    // Workspace of `group` slots.
    struct WorkSet {
        float *Htmp = nullptr;       // scratch of the two-pass blur+resize (layers whose Gaussian is too long for the fused kernel)
        // R = R0 | R1 in ONE allocation (R1 = R0 + 5 n0 group): the expansions of the two frames of every pair.  For a frame SEQUENCE
        // (next = prev + one frame) the group's g + 1 frames are expanded once into slots 0 .. g and pair s reads slots s and s + 1.
        float *I = nullptr, *R = nullptr, *Ma = nullptr, *Mb = nullptr, *fc[2] = {nullptr, nullptr};
        // small groups (flow_group): the coarse layers' images / expansions, every layer in a region of its own (layer k: c_off[k]
        // floats per frame in, c_stride[k] floats per frame), so that the whole pyramid can be blurred and expanded in two launches
        float *Ic = nullptr, *Rc = nullptr;
    } ws;
    std::vector<size_t> c_off, c_stride;      // per layer (index 0 unused); c_total = sum of the strides
    size_t c_total = 0;
    // DEEP LAYERS (deep_layers): layers kd .. top, each at most 1/deep_frac of the frame -- every coarse layer of a 0.4-scale pyramid.
    // When a call has more than one group they run ONCE for up to deep_cap pairs of the call (their images from one launch per tile code,
    // all expansions from one launch, sweeps over all pairs in cache-sized sub-groups) before the groups start; the groups then begin at
    // layer kd - 1 with the deep flow as their coarser layer.  Buffers of their own, every layer in a compact region.
    struct DeepSet { float *I = nullptr, *R = nullptr, *Ma = nullptr, *Mb = nullptr, *f[2] = {nullptr, nullptr}; } deep;
    int kd = 0, deep_cap = 0;                 // kd = 0: no deep layer
    // option "deep_frac" (before the first flow call): a layer is deep when its pixels x deep_frac <= the frame's.  6: every coarse layer
    // of a 0.4-scale pyramid (layer 1 is 0.16 of the frame).  Measured with 32 (layers 2 - 4 of the 4K preset only) vs 6: 1080p, 64 pairs
    // 2 579 - 2 637 vs 2 653 - 2 686 pairs/s (+2.4 %: layer 1's sixteen sub-groups of 4 pairs run back to back for the whole call instead
    // of four per group behind a fork / join each); 4K 607 - 609 vs 609 - 610 (profiles/r04/ab_deep_frac.log)
    int deep_frac = 6;
    bool deep_batch = true;                   // option "deep_batch"
    int band_skew = -1;                       // option "band_skew": tile rows the band boundaries move down to compensate the sweeps' skew
                                              // (sweeps_band_major); -1 = (iterations - 1) / 2, 0 = equal bands
    int band_phase = 0;                       // option "band_phase": n > 0 = the second stream's pairs use a partition shifted by half a band
                                              // when a pair has at least n bands (sweeps_band_major); 0 = never (default: measured slower)
    bool coarse_bands = false;                // option "coarse_bands": a coarse layer whose per-pair working set exceeds band_mb is swept like the finest one
                                              // (measured at 3840x2160 / 5 layers: 584 vs 594 pairs/s -- half-size launches cost more than the cache returns; off)
    int small_g = 0;                          // pairs the Ic / Rc buffers were sized for (0: none)
    bool small_batch = true;                  // option "small_batch"
    int sweep_wt = -1;                        // option "sweep_write_through": -1 = in the two-stream schedules only (default), 0 / 1 = never / always
    int small_batch_mb = 200;                 // option "small_batch_mb": ... for groups of at most this much finest-layer sweep working set
    int window = MAV_WINDOW_BOX;     // mav_set_window: the sweeps' window (not an option: a box context's schedule line never names it)
    GaussTaps gauss;                 // the Gaussian window's taps for fb.winsize (mav_create)
    int bands = 1;                   // option "bands": the finest layer's sweeps in band-major order over this many skewed bands
    // option "pairs_in_flight" (1 or 2): the finest layer's per-pair work (initial M + sweeps) of a group alternates between the
    // compute stream and pair_stream, every pair band-major over bands of at most pif_band_mb of working set (layer_sweeps)
    // band_mb 96: 2 bands at 1080p (83 MB each), 7 at 3840x2160 (95 MB, ~1 160 tiles per launch on 1 280 resident slots): 608 vs 605
    // pairs/s with 8 bands of 83 MB, 597 with 6 of 111 MB, 567 with 5 (profiles/r04/ab_band_mb_4k.log)
    int pairs_in_flight = 2, pif_band_mb = 96;
    bool bands_set = false;          // "bands" given explicitly: that many bands in either schedule
    int bands_auto = 1;              // what "bands" = 0 restores
    bool group_fine_set = false;     // "group_fine" given explicitly
    hipStream_t pair_stream = nullptr;
    hipEvent_t pif_fork = nullptr, pif_join = nullptr;
    bool share_frames = true;        // option "share_frames": expand a frame once when next == prev + one frame (a frame sequence)
    int coarse_cache_mb = 220;       // coarse layers: pairs per launch capped so that the sweeps' working set stays below this (0 = no cap)
    // tuning options that used to be environment variables (mav_set_option / mav_get_option; all reported by mav_schedule_info)
    bool share_m = true;             // "share_m": one-stream schedule, every pair of a group ping-pongs M through the first slot's buffers
    int coarse_half = 0;             // "coarse_half": pairs per launch of the coarse layers' two-stream schedule (0 = half the cache-sized count)
    int strip = 0;                   // "strip": width in tiles of the column strips of the XCD-aware tile order (0 = automatic)
    bool phi_screen = true;          // "phi_screen": the float32 screen in front of the exact phi / threshold arithmetic
    int phi_yloop = 0;               // "phi_yloop": 16-row blocks per workgroup of the phi kernel (0 = automatic)
    size_t htmp_stride = 0;
    DevMem mem;                    // every device allocation below (and the layers' tables): owner, byte counts, release at mav_destroy
    bool ws_ready = false;         // the Farneback workspace exists (ensure_workspace: allocated by the first call that computes flow)
    float* flow_ws = nullptr;      // lazily allocated (max_batch) when the caller does not want the flow (ensure_flow_ws)
    // OPTFLOW_USE_INITIAL_FLOW (mav_farneback_init / _init_dev): the top layer's initial flow, resize(flow0, INTER_AREA) * scale, of the
    // pairs that enter the top layer together (a group, or the deep layers' pairs), built before the first launch that reads it -- so a
    // call may write its flow over flow0 (the cv2 idiom).  Allocated by the first such call, grown on demand; part of the workspace.
    float* init_snap = nullptr;
    int init_cap = 0;              // pairs it holds
    size_t init_stride = 0;
    // detection scratch (max_batch)
    FoeScratch foe_sc{nullptr, nullptr, nullptr};
    int foe_sc_n = 0;
    double* foe_dev = nullptr;
    int32_t* box_acc = nullptr;
    unsigned long long* u64_scratch = nullptr;  // [max_batch*8]
    int* i32_scratch = nullptr;                 // [max_batch]
    DerotParams* derot_dev = nullptr;
    // result images (mav_render*): per-pair max |flow| and the render calls' own derotation constants (lazily, max_batch), and what the
    // latest mav_detect_dev left resident for mav_last_render (batch 0: nothing)
    unsigned long long* render_max = nullptr;
    DerotParams* render_derot = nullptr;
    struct LastRender {
        const float* flow = nullptr; const DerotParams* derot = nullptr; const double* foe = nullptr; const uint8_t* sky = nullptr;
        const uint8_t* mask_fixed = nullptr;         // the call's fixed mask, if it kept one (mav_last_overlay)
        mav_thr_params thr{};
        int batch = 0;
    } last_render;
    // what mav_last_roc_sweep reads: last_render's fields after a detection call, or the field (float32 or float64), FoE and sky a
    // mav_phi_mask(_f32) call left in its staging blocks (batch 0: nothing)
    struct LastRoc {
        const void* flow = nullptr; bool f64 = false; const DerotParams* derot = nullptr; const double* foe = nullptr; const uint8_t* sky = nullptr;
        int batch = 0;
    } last_roc;
    // staging buffers of the host-pointer entry points: slot i of a call re-uses the block slot i of the previous call
    // left behind (grow-only), so the staged path performs no hipMalloc / hipFree once warm
    struct Block { void* p = nullptr; size_t cap = 0; };
    std::vector<Block> scratch;
    size_t scratch_next = 0;
    LkState lk;                                 // sparse optical flow workspace (first mav_good_features / mav_lk_track call)
    uint8_t* png_ws = nullptr;                  // PNG encoder: segment slots and records of one chunk of images (first encode call, grow-only)
    size_t png_ws_cap = 0;                      // bytes it holds
    uint8_t* pyr_ws = nullptr;                  // analyze_pyramid level images (lazily, max_batch)
    size_t pyr_ws_cap = 0;
    unsigned long long* sat = nullptr;          // optimize_window summed-area tables (lazily, max_batch)
    uint8_t* cc_ws = nullptr;                   // connected components: label planes + chunk counters of one sub-batch (first call, grow-only
    size_t cc_ws_cap = 0;                       // up to "cc_workspace_mb", or one image's)
    int cc_workspace_mb = 256;                  // option "cc_workspace_mb"
    // threshold sweep armed for the frame steps (mav_roc_arm): the checked lists and where a step's tables go inside its out block
    bool roc_armed = false;
    RocThr roc_thr{};
    size_t roc_off = 0;
    // global-motion subtraction (mav_global_motion*, mav_find_homography*): per-item scratch (lazily, max_batch), the pair buffers
    // (grow-only, pairs_cap = pairs per item they hold) and what the latest call left resident for mav_last_global_motion_render
    struct Motion {
        double* H = nullptr; int* ok = nullptr; int64_t* pyr = nullptr; int32_t* win = nullptr; int32_t* opt_win = nullptr;
        int64_t* opt_score = nullptr; unsigned long long* key = nullptr;      // key: [2 * max_batch] the residual maximum | the window scan
        uint8_t* gray = nullptr;                                              // the normalised image of a call whose caller does not want it
        double *src = nullptr, *dst = nullptr, *work = nullptr;
        int32_t* coords = nullptr;
        size_t pairs_cap = 0;
        struct Last { const float* flow = nullptr; const double* M = nullptr; int m_stride = 0; int batch = 0; } last;
    } gm;
    std::vector<mav_history*> histories;       // flow histories (mav_history_create): the objects are the context's, their rings are in `mem`
    double* radial_edges = nullptr;            // mav_radial_error_hist: the two edge lists of the call in hand (first call; 2 * MAV_RADIAL_MAX_EDGES doubles)
    RadialEdges radial_mag{}, radial_err{};    // ... and what the stream's last call put there (n = 0: nothing): a sequence sends its lists once
    void* gts_scratch = nullptr;               // mav_gt_stats: accumulators, row counts and (without a caller's index list) the list of the call in hand
    size_t gts_cap = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    int profiling = 0;               // 0 off; 1 = HIP events around every launch; 2 = around every RUN of launches of one class on a stream
    struct OpenRun { hipStream_t st; int kid; hipEvent_t a; };
    std::vector<OpenRun> open_runs;  // mode 2: the run in progress on each stream
    std::vector<ProfRec> prof;
    std::vector<ProfInterval> prof_iv;          // every profiled launch as an interval (mav_profile_busy: union over concurrent streams)
    hipEvent_t prof_base = nullptr;
    double prof_ms[K_COUNT] = {0};
    long prof_n[K_COUNT] = {0};
};

// mode 2: the end event of a run is recorded when the next launch on that stream belongs to another class (or at collection): it
// completes, in stream order, when the run's last kernel has -- two events per run instead of two per launch, so that the
// overlap of the two streams is measured almost undisturbed (mav_profile_busy)
static void close_run(mav_ctx* c, size_t i)
{
    mav_ctx::OpenRun r = c->open_runs[i];
    hipEvent_t b = nullptr;
    hipEventCreate(&b);
    hipEventRecord(b, r.st);
    c->prof.push_back({r.kid, r.a, b, r.st == c->stream ? 0 : 1});
    c->open_runs.erase(c->open_runs.begin() + i);
}
static void prof_close_stream(mav_ctx* c, hipStream_t st)       // before a stream waits for another one: the wait is not part of the run
{
    for (size_t i = 0; i < c->open_runs.size(); i++) if (c->open_runs[i].st == st) { close_run(c, i); return; }
}
struct ProfScope {
    mav_ctx* c; int kid; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(mav_ctx* c_, int k, hipStream_t st_ = nullptr) : c(c_), kid(k), st(st_ ? st_ : c_->stream)
    {
        if (c->profiling == 1) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, st); }
        else if (c->profiling == 2) {
            for (size_t i = 0; i < c->open_runs.size(); i++)
                if (c->open_runs[i].st == st) {
                    if (c->open_runs[i].kid == kid) return;          // the run goes on
                    close_run(c, i);
                    break;
                }
            hipEventCreate(&a);
            hipEventRecord(a, st);
            c->open_runs.push_back({st, kid, a});
        }
    }
    ~ProfScope()
    {
        if (c->profiling == 1) { hipEventRecord(b, st); c->prof.push_back({kid, a, b, st == c->stream ? 0 : 1}); }
    }
};

// Pairs of the largest group the small-group schedule can take (is_small_group) when the context runs groups of `group` pairs.
static int small_group_cap(const mav_ctx* c, int group)
{
    size_t sg = c->c_total ? ((size_t)c->small_batch_mb << 20) / (c->n0 * 80) : 0;
    return (int)(sg > (size_t)group ? (size_t)group : sg);
}
// Workspace for `group` slots.  The new buffers are allocated in full before the old ones are released: when an allocation fails the
// context keeps its previous group and stays usable (the caller sees MAV_ERR_OOM).
static int alloc_group(mav_ctx* c, int group)
{
    const size_t g = (size_t)group, nc = 2 * (c->n1 ? c->n1 : 1);
    // I / I2 hold the 2 g frames of a group (prev and next in one launch; a frame sequence of g pairs has g + 1 <= 2 g frames);
    // Htmp holds g + 1 (the two-pass blur never runs over more frames per launch)
    // Ic / Rc: for the largest group the small-group schedule can take (is_small_group), 2 g frames of every coarse layer
    const size_t sg = (size_t)small_group_cap(c, group), F = sizeof(float);
    mav_ctx::WorkSet n;            // the new set, in full before the old one goes
    mav_ctx::WorkSet& w = c->ws;
    CHK(c->mem.alloc_set({{&n.I, F * c->n0 * 2 * g}, {&n.R, F * 10 * c->n0 * g}, {&n.Ma, F * 5 * c->n0 * g}, {&n.Mb, F * 5 * c->n0 * g},
                          {&n.fc[0], F * nc * g}, {&n.fc[1], F * nc * g}, {&n.Htmp, F * c->htmp_stride * (g + 1)},
                          {&n.Ic, F * (sg ? 2 * sg * c->c_total : 1)}, {&n.Rc, F * (sg ? 10 * sg * c->c_total : 1)}},
                         MEM_WORKSPACE, ("Farneback workspace: a buffer of the slots of group " + std::to_string(group)).c_str()));
    for (float* old : {w.I, w.R, w.Ma, w.Mb, w.fc[0], w.fc[1], w.Htmp, w.Ic, w.Rc}) c->mem.release(old);
    w = n;
    c->group = group;
    c->small_g = (int)sg;
    c->ws_ready = true;
    return MAV_OK;
}
// The deep layers' work set (deep_layers) does not depend on the group and is reachable only by calls of more than one group
// (use_deep_batch): allocated by the first such call -- a context whose calls never exceed one group (max_batch <= group, or one-pair
// calls) never holds it (150 MB per pair at 3840x2160 / 5 levels) --, kept across "group" changes until mav_destroy.
static int ensure_deep(mav_ctx* c)
{
    if (c->kd <= 0 || c->deep.I) return MAV_OK;
    const size_t D = (size_t)c->deep_cap, dt = c->c_total - c->c_off[c->kd], top = c->c_stride[c->kd], F = sizeof(float);
    mav_ctx::DeepSet& d = c->deep;
    return c->mem.alloc_set({{&d.I, F * 2 * D * dt}, {&d.R, F * 10 * D * dt}, {&d.Ma, F * 5 * D * top}, {&d.Mb, F * 5 * D * top},
                             {&d.f[0], F * 2 * D * top}, {&d.f[1], F * 2 * D * top}}, MEM_WORKSPACE, "Farneback workspace: a buffer of the deep layers");
}
// The Farneback workspace (174 MB per 1080p slot, 16 slots by default) belongs to the calls that compute flow: a context created for
// mav_bbox / mav_tpr_fpr_counts / mav_phi_mask / mav_detect never pays for it (the reference's helpers are stateless free functions,
// src/im_helpers.py:55-84,244-252).  Allocated by the first call that needs it, kept until mav_destroy.
static int ensure_workspace(mav_ctx* c)
{
    return c->ws_ready ? MAV_OK : alloc_group(c, c->group);
}

static int ensure_copy_stream(mav_ctx* c)
{
    if (c->copy_stream) return MAV_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&c->copy_done, &c->compute_mark}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return MAV_OK;
}
static int ensure_pair_stream(mav_ctx* c)
{
    if (c->pair_stream) return MAV_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamCreateWithFlags(&c->pair_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&c->pif_fork, &c->pif_join}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return MAV_OK;
}

static int sync_all_streams(mav_ctx* c)
{
    for (hipStream_t st : {c->stream, c->pair_stream})
        if (st) HIPCHK(hipStreamSynchronize(st));
    return MAV_OK;
}

// A grow-only buffer: *p holds *cap bytes and is replaced by one of `need` bytes when that is more (contents are not kept).  `cap` is NULL
// when the caller keeps the capacity in a unit of its own and has decided already.  The caller says on which streams enqueued work may
// still read the old buffer -- they are drained before it goes -- and whether it goes before the new one is taken (RELEASE_FIRST: the peak
// is the larger of the two; after a failed allocation the context holds neither, *p NULL and *cap 0) or after (ALLOC_FIRST: a failed
// allocation leaves *p and *cap as they were, the context stays usable).
enum ReadOn { READ_ON_COMPUTE, READ_ON_ALL };           // the compute stream | the compute stream and the pair stream
enum GrowOrder { RELEASE_FIRST, ALLOC_FIRST };
static int grow_buffer(mav_ctx* c, DevMem::Out p, size_t* cap, size_t need, MemTag tag, ReadOn streams, GrowOrder order, const char* what)
{
    if (cap && need <= *cap) return MAV_OK;
    void* old = *p.pp;
    if (old && streams == READ_ON_ALL) CHK(sync_all_streams(c));
    else if (old) HIPCHK(hipStreamSynchronize(c->stream));
    if (order == RELEASE_FIRST) {
        c->mem.release(old);
        old = *p.pp = nullptr;
        if (cap) *cap = 0;
    }
    CHK(c->mem.alloc(p, need, tag, what));
    c->mem.release(old);
    if (cap) *cap = need;
    return MAV_OK;
}
static int ensure_flow_ws(mav_ctx* c)          // the flow of a call whose caller does not want to see it
{
    return c->flow_ws ? MAV_OK : c->mem.alloc(&c->flow_ws, sizeof(float) * 2 * c->n0 * c->max_batch, MEM_OTHER, "flow buffer");
}

static void stop_worker(mav_ctx* c);
extern "C" int mav_destroy(mav_ctx* c)
{
    if (!c) return MAV_OK;
    hipSetDevice(c->device);
    stop_worker(c);                  // (finishes the step it is enqueueing, drops the rest, leaves)
    (void)sync_all_streams(c);
    if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
    if (c->stager) { c->stager->shutdown(); delete c->stager; c->stager = nullptr; }
    c->mem.release_all();
    for (mav_history* h : c->histories) delete h;
    for (auto& r : c->prof) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    if (c->prof_base) hipEventDestroy(c->prof_base);
    for (hipEvent_t e : {c->t0, c->t1, c->copy_done, c->compute_mark, c->gather_done, c->pif_fork, c->pif_join}) if (e) hipEventDestroy(e);
    for (hipStream_t st : {c->pair_stream, c->copy_stream, c->stream}) if (st) hipStreamDestroy(st);
    delete c;
    return MAV_OK;
}

extern "C" int mav_create(mav_ctx** out, int device, int W, int H, int max_batch, const mav_fb_params* fbp)
{
    if (!out) return fail(MAV_ERR_ARG, "mav_create: out is NULL");
    *out = nullptr;
    mav_fb_params fb;
    if (fbp) fb = *fbp; else mav_fb_defaults(&fb);
    if (W < 1 || H < 1 || max_batch < 1) return fail(MAV_ERR_ARG, "mav_create: bad size W=%d H=%d max_batch=%d", W, H, max_batch);
    if (max_batch > 65535 || (size_t)max_batch * (size_t)W * (size_t)H > MAV_MAX_BATCH_PIXELS)
        return fail(MAV_ERR_ARG, "mav_create: max_batch %d x %dx%d exceeds the bound (max_batch <= 65535, max_batch * W * H <= %zu pixels)", max_batch,
                    W, H, (size_t)MAV_MAX_BATCH_PIXELS);
    if (!(fb.pyr_scale > 0 && fb.pyr_scale < 1)) return fail(MAV_ERR_ARG, "pyr_scale must be in (0, 1), got %g", fb.pyr_scale);
    if (fb.levels < 0 || fb.winsize < 2 || fb.winsize > 64 || fb.iterations < 1 || fb.poly_n < 1 || fb.poly_n > MAV_MAX_POLY_N)
        return fail(MAV_ERR_ARG, "unsupported Farneback parameters (levels=%d winsize=%d iterations=%d poly_n=%d)", fb.levels,
                    fb.winsize, fb.iterations, fb.poly_n);
    // OPTFLOW_USE_INITIAL_FLOW is accepted so that a cv2 argument list passes as it is; only the entry points that take an initial flow
    // (mav_farneback_init / _init_dev) use one, the others start from zero whatever the bit says
    if (fb.flags & ~MAV_OPTFLOW_USE_INITIAL_FLOW)
        return fail(MAV_ERR_ARG, "mav_create takes flags 0 and OPTFLOW_USE_INITIAL_FLOW (4) only, got %d (OPTFLOW_FARNEBACK_GAUSSIAN = 256 is "
                    "chosen with mav_set_window(ctx, MAV_WINDOW_GAUSSIAN): mask the bit)", fb.flags);
    if (fb.winsize / 2 != 6 && blur_iter_lds_bytes(fb.winsize) > (size_t)160 * 1024)
        return fail(MAV_ERR_ARG, "winsize %d needs %zu bytes of LDS per workgroup in the general sweep kernel, the CU has 163840", fb.winsize,
                    blur_iter_lds_bytes(fb.winsize));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(MAV_ERR_STATE, "no HIP device visible: libmavflow has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(MAV_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    if (fb.winsize / 2 != 6) {      // the general sweep kernel asks for more dynamic LDS than the default limit: per device, checked
        const char* err = blur_iter_prepare(fb.winsize);
        if (err) return fail(MAV_ERR_HIP, "winsize %d: %s", fb.winsize, err);
    }

    mav_ctx* c = new mav_ctx();
    c->device = device; c->W = W; c->H = H; c->max_batch = max_batch; c->fb = fb;
    gauss_taps(fb.winsize, &c->gauss);
    struct Guard { mav_ctx* c; ~Guard() { mav_destroy(c); } } half_built{c};      // any failure below destroys what exists by then
    // The compute stream now; the copy stream (overlapped uploads) and the pair stream (two pairs in flight) with their events when a
    // call first needs them (ensure_copy_stream / ensure_pair_stream): a context that serves one-pair calls as one of several LANES
    // (mavflow/pipeline.py) then owns exactly one stream, i.e. one hardware queue of the runtime's small pool -- streams beyond the
    // pool's size share queues, and two lanes whose streams share one do not overlap at all.
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->t0));
    HIPCHK(hipEventCreate(&c->t1));
    if (!prepare_poly(fb.poly_n, fb.poly_sigma, &c->pc)) return fail(MAV_ERR_ARG, "poly_sigma %g gives a singular moment matrix", fb.poly_sigma);

    // layer selection exactly as optflowgf.cpp (A.1): levels is the number of EXTRA layers actually reachable
    int levels = 0;
    {
        double scale = 1;
        for (levels = 0; levels < fb.levels; levels++) {
            scale *= fb.pyr_scale;
            if (W * scale < 32 || H * scale < 32) break;
        }
    }
    c->layers.resize(levels + 1);
    for (int k = 0; k <= levels; k++) {
        Layer& l = c->layers[k];
        double scale = 1;
        for (int i = 0; i < k; i++) scale *= fb.pyr_scale;
        l.sigma = (1. / scale - 1) * 0.5;
        l.ksize = cv_round(l.sigma * 5) | 1;
        if (l.ksize < 3) l.ksize = 3;
        l.w = cv_round(W * scale);
        l.h = cv_round(H * scale);
        if (l.w < 1 || l.h < 1) return fail(MAV_ERR_ARG, "layer %d collapses to %dx%d", k, l.w, l.h);
        std::vector<float> g;
        gaussian_kernel(l.ksize, l.sigma, g);
        CHK(c->mem.alloc(&l.g, g.size() * sizeof(float), MEM_OTHER, "layer taps"));
        HIPCHK(hipMemcpy(l.g, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
        if (k > 0) {                                    // the layer's resize coordinates, once (the kernels used to evaluate them per thread, in double)
            std::vector<int> tab(2 * (size_t)(l.w + l.h));
            for (int x = 0; x < l.w; x++) resize_coord_host(x, W, l.w, (double)W / l.w, &tab[x], (float*)&tab[l.w + x]);
            for (int y = 0; y < l.h; y++) resize_coord_host(y, H, l.h, (double)H / l.h, &tab[2 * l.w + y], (float*)&tab[2 * l.w + l.h + y]);
            CHK(c->mem.alloc(&l.coord, tab.size() * sizeof(int), MEM_OTHER, "layer resize coordinates"));
            HIPCHK(hipMemcpy(l.coord, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    c->n0 = (size_t)W * H;
    c->n1 = levels >= 1 ? (size_t)c->layers[1].w * c->layers[1].h : 0;
    c->c_off.assign(levels + 1, 0); c->c_stride.assign(levels + 1, 0);
    for (int k = 1; k <= levels; k++) {                 // slot strides rounded up to 64 floats: every slot stays 256-byte aligned
        c->c_stride[k] = ((size_t)c->layers[k].w * c->layers[k].h + 63) & ~(size_t)63;
        c->c_off[k] = c->c_total;
        c->c_total += c->c_stride[k];
    }
    for (int k = levels; k >= 1; k--)                   // deep layers: the top of the pyramid, every layer at most 1/deep_frac of the frame
        if ((size_t)c->layers[k].w * c->layers[k].h * (size_t)c->deep_frac <= c->n0) c->kd = k; else break;
    c->deep_cap = max_batch < 64 ? max_batch : 64;
    c->htmp_stride = (size_t)H * W;                    // any layer (even layer 0 when its fast form does not apply) fits
    // group: pairs per launch for everything but the finest layer's sweeps (see flow_group).
    // (1080p, 64 pairs: 27.0 - 27.5 ms with groups of 16 or 32, 27.8 - 28.1 with 8, 28.4 with 4 -- the batched blur / expansion
    // launches of 16 pairs run 10 - 15 % faster than two of 8; at 3840x2160 8 and 16 are equal, 4 is slower: profiles/r02/ab_group*.log)
    int group = (size_t)W * H <= ((size_t)4 << 20) ? 16 : 8;
    if (group > max_batch) group = max_batch;
    // One pair's finest-layer working set (80 B/px) fits the 256 MB Infinity Cache up to ~2.6 Mpx.  Beyond that a pair is swept
    // band by band (sweeps_band_major): the one-stream schedule ("pairs_in_flight" = 1) over bands of at most ~230 MB (measured at
    // 3840x2160, 16 pairs: 3 bands 31.6 ms, 4 bands 32.4, 5 bands 34.3, 6 bands 35.0, batched sweep-major 35.4); the default
    // two-stream schedule sizes its own bands ("band_mb").
    if ((size_t)W * H * 80 > (size_t)200 << 20) {
        c->bands = (int)(((size_t)W * H * 80 + ((size_t)230 << 20) - 1) / ((size_t)230 << 20));
        if (c->bands > 8) c->bands = 8;
    }
    c->bands_auto = c->bands;
    c->group = group;                                   // the workspace itself comes with the first call that computes flow (ensure_workspace)
    c->small_g = small_group_cap(c, group);
    const size_t B = (size_t)max_batch;
    // foe_dev: a FoE per pair, which last_render / last_roc point at, and behind them the one of mav_ransac -- a vote on caller-supplied
    // estimates is no detection call and must not write what those records read
    CHK(c->mem.alloc_set({{&c->foe_dev, sizeof(double) * 2 * (B + 1)}, {&c->box_acc, sizeof(int32_t) * 4 * B},
                          {&c->u64_scratch, sizeof(unsigned long long) * 8 * B},       // two count blocks of 4 per pair
                          {&c->i32_scratch, sizeof(int) * B}, {&c->derot_dev, sizeof(DerotParams) * B}, {&c->foe_sc.count, sizeof(int) * B},
                          {&c->foe_sc.best_key, sizeof(unsigned long long) * B}, {&c->foe_sc.done, sizeof(unsigned) * 2 * B}},
                         MEM_OTHER, "detection scratch"));
    HIPCHK(hipMemset(c->foe_sc.done, 0, sizeof(unsigned) * 2 * B));
    half_built.c = nullptr;
    *out = c;
    return MAV_OK;
}

// ---- options: every scheduling / tuning switch of the library lives here (no environment variables) -----------------------------
// The options that do more than store a value:
static int set_group(mav_ctx* c, long value)
{
    const int g = value > c->max_batch ? c->max_batch : (int)value;
    HIPCHK(hipSetDevice(c->device));
    CHK(sync_all_streams(c));
    if (g == c->group) return MAV_OK;
    if (!c->ws_ready) { c->group = g; c->small_g = small_group_cap(c, g); return MAV_OK; }    // nothing allocated yet: the plan changes
    return alloc_group(c, g);
}
static int set_group_fine(mav_ctx* c, long value) { c->group_fine = (int)value; c->group_fine_set = true; return MAV_OK; }
static int set_bands(mav_ctx* c, long value)             // 0 = back to automatic
{
    c->bands_set = value > 0;
    c->bands = value > 0 ? (int)value : c->bands_auto;
    return MAV_OK;
}
static int set_deep_frac(mav_ctx* c, long value)
{
    if (c->ws_ready) return fail(MAV_ERR_STATE, "deep_frac must be set before the first call that computes flow");
    c->deep_frac = (int)value; c->kd = 0;
    for (int k = (int)c->layers.size() - 1; k >= 1; k--)
        if ((size_t)c->layers[k].w * c->layers[k].h * (size_t)value <= c->n0) c->kd = k; else break;
    return MAV_OK;
}
static int set_inline_uploads(mav_ctx* c, long value)
{
    if (value < 0 || value > 1) return fail(MAV_ERR_ARG, "option 'inline_uploads' must be 0 or 1, got %ld", value);
    HIPCHK(hipSetDevice(c->device));
    if (c->copy_stream) HIPCHK(hipStreamSynchronize(c->copy_stream));      // nothing of the old mode is left in flight
    HIPCHK(hipStreamSynchronize(c->stream));
    c->inline_uploads = value != 0;
    return MAV_OK;
}
static int set_stream_priority(mav_ctx* c, long value)
{
    // The HIP runtime maps streams onto a pool of (by default four) hardware queues PER PRIORITY CLASS, least-used first; which
    // queue a new stream gets depends on every stream the process has ever made.  Lanes -- contexts that take a stream of small calls
    // in turn and must not share a queue (pipeline.py) -- ask for a class of their own: -1 = high.  The context's compute stream is
    // re-created in that class; nothing may be in flight (the call drains it).
    int lo = 0, hi = 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));            // lo = least (numerically largest), hi = greatest
    if (value < hi || value > lo) return fail(MAV_ERR_ARG, "option 'stream_priority' must be in [%d, %d], got %ld", hi, lo, value);
    if ((int)value == c->stream_priority) return MAV_OK;
    CHK(mav_worker_drain(c));
    CHK(sync_all_streams(c));
    if (c->copy_stream) HIPCHK(hipStreamSynchronize(c->copy_stream));
    hipStream_t fresh = nullptr;
    HIPCHK(hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, (int)value));
    HIPCHK(hipStreamDestroy(c->stream));
    c->stream = fresh;
    c->stream_priority = (int)value;
    return MAV_OK;
}
static int set_upload_threads(mav_ctx* c, long value)
{
    if (c->stager) return fail(MAV_ERR_STATE, "upload_threads must be set before the first mav_upload_gather call");
    c->upload_threads = (int)value;
    return MAV_OK;
}
// One row per option: its name, its range, the member behind it (an int or a bool), whether it is part of the launch schedule --
// mav_schedule_info prints exactly those, in this order (bench.py hashes the line) -- and, for the options above, the function that
// stores it.  mav_get_option, mav_set_option and mav_schedule_info all go through this table: a new option is one row plus its use.
struct Option {
    const char* name;
    long lo, hi;
    int mav_ctx::*i;
    bool mav_ctx::*b;
    bool in_schedule;
    int (*set)(mav_ctx*, long);
};
static const long kAny = 1L << 40;           // a range the option's own function checks (it depends on the device, or has a text of its own)
static const Option kOptions[] = {
    {"group", 1, 1 << 20, &mav_ctx::group, nullptr, true, set_group},
    {"group_fine", 0, 1 << 20, &mav_ctx::group_fine, nullptr, true, set_group_fine},
    {"bands", 0, 8, &mav_ctx::bands, nullptr, true, set_bands},
    {"pairs_in_flight", 1, 2, &mav_ctx::pairs_in_flight, nullptr, true, nullptr},
    {"band_mb", 8, 1 << 20, &mav_ctx::pif_band_mb, nullptr, true, nullptr},
    {"coarse_cache_mb", 0, 1 << 20, &mav_ctx::coarse_cache_mb, nullptr, true, nullptr},
    {"coarse_half", 0, 1 << 20, &mav_ctx::coarse_half, nullptr, true, nullptr},
    {"share_m", 0, 1, nullptr, &mav_ctx::share_m, true, nullptr},
    {"share_frames", 0, 1, nullptr, &mav_ctx::share_frames, true, nullptr},
    {"strip", 0, 1 << 20, &mav_ctx::strip, nullptr, true, nullptr},
    {"phi_screen", 0, 1, nullptr, &mav_ctx::phi_screen, true, nullptr},
    {"phi_yloop", 0, 1 << 20, &mav_ctx::phi_yloop, nullptr, true, nullptr},
    {"small_batch", 0, 1, nullptr, &mav_ctx::small_batch, true, nullptr},
    {"sweep_write_through", -1, 1, &mav_ctx::sweep_wt, nullptr, true, nullptr},
    {"deep_batch", 0, 1, nullptr, &mav_ctx::deep_batch, true, nullptr},
    {"coarse_bands", 0, 1, nullptr, &mav_ctx::coarse_bands, true, nullptr},
    {"band_phase", 0, 64, &mav_ctx::band_phase, nullptr, true, nullptr},
    {"band_skew", -1, 64, &mav_ctx::band_skew, nullptr, true, nullptr},
    {"deep_frac", 1, 1 << 20, &mav_ctx::deep_frac, nullptr, true, set_deep_frac},
    // not part of the launch schedule: the host side of mav_upload_gather, where uploads go, the compute stream's priority class
    {"upload_threads", 1, 64, &mav_ctx::upload_threads, nullptr, false, set_upload_threads},
    {"inline_uploads", -kAny, kAny, nullptr, &mav_ctx::inline_uploads, false, set_inline_uploads},
    {"stream_priority", -kAny, kAny, &mav_ctx::stream_priority, nullptr, false, set_stream_priority},
    {"cc_workspace_mb", 0, 1 << 20, &mav_ctx::cc_workspace_mb, nullptr, false, nullptr},
};
static const Option* find_option(const char* name)
{
    for (const Option& o : kOptions) if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
static long option_value(const mav_ctx* c, const Option& o) { return o.i ? (long)(c->*o.i) : (long)(c->*o.b); }
extern "C" int mav_get_option(mav_ctx* c, const char* name, long* value)
{
    if (!c || !name || !value) return fail(MAV_ERR_ARG, "mav_get_option: NULL argument");
    const Option* o = find_option(name);
    if (!o) return fail(MAV_ERR_ARG, "unknown option '%s'", name);
    *value = option_value(c, *o);
    return MAV_OK;
}
extern "C" int mav_set_option(mav_ctx* c, const char* name, long value)
{
    if (!c || !name) return fail(MAV_ERR_ARG, "mav_set_option: NULL argument");
    const Option* o = find_option(name);
    if (!o) return fail(MAV_ERR_ARG, "unknown option '%s'", name);
    if (value < o->lo || value > o->hi) return fail(MAV_ERR_ARG, "option '%s' must be in [%ld, %ld], got %ld", name, o->lo, o->hi, value);
    if (o->set) return o->set(c, value);
    if (o->i) c->*o->i = (int)value; else c->*o->b = value != 0;
    return MAV_OK;
}

// The sweeps' window.  Not a row of kOptions: mav_schedule_info prints that table, and a box context's line is pinned byte for byte.
static const GaussTaps* window_taps(const mav_ctx* c) { return c->window == MAV_WINDOW_GAUSSIAN ? &c->gauss : nullptr; }
extern "C" int mav_set_window(mav_ctx* c, int window)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_set_window: NULL context");
    if (window != MAV_WINDOW_BOX && window != MAV_WINDOW_GAUSSIAN)
        return fail(MAV_ERR_ARG, "mav_set_window: window must be MAV_WINDOW_BOX (0) or MAV_WINDOW_GAUSSIAN (1), got %d", window);
    HIPCHK(hipSetDevice(c->device));
    CHK(mav_worker_drain(c));                  // nothing enqueued with the old window is still to come, nothing of it is in flight
    CHK(sync_all_streams(c));
    c->window = window;
    return MAV_OK;
}
extern "C" int mav_get_window(mav_ctx* c, int* window)
{
    if (!c || !window) return fail(MAV_ERR_ARG, "mav_get_window: NULL argument");
    *window = c->window;
    return MAV_OK;
}

extern "C" int mav_num_layers(const mav_ctx* c) { return c ? (int)c->layers.size() : 0; }
extern "C" int mav_layer_dims(const mav_ctx* c, int k, int* w, int* h, int* ksize, double* sigma)
{
    if (!c || k < 0 || k >= (int)c->layers.size()) return fail(MAV_ERR_ARG, "mav_layer_dims: bad layer %d", k);
    if (w) *w = c->layers[k].w; if (h) *h = c->layers[k].h; if (ksize) *ksize = c->layers[k].ksize; if (sigma) *sigma = c->layers[k].sigma;
    return MAV_OK;
}

// Device memory: what the GPU has free / in total (hipMemGetInfo) and what THIS context holds -- the sum of its live device allocations
// as its ledger has them, and of those the Farneback workspace alone (0 until a call computes flow).
extern "C" int mav_mem_info(mav_ctx* c, size_t* dev_free, size_t* dev_total, size_t* ctx_bytes, size_t* workspace_bytes)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_mem_info: NULL context");
    HIPCHK(hipSetDevice(c->device));
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    if (dev_free) *dev_free = fr;
    if (dev_total) *dev_total = tot;
    if (workspace_bytes) *workspace_bytes = c->mem.total(MEM_WORKSPACE);
    if (ctx_bytes) *ctx_bytes = c->mem.total(MEM_WORKSPACE) + c->mem.total(MEM_OTHER);
    return MAV_OK;
}

extern "C" int mav_sync(mav_ctx* c)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_sync: NULL context");
    HIPCHK(hipStreamSynchronize(c->stream));
    return MAV_OK;
}
extern "C" void* mav_stream(mav_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int mav_dev_alloc(mav_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return fail(MAV_ERR_ARG, "mav_dev_alloc: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(out, bytes ? bytes : 1));
    return MAV_OK;
}
extern "C" int mav_dev_free(mav_ctx* c, void* p)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_dev_free: NULL context");
    if (p) HIPCHK(hipFree(p));
    return MAV_OK;
}
extern "C" int mav_memcpy_h2d(mav_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || !dst || !src) return fail(MAV_ERR_ARG, "mav_memcpy_h2d: NULL argument");
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MAV_OK;
}
extern "C" int mav_memcpy_d2h(mav_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || !dst || !src) return fail(MAV_ERR_ARG, "mav_memcpy_d2h: NULL argument");
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MAV_OK;
}

// Pinned host memory + uploads on a second stream: the next batch's frames cross PCIe while the current batch computes.
extern "C" int mav_host_alloc(mav_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return fail(MAV_ERR_ARG, "mav_host_alloc: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return MAV_OK;
}
extern "C" int mav_host_free(mav_ctx* c, void* p)
{
    (void)c;                     // page-locked memory outlives the context that allocated it (NULL context allowed)
    if (p) HIPCHK(hipHostFree(p));
    return MAV_OK;
}
extern "C" int mav_upload_async(mav_ctx* c, void* dst_dev, const void* src_host, size_t bytes)
{
    if (!c || !dst_dev || !src_host) return fail(MAV_ERR_ARG, "mav_upload_async: NULL argument");
    if (c->inline_uploads) { HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream)); return MAV_OK; }
    CHK(ensure_copy_stream(c));
    // the copy may overwrite a buffer that work already enqueued on the compute stream still reads (the previous user of a
    // double-buffered set): order the copy stream behind everything enqueued there so far
    HIPCHK(hipEventRecord(c->compute_mark, c->stream));
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->compute_mark, 0));
    HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->copy_stream));
    return MAV_OK;
}
extern "C" int mav_upload_async_unordered(mav_ctx* c, void* dst_dev, const void* src_host, size_t bytes)
{
    if (!c || !dst_dev || !src_host) return fail(MAV_ERR_ARG, "mav_upload_async_unordered: NULL argument");
    if (c->inline_uploads) { HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream)); return MAV_OK; }
    CHK(ensure_copy_stream(c));
    // no wait for the compute stream: the caller vouches that nothing enqueued so far touches dst_dev (a buffer set that work
    // already enqueued does not use), so the copy overlaps that work whatever the order of the two calls
    HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->copy_stream));
    return MAV_OK;
}
extern "C" int mav_upload_fence(mav_ctx* c)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_upload_fence: NULL context");
    if (c->inline_uploads || !c->copy_stream) return MAV_OK;          // the copies ARE on the compute stream / there have been none
    HIPCHK(hipEventRecord(c->copy_done, c->copy_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->copy_done, 0));   // work enqueued after this call sees the uploaded bytes
    return MAV_OK;
}

static int ensure_gather_event(mav_ctx* c)
{
    if (!c->gather_done) HIPCHK(hipEventCreateWithFlags(&c->gather_done, hipEventDisableTiming));
    return MAV_OK;
}
static int ensure_stager(mav_ctx* c)
{
    if (c->stager) return MAV_OK;
    Stager* s = new Stager();
    for (int i = 0; i < Stager::NCHUNK; i++) {
        if (hipHostMalloc(&s->chunk[i], Stager::CHUNK, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->sent[i], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            s->shutdown();
            delete s;
            return fail(MAV_ERR_OOM, "page-locked staging ring (%d x %zu bytes)", (int)Stager::NCHUNK, (size_t)Stager::CHUNK);
        }
    }
    for (int t = 1; t < c->upload_threads; t++) s->workers.emplace_back([s] { s->worker(); });   // the calling thread is the first copier
    c->stager = s;
    return MAV_OK;
}
// 1: page-locked host memory (send it from where it is); 0: plain host memory (stage it); -1: device memory (a caller's mistake)
static int host_ptr_kind(const void* p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }   // plain malloc'd memory: an error or "unregistered"
    if (a.type == hipMemoryTypeHost) return 1;
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return -1;
    return a.type == hipMemoryTypeManaged ? 1 : 0;
}

extern "C" int mav_upload_gather(mav_ctx* c, void* dst_dev, const void* const* src_host, int count, size_t bytes_each, int flags)
{
    if (!c || !dst_dev || !src_host || count < 1) return fail(MAV_ERR_ARG, "mav_upload_gather: NULL argument or count < 1");
    for (int i = 0; i < count; i++) if (!src_host[i]) return fail(MAV_ERR_ARG, "mav_upload_gather: source %d is NULL", i);
    if (!bytes_each) return MAV_OK;
    const bool ordered = (flags & MAV_GATHER_ORDERED) != 0, held = (flags & MAV_GATHER_SOURCES_HELD) != 0;
    std::vector<int> kind(count);
    for (int i = 0; i < count; i++) {
        kind[i] = (i > 0 && src_host[i] == src_host[i - 1]) ? kind[i - 1] : host_ptr_kind(src_host[i]);
        if (kind[i] < 0) return fail(MAV_ERR_ARG, "mav_upload_gather: source %d is a device pointer (host arrays expected)", i);
        // "on return every source has been read": a page-locked source is read by the DMA engine when the stream gets there.  With
        // inline uploads that is behind whatever the compute stream still has to run -- waiting for it would drain the lane -- so such
        // a source is staged like a pageable one unless the caller vouches that it holds its sources (MAV_GATHER_SOURCES_HELD)
        if (kind[i] == 1 && !held && c->inline_uploads) kind[i] = 0;
    }
    HIPCHK(hipSetDevice(c->device));
    if (!c->inline_uploads) CHK(ensure_copy_stream(c));
    const hipStream_t cs = c->inline_uploads ? c->stream : c->copy_stream;
    if (ordered && !c->inline_uploads) {   // as mav_upload_async: behind everything enqueued on the compute stream so far
        HIPCHK(hipEventRecord(c->compute_mark, c->stream));
        HIPCHK(hipStreamWaitEvent(c->copy_stream, c->compute_mark, 0));
    }
    char* dst = (char*)dst_dev;
    Stager* s = nullptr;
    size_t fill = 0;                           // bytes staged in the chunk being filled
    size_t chunk_dst = 0;                      // device offset the chunk being filled starts at
    bool direct = false;                       // a page-locked source was sent from where it is
    auto flush = [&]() -> int {                // copy the collected segments, send the chunk
        if (!fill) return MAV_OK;
        const unsigned k = s->next_chunk % Stager::NCHUNK;
        s->copy_all();
        s->segs.clear();
        HIPCHK(hipMemcpyAsync(dst + chunk_dst, s->chunk[k], fill, hipMemcpyHostToDevice, cs));
        HIPCHK(hipEventRecord(s->sent[k], cs));
        s->in_flight[k] = true;
        s->next_chunk++;
        fill = 0;
        return MAV_OK;
    };
    auto open_chunk = [&](size_t dev_off) -> int {   // the next ring slot, once its previous transfer has left it
        const unsigned k = s->next_chunk % Stager::NCHUNK;
        if (s->in_flight[k]) { HIPCHK(hipEventSynchronize(s->sent[k])); s->in_flight[k] = false; }
        chunk_dst = dev_off;
        return MAV_OK;
    };
    for (int i = 0; i < count; i++) {
        const char* src = (const char*)src_host[i];
        const size_t dev_off = (size_t)i * bytes_each;
        if (kind[i] == 1) {                    // straight from where it is; whatever was staged before it goes first (keeps nothing waiting)
            if (s) CHK(flush());
            HIPCHK(hipMemcpyAsync(dst + dev_off, src, bytes_each, hipMemcpyHostToDevice, cs));
            direct = true;
            continue;
        }
        if (!s) { CHK(ensure_stager(c)); s = c->stager; }
        size_t done = 0;
        while (done < bytes_each) {
            if (!fill) CHK(open_chunk(dev_off + done));
            const size_t n = std::min(bytes_each - done, Stager::CHUNK - fill);
            char* into = (char*)s->chunk[s->next_chunk % Stager::NCHUNK] + fill;
            for (size_t o = 0; o < n; o += Stager::PIECE)
                s->segs.push_back({into + o, src + done + o, std::min(Stager::PIECE, n - o)});
            fill += n; done += n;
            if (fill == Stager::CHUNK) CHK(flush());
        }
    }
    if (s) {
        CHK(flush());
        // the staged sources have been read; the ring's last transfers may still be in flight (the next call waits for a slot before it refills it)
    }
    if (direct && !held) {
        // page-locked sources sent from where they are (copy stream: nothing but copies ahead of them): the caller may overwrite them
        // when this call returns, so wait until the engine has read them
        CHK(ensure_gather_event(c));
        HIPCHK(hipEventRecord(c->gather_done, cs));
        HIPCHK(hipEventSynchronize(c->gather_done));
    }
    return MAV_OK;
}

extern "C" int mav_download_async(mav_ctx* c, void* dst_host, const void* src_dev, size_t bytes)
{
    if (!c || !dst_host || !src_dev) return fail(MAV_ERR_ARG, "mav_download_async: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return MAV_OK;
}

// Markers: "everything enqueued on the context's stream so far" as an object the host can wait for without draining the stream
// (mav_sync waits for the work enqueued AFTER the marker too).  The pipelined loop records one per batch.
extern "C" int mav_marker_create(mav_ctx* c, void** out)
{
    if (!c || !out) return fail(MAV_ERR_ARG, "mav_marker_create: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = (void*)e;
    return MAV_OK;
}
extern "C" int mav_marker_record(mav_ctx* c, void* marker)
{
    if (!c || !marker) return fail(MAV_ERR_ARG, "mav_marker_record: NULL argument");
    HIPCHK(hipEventRecord((hipEvent_t)marker, c->stream));
    return MAV_OK;
}
extern "C" int mav_marker_wait(mav_ctx* c, void* marker)
{
    // Waiting needs no context, and a marker may outlive the one it was recorded on -- as an object.  Once that context is destroyed
    // everything the marker stood behind has finished (mav_destroy drains the streams) and the caller must answer "done" by itself, as
    // the Python layer's _Marker does: the runtime's event still refers to the stream it was last recorded on, which is gone.
    (void)c;
    if (!marker) return fail(MAV_ERR_ARG, "mav_marker_wait: NULL marker");
    HIPCHK(hipEventSynchronize((hipEvent_t)marker));
    return MAV_OK;
}
extern "C" int mav_marker_query(mav_ctx* c, void* marker, int* done)
{
    (void)c;
    if (!marker || !done) return fail(MAV_ERR_ARG, "mav_marker_query: NULL argument");
    const hipError_t e = hipEventQuery((hipEvent_t)marker);
    if (e == hipSuccess) { *done = 1; return MAV_OK; }
    if (e == hipErrorNotReady) { (void)hipGetLastError(); *done = 0; return MAV_OK; }
    HIPCHK(e);
    return MAV_OK;
}
extern "C" int mav_marker_destroy(mav_ctx* c, void* marker)
{
    (void)c;
    if (marker) HIPCHK(hipEventDestroy((hipEvent_t)marker));
    return MAV_OK;
}

extern "C" int mav_timer_start(mav_ctx* c)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_timer_start: NULL context");
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return MAV_OK;
}
extern "C" int mav_timer_stop(mav_ctx* c, float* ms)
{
    if (!c || !ms) return fail(MAV_ERR_ARG, "mav_timer_stop: NULL argument");
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    HIPCHK(hipEventElapsedTime(ms, c->t0, c->t1));
    return MAV_OK;
}

static int prof_collect(mav_ctx* c)
{
    while (!c->open_runs.empty()) close_run(c, c->open_runs.size() - 1);
    if (c->prof.empty()) return MAV_OK;
    CHK(sync_all_streams(c));
    for (auto& r : c->prof) {
        float ms = 0, t0 = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            c->prof_ms[r.kid] += ms; c->prof_n[r.kid]++;
            if (c->prof_base && hipEventElapsedTime(&t0, c->prof_base, r.a) == hipSuccess) c->prof_iv.push_back({r.kid, t0, t0 + ms, r.stream});
        }
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    c->prof.clear();
    return MAV_OK;
}
extern "C" int mav_profile_enable(mav_ctx* c, int on)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_profile_enable: NULL context");
    CHK(prof_collect(c));
    if (on) {
        memset(c->prof_ms, 0, sizeof(c->prof_ms)); memset(c->prof_n, 0, sizeof(c->prof_n));
        c->prof_iv.clear();
        if (!c->prof_base) HIPCHK(hipEventCreate(&c->prof_base));
        HIPCHK(hipEventRecord(c->prof_base, c->stream));
    }
    c->profiling = on == 2 ? 2 : (on != 0);
    return MAV_OK;
}
// Time during which at least one launch of the named kernel classes (comma-separated names of mav_profile_get) was running:
// the union of the profiled launches' intervals.  With two pairs in flight launches of one class overlap, their summed
// durations exceed the wall time and this is the figure a rate has to be quoted on.
extern "C" int mav_profile_busy(mav_ctx* c, const char* names, double* busy_ms)
{
    if (!c || !names || !busy_ms) return fail(MAV_ERR_ARG, "mav_profile_busy: NULL argument");
    CHK(prof_collect(c));
    bool want[K_COUNT] = {false};
    for (int i = 0; i < K_COUNT; i++) {
        const char* p = strstr(names, kKernelNames[i]);
        const size_t len = strlen(kKernelNames[i]);
        while (p) {                                          // whole-name match between commas
            if ((p == names || p[-1] == ',') && (p[len] == 0 || p[len] == ',')) { want[i] = true; break; }
            p = strstr(p + 1, kKernelNames[i]);
        }
    }
    std::vector<std::pair<float, float>> iv;
    for (const auto& r : c->prof_iv) if (want[r.kid]) iv.push_back({r.t0, r.t1});
    std::sort(iv.begin(), iv.end());
    double busy = 0;
    float lo = 0, hi = -1;
    for (const auto& x : iv) {
        if (hi < lo || x.first > hi) { if (hi >= lo) busy += hi - lo; lo = x.first; hi = x.second; }
        else if (x.second > hi) hi = x.second;
    }
    if (hi >= lo) busy += hi - lo;
    *busy_ms = busy;
    return MAV_OK;
}
// Every profiled launch (mode 1) or run of launches (mode 2) since mav_profile_enable as an interval: class index (order of
// mav_profile_get), stream (0 = the context's stream, 1 = its second compute stream), start / end in ms since the profile was switched
// on.  *n: capacity in, count out (the total when the arrays are NULL).
extern "C" int mav_profile_intervals(mav_ctx* c, int* n, int* kernel_class, int* stream, float* t0_ms, float* t1_ms)
{
    if (!c || !n) return fail(MAV_ERR_ARG, "mav_profile_intervals: NULL argument");
    CHK(prof_collect(c));
    const int total = (int)c->prof_iv.size();
    if (!kernel_class || !stream || !t0_ms || !t1_ms) { *n = total; return MAV_OK; }
    const int k = total < *n ? total : *n;
    for (int i = 0; i < k; i++) {
        kernel_class[i] = c->prof_iv[i].kid; stream[i] = c->prof_iv[i].stream; t0_ms[i] = c->prof_iv[i].t0; t1_ms[i] = c->prof_iv[i].t1;
    }
    *n = k;
    return MAV_OK;
}
extern "C" int mav_profile_get(mav_ctx* c, int* n, const char** names, double* total_ms, long* launches)
{
    if (!c || !n) return fail(MAV_ERR_ARG, "mav_profile_get: NULL argument");
    CHK(prof_collect(c));
    int cap = *n, k = 0;
    for (int i = 0; i < K_COUNT && k < cap; i++, k++) {
        if (names) names[k] = kKernelNames[i];
        if (total_ms) total_ms[k] = c->prof_ms[i];
        if (launches) launches[k] = c->prof_n[i];
    }
    *n = k;
    return MAV_OK;
}

// Calibration: GB/s of a plain 3-reads-1-write float4 streaming kernel over four buffers of bytes_per_buffer each (the sweeps' mix).
extern "C" int mav_membw_probe(mav_ctx* c, size_t bytes_per_buffer, int reps, double* gbs)
{
    if (!c || !gbs || reps < 1 || bytes_per_buffer < 4096) return fail(MAV_ERR_ARG, "mav_membw_probe: bad argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = bytes_per_buffer & ~(size_t)4095;
    float* buf[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = c->mem.alloc_set({{&buf[0], bytes}, {&buf[1], bytes}, {&buf[2], bytes}, {&buf[3], bytes}}, MEM_OTHER, "mav_membw_probe");
    float ms = 0.f;
    if (rc == MAV_OK) {
        for (int i = 0; i < 3; i++) hipMemsetAsync(buf[i], 0, bytes, c->stream);
        for (int w = 0; w < 2; w++) launch_probe_r3w1(c->stream, buf[0], buf[1], buf[2], buf[3], bytes / 16);
        hipEventRecord(c->t0, c->stream);
        for (int r = 0; r < reps; r++) launch_probe_r3w1(c->stream, buf[0], buf[1], buf[2], buf[3], bytes / 16);
        hipEventRecord(c->t1, c->stream);
        if (hipEventSynchronize(c->t1) != hipSuccess || hipEventElapsedTime(&ms, c->t0, c->t1) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = fail(MAV_ERR_HIP, "mav_membw_probe: launch or timing failed");
    }
    for (float* b : buf) c->mem.release(b);
    if (rc == MAV_OK) *gbs = 4.0 * (double)bytes * reps / (ms * 1e-3) / 1e9;
    return rc;
}

static int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MAV_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return MAV_OK;
}
// The prologue of an entry point that takes a batch: a context, a batch it was created for, its device current.
static int check_dev_call(mav_ctx* c, int batch, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (batch < 1 || batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    HIPCHK(hipSetDevice(c->device));
    return MAV_OK;
}
// The caller's parameters, or the defaults where it passed NULL.
static mav_thr_params thr_or_defaults(const mav_thr_params* tp)
{
    mav_thr_params t;
    if (tp) t = *tp; else mav_thr_defaults(&t);
    return t;
}
static int foe_or_defaults(const mav_foe_params* fp, mav_foe_params* f)
{
    if (fp) *f = *fp; else mav_foe_defaults(f);
    if (f->n_pairs < 1 || f->n_pairs > 4096) return fail(MAV_ERR_ARG, "n_pairs %d outside [1, 4096]", f->n_pairs);
    return MAV_OK;
}

// ---- Farneback: the schedule of one group of pairs --------------------------------------------------------------------
static BlurParams blur_of(const mav_ctx* c, const Layer& l)
{
    BlurParams bp{l.ksize, (l.ksize == 3 && l.sigma <= 0) ? 1 : 0, l.g, (double)c->W / l.w, (double)c->H / l.h, nullptr, nullptr, nullptr, nullptr};
    if (l.coord) {
        bp.xs = l.coord; bp.xf = (const float*)(l.coord + l.w);
        bp.ys = l.coord + 2 * l.w; bp.yf = (const float*)(l.coord + 2 * l.w + l.h);
    }
    return bp;
}

// How the sweeps of layer k run for a group of g pairs: plan_sweeps decides, layer_sweeps executes, mav_schedule_info reports -- all
// from these fields alone.  The group is cut into sub-groups of per_launch pairs; sub-group i runs on stream i & 1 of `streams`.
enum MBuild { M_GROUP, M_SUB, M_BAND };          // the initial M: of the whole group up front / of a sub-group right before its sweeps /
                                                 // of a sub-group band by band, right before each band's first sweep
enum MSlot { SLOT_OWN, SLOT_FIRST, SLOT_ALTERNATE };   // the M buffers of the sub-group that starts at pair s0: slot s0 / slot 0 (option
                                                       // "share_m") / slot (i & 1) * per_launch, one set per stream
struct SweepPlan {
    const char* name;     // what mav_schedule_info calls it
    int per_launch;       // pairs per sub-group = per launch
    int streams;          // 1: the compute stream; 2: sub-groups alternate between it and pair_stream (one fork and one join per group)
    int J;                // horizontal bands per pair (one pair per launch); 1 = sweep-major
    bool shift_second;    // the second stream's sub-groups use the partition shifted by half a band (option "band_phase")
    MBuild m_build;
    MSlot m_slot;
    bool write_through;   // the sweeps' M' through write-through stores (option "sweep_write_through": by default with two streams only)
};
static SweepPlan plan_sweeps(const mav_ctx* c, int k, int g, bool bands_ok)
{
    const Layer& l = c->layers[k];
    const int T = blur_iter_tile_rows(l.h), I = c->fb.iterations;
    auto wt = [&](int streams) { return c->sweep_wt < 0 ? streams == 2 : c->sweep_wt != 0; };
    int sub = g;
    // The finest layer's ten sweeps re-read R0/R1 and M: run them `group_fine` pairs at a time so that one sub-group's working
    // set stays resident in the 256 MB Infinity Cache between sweeps.  Coarse layers are small: as many pairs per launch as keep
    // the sweeps' working set cache-sized, to fill the 256 CUs.
    if (k == 0 && c->group_fine > 0 && c->group_fine < g) sub = c->group_fine;
    if (k > 0 && c->coarse_cache_mb > 0) {
        const size_t ws = (size_t)l.w * l.h * 80, cap = (size_t)c->coarse_cache_mb << 20;
        const int fit = (int)(cap / (ws ? ws : 1));
        if (fit < sub) sub = fit > 1 ? fit : 1;
    }
    // with per-sub-group sweeps the initial M of a sub-group is built right before its sweeps: M, R0 and R1 are then still in the
    // Infinity Cache when the first sweep reads them (measured -0.5 ms per 64 pairs; doing the same with the blur and the expansion
    // costs more in small launches than it returns)
    bool m_per_sub = sub < g;
    const size_t ws_pair = (size_t)l.w * l.h * 80, band_bytes = (size_t)c->pif_band_mb << 20;
    // A COARSE layer whose per-pair working set exceeds a band (layer 1 of the 4K preset: 1536 x 864, 106 MB) is swept exactly like the
    // finest one: pairs alternate between the two streams, each band-major, so that the two pairs in flight occupy 2 x <= band_mb of the
    // Infinity Cache instead of 2 x 106 MB (option "coarse_bands").
    const bool big_coarse = k > 0 && c->coarse_bands && bands_ok && ws_pair > band_bytes && T / (I + 2) >= 2;
    if (big_coarse) { sub = 1; m_per_sub = true; }
    if (k > 0 && !big_coarse && c->pairs_in_flight == 2 && g >= 2) {
        // COARSE LAYERS with two sub-groups in flight: sub-groups of half the cache-sized count alternate between the compute stream
        // and pair_stream, each with its own M slots, for the same reason as the pairs of the finest layer below -- 25.5 - 25.6 vs
        // 26.0 - 26.6 ms per 64 pairs at 1080p with 4 + 4 instead of 8 pairs per launch (3 + 3: 25.7 - 25.8; 8 + 8: 26.4;
        // profiles/r02/ab_coarse_two*.log).
        int half = sub / 2 > 0 ? sub / 2 : 1;
        if (c->coarse_half > 0) half = c->coarse_half;
        if (2 * half > g) half = (g + 1) / 2;
        return {"two sub-groups in flight", half, 2, 1, false, M_SUB, SLOT_ALTERNATE, wt(2)};
    }
    if ((k == 0 || big_coarse) && c->pairs_in_flight == 2 && m_per_sub && sub == 1 && g >= 2) {
        // TWO PAIRS IN FLIGHT (finest layer, one pair per launch).  Pair s of the group runs on stream s & 1 -- the compute stream
        // and pair_stream -- and ping-pongs M through slot s & 1.  The two streams never wait for each other inside the group
        // (different pairs: no dependency; one fork and one join event per group), so one stream's launches fill the kernel
        // boundaries and the fill / drain of the other's.  What keeps this inside the 256 MB Infinity Cache is the band-major order:
        // each pair is swept (and its initial M built) band by band, bands of at most band_mb (96 MB) of working set -- 2 bands at 1080p, 7 at
        // 3840x2160 -- so the hot set is 2 x 83 MB, what ONE whole 1080p pair occupies in the one-stream schedule.  Measured
        // (profiles/r02/ab_two_pairs*.log): 1080p 25.9 - 26.3 vs 27.1 - 27.4 ms per 64 pairs, 4K 28.7 vs 30.1 ms per 16 pairs; two full
        // pairs without bands 28.6 ms, three or four streams 27.9 - 28.1 ms.  Same tiles, same arithmetic as every other schedule:
        // bit-identical flow (tests/test_gpu_flow.py).
        int J = (c->bands_set && k == 0) ? c->bands : (int)((ws_pair + band_bytes - 1) / band_bytes);
        const int Jmax = T / (I + 2);          // a band needs iterations + 2 tile rows (the skew must not reach the image top)
        if (J > Jmax) J = Jmax;
        if (J < 1) J = 1;
        if (J == 1 || bands_ok)
            return {"two pairs in flight, band-major", 1, 2, J, J > 1 && c->band_phase && J >= c->band_phase, J > 1 ? M_BAND : M_SUB,
                    SLOT_ALTERNATE, wt(2)};
    }
    // ONE STREAM: sub-groups are swept one after the other, so they all ping-pong M through the SAME two buffers (the first
    // sub-group's slots; option "share_m"): the M lines then stay hot in the Infinity Cache from pair to pair instead of leaving a
    // dead 83 MB copy behind per pair.  Measured at 1080p, 64 pairs: 27.6 / 28.0 ms shared vs 28.2 / 28.6 ms with per-slot buffers.
    // Bands (finest layer, one pair per launch) of at least iterations + 2 tile rows each: the pair's whole initial M first, then the
    // sweeps band-major.
    const int J = (k == 0 && (m_per_sub || g == 1) && sub == 1 && T >= (I + 2) * c->bands && bands_ok) ? c->bands : 1;
    return {"one stream", sub, 1, J, false, m_per_sub ? M_SUB : M_GROUP, (m_per_sub && c->share_m) ? SLOT_FIRST : SLOT_OWN, wt(1)};
}

// The `iterations` sweeps of gs pairs on stream st.  J > 1: the sweeps of one pair in BAND-MAJOR order, for frames whose per-pair working set (80 B per pixel: M in, M out,
// R0, R1) does not fit the 256 MB Infinity Cache -- 664 MB at 3840x2160.  The image is cut into J horizontal bands of tile rows
// and ALL sweeps of a band run before the next band starts, so that a band's M, R0 and R1 stay cache-resident across its sweeps
// exactly as a whole 1080p pair does.  What makes this legal without recomputing halos is a skew: sweep `it` processes band j as
// tile rows [A_j - it, A_(j+1) - it) (16 pixel rows per tile row; the first band starts at row 0, the last ends at the bottom).
//   * reads: sweep it on band j needs sweep it - 1 within 6 pixels of its rows = output of (it - 1, j), just computed, and of
//     (it - 1, j - 1), computed with the previous band;
//   * the M ping-pong: (it, j) writes the buffer that (it - 1, j + 1) will read later, but only up to tile row A_(j+1) - it - 1,
//     while that reader starts 6 pixels above tile row A_(j+1) - it + 1; and the rows of band j - 1 that (it, j) itself reads have
//     been overwritten by (it + 1, j - 1) only up to one tile row above them.  A skew of one tile row (16 >= 6 pixels) covers both.
// Every tile is computed exactly once on the same tile grid: results are bit-identical to the sweep-major schedule
// (tests/test_gpu_flow.py).  One stream, no events.  J = 1 is the sweep-major order: every sweep one launch over all tile rows, for
// any number of pairs gs and any kernel form (bands of their own exist for one pair and the fast form only: blur_iter_bands_ok).
// upd != nullptr: the initial M (UpdateMatrices from the coarser layer's flow) is built band by band too, right before a band's
// first sweep: pixel rows [16 a0 - 8, 16 a1 + 8) -- what that sweep reads (6-pixel halo) -- which lie below everything the bands
// above have written into Ma (their odd sweeps end one whole tile row higher); the rows two neighbouring bands both need are
// simply built twice, to the same values.
// a: the operands every sweep of the run shares; M_in / M_out (the ping-pong through Ma / Mb), do_update, store_flow, ty0 and ty1 are
// set per launch here.
struct BandRun { float *Ma, *Mb; int kid /* profile class of the sweeps */, J, phase; };
// phase = 1 (the pairs of the second stream, option "band_phase", off by default): the partition is shifted by half a band -- J + 1 bands,
// the first and the last of half size.  Two streams that start a group together with the same partition stay in lockstep: both build a
// band's initial M (HBM-bound) at the same moments and both sweep (cache-bound) at the same moments -- untraced at 3840x2160: 1.3 ms per
// step with two initial-M launches running and no sweep, 1.0 ms with one (tools/untraced_anatomy.py).  Shifted by half a band, one
// stream's initial M does fall into the other's sweeps (3.6 ms per step) -- and the step gets SLOWER: 581 vs 602 pairs/s at 4K, 2 320 vs
// 2 630 at 1080p (profiles/r04/ab_band_phase.log): the 66 MB a band's initial M streams in from HBM push the sweeping pair's band out
// of the Infinity Cache (sweep launches 37.1 vs 34.6 ms summed).  The lockstep is worth keeping.  (Those figures were taken while bound()
// divided by 2 (J + 1) instead of 2 J -- a first band of half a band's size and a last one of one and a half; tests/test_gpu_schedule_forms.py
// now holds the partition to the one described here.)  The band arguments above hold for any
// monotone sequence of boundaries (a band whose rows have all moved above the image top at a late sweep is empty and skipped; its
// successor then starts at row 0): bit-identical (tests/test_gpu_flow.py).
static void sweeps_band_major(mav_ctx* c, hipStream_t st, SweepArgs a, const BandRun& run, const FlowSource* upd)
{
    const int I = c->fb.iterations, T = blur_iter_tile_rows(a.h), phase = run.phase;
    const int J = run.J, NBands = phase ? J + 1 : J;
    auto bound = [&](int j) -> int {                      // first tile row of band j; bound(NBands) = T
        if (j <= 0) return 0;
        if (j >= NBands) return T;
        if (phase) return (int)((long long)T * (2 * j - 1) / (2 * J));      // (J = the unshifted partition's count: half a band of ITS size)
        // Sweep `it` shifts every boundary up by `it` tile rows: over a band's sweeps the first band loses (I - 1) / 2 rows on average
        // and the last one gains as many.  Boundaries moved down by that amount give every band the same AVERAGE size -- launches and
        // cache footprints stay even (option "band_skew"; 1080p: first band 38 of 68 tile rows instead of 34; equal split: 0).
        int b = (int)((long long)T * j / J) + (c->band_skew < 0 ? (I - 1) / 2 : c->band_skew);
        const int lo = j, hi = T - (NBands - j);             // at least one tile row per band
        return b < lo ? lo : (b > hi ? hi : b);
    };
    for (int j = 0; j < NBands; j++) {
        const int a0 = bound(j), a1 = bound(j + 1);
        if (a1 <= a0) continue;
        if (upd) {
            ProfScope ps(c, K_UPDATE, st);
            launch_initial_m(st, {a, run.Ma, a.M_stride, a0 == 0 ? 0 : a0 * 16 - 8, j == NBands - 1 ? a.h : a1 * 16 + 8}, *upd);
        }
        for (int it = 0; it < I; it++) {
            const int update = it < I - 1;
            int ty0 = a0 - it, ty1 = j == NBands - 1 ? T : a1 - it;
            if (ty0 < 0) ty0 = 0;
            if (ty1 <= ty0) continue;
            ProfScope ps(c, run.kid, st);
            a.M_in = (it & 1) ? run.Mb : run.Ma; a.M_out = (it & 1) ? run.Ma : run.Mb;
            a.do_update = update; a.store_flow = !update; a.ty0 = ty0; a.ty1 = ty1;
            launch_blur_iter(st, a);
        }
    }
}

// Where layer k of a walk of g pairs finds its expansions (pair 0's two; slot stride rs) and puts its flow (slot stride fstride), and
// the slot stride ms of the M buffers at that layer.
struct LayerIO { int k, g; const float *r0, *r1; size_t rs; float* flow; size_t fstride, ms; };
struct MBuffers { float *a, *b; };               // M ping-pongs through them
// Initial M and the `iterations` sweeps of layer io.k for io.g pairs, starting on stream st; the initial flow comes from `src` (the
// coarser layer's flow; zero or the call's initial flow at the top layer).  On return everything has been joined back into st.
static int layer_sweeps(mav_ctx* c, hipStream_t st, const LayerIO& io, const FlowSource& src, const MBuffers& m)
{
    const int k = io.k, g = io.g;
    const Layer& l = c->layers[k];
    const size_t ms = io.ms, rs = io.rs;
    const PairOperands group{io.r0, io.r1, rs, g, l.w, l.h};
    SweepArgs sa{group, m.a, m.b, ms, c->fb.winsize, io.flow, io.fstride, 1, 0};
    sa.strip = c->strip; sa.gauss = window_taps(c);
    const SweepPlan p = plan_sweeps(c, k, g, blur_iter_bands_ok(sa));
    sa.write_through = p.write_through;
    if (p.streams == 2) {
        CHK(ensure_pair_stream(c));
        HIPCHK(hipEventRecord(c->pif_fork, st));
        HIPCHK(hipStreamWaitEvent(c->pair_stream, c->pif_fork, 0));
    }
    if (p.m_build == M_GROUP) {
        ProfScope ps(c, K_UPDATE, st);
        launch_initial_m(st, {group, m.a, ms}, src);
    }
    // With two streams the host alternates between them sub-group by sub-group, and within a pair band by band (a band's initial M, then
    // all its sweeps): the two streams never wait for each other inside the group.
    for (int s0 = 0, i = 0; s0 < g; s0 += p.per_launch, i++) {
        const int gs = g - s0 < p.per_launch ? g - s0 : p.per_launch;
        const bool second = p.streams == 2 && (i & 1);
        const hipStream_t ss = second ? c->pair_stream : st;
        const size_t m_off = p.m_slot == SLOT_OWN ? (size_t)s0 * ms : p.m_slot == SLOT_FIRST ? 0 : (size_t)(i & 1) * p.per_launch * ms;
        sa.R0 = io.r0 + (size_t)s0 * rs; sa.R1 = io.r1 + (size_t)s0 * rs; sa.G = gs;
        sa.flow = io.flow + (size_t)s0 * io.fstride;
        const FlowSource bu = src.from_pair(s0);
        if (p.m_build == M_SUB) {
            ProfScope ps(c, K_UPDATE, ss);
            launch_initial_m(ss, {sa, m.a + m_off, ms}, bu);
        }
        sweeps_band_major(c, ss, sa, {m.a + m_off, m.b + m_off, k == 0 ? K_ITER : K_ITER_COARSE, p.J, p.shift_second && second},
                          p.m_build == M_BAND ? &bu : nullptr);
    }
    if (p.streams == 2) {
        prof_close_stream(c, c->pair_stream); prof_close_stream(c, st);
        HIPCHK(hipEventRecord(c->pif_join, c->pair_stream));
        HIPCHK(hipStreamWaitEvent(st, c->pif_join, 0));
    }
    return MAV_OK;
}

// Layer images and polynomial expansions of both frames of g pairs at layer k, on stream st, through image buffer I into the
// expansion set R (R0 | R1 in one piece); *r0 / *r1 = where pair 0's two expansions lie (pair s: + s * 5 n0).
// seq: `prev` is a run of g + 1 consecutive frames and pair s = (frame s, frame s + 1): every frame is blurred and expanded ONCE.
// Otherwise, when the 2 g layer images are small (merge_frames), prev and next go through ONE blur and ONE expansion launch of 2 g
// images instead of two of g: a group of one or two pairs is bound by launch latency, not by bytes.
template <typename T>
static void layer_expansions(mav_ctx* c, hipStream_t st, int k, const T* prev, const T* next, int g, bool seq, float* I, float* R,
                             const float** r0, const float** r1)
{
    mav_ctx::WorkSet& w = c->ws;
    const size_t n0 = c->n0;
    const Layer& l = c->layers[k];
    const LayerTarget target{I, n0, blur_of(c, l), l.w, l.h};
    const BlurScratch scratch{w.Htmp, c->htmp_stride};
    auto frames = [&](const T* a, const T* b, int split, int G) { return FrameRun<T>{a, b, split, n0, G, c->W, c->H}; };
    if (seq) {
        { ProfScope ps(c, K_BLUR_RESIZE, st);
          launch_blur_resize(st, frames(prev, nullptr, 0, g + 1), target, scratch); }
        { ProfScope ps(c, K_POLYEXP, st);
          launch_polyexp(st, I, n0, g + 1, l.w, l.h, c->pc, R, 5 * n0); }
        *r0 = R; *r1 = R + 5 * n0;
        return;
    }
    float* R1 = R + 5 * n0 * (size_t)g;
    *r0 = R; *r1 = R1;
    // (the two-pass blur's scratch holds g + 1 frames)
    const bool no_tmp = !blur_resize_needs_tmp(frames(prev, next, g, 2 * g), target);
    const bool merge_frames = (no_tmp || 2 * g <= g + 1) && (size_t)2 * g * l.w * l.h * sizeof(float) <= ((size_t)48 << 20);
    if (merge_frames) {
        { ProfScope ps(c, K_BLUR_RESIZE, st);
          launch_blur_resize(st, frames(prev, next, g, 2 * g), target, scratch); }
        { ProfScope ps(c, K_POLYEXP, st);
          launch_polyexp(st, I, n0, 2 * g, l.w, l.h, c->pc, R, 5 * n0); }
        return;
    }
    const T* img[2] = {prev, next};
    float* Rs[2] = {R, R1};
    for (int i = 0; i < 2; i++) {
        { ProfScope ps(c, K_BLUR_RESIZE, st);
          launch_blur_resize(st, frames(img[i], nullptr, 0, g), target, scratch); }
        { ProfScope ps(c, K_POLYEXP, st);
          launch_polyexp(st, I, n0, g, l.w, l.h, c->pc, Rs[i], 5 * n0); }
    }
}

// does a group of g pairs take the small-group schedule?
static bool is_small_group(const mav_ctx* c, int g)
{
    return c->small_batch && c->layers.size() > 1 && (int)c->layers.size() <= MAV_MAX_JOBS && g <= c->small_g &&
           (size_t)g * c->n0 * 80 <= ((size_t)c->small_batch_mb << 20);
}

// The layer images of layers k_lo .. k_hi for the frames f into regions Ik(k) with slot stride sk(k): every layer blur_multi_ok accepts through ONE launch, the others (long Gaussians)
// through the two-pass kernels in chunks the H x w scratch holds; then ALL their expansions through one launch (per MAV_MAX_JOBS layers).
template <typename T, typename IkFn, typename RkFn, typename SkFn>
static void pyramid_multi(mav_ctx* c, hipStream_t st, const FrameRun<T>& f, int k_lo, int k_hi, IkFn Ik, RkFn Rk, SkFn sk)
{
    mav_ctx::WorkSet& w = c->ws;
    const size_t n0 = c->n0;
    const int F = f.G;
    BlurJobs bj{0, 0, {}};
    PolyJobs pj{0, 0, {}};
    auto flush_blur = [&]() { if (bj.n) { ProfScope ps(c, K_BLUR_RESIZE, st); launch_blur_multi(st, f, bj); bj.n = 0; } };
    auto flush_poly = [&]() { if (pj.n) { ProfScope ps(c, K_POLYEXP, st); launch_polyexp_multi(st, pj, F, c->pc); pj.n = 0; } };
    for (int k = k_lo; k <= k_hi; k++) {
        const Layer& l = c->layers[k];
        const LayerTarget target{Ik(k), sk(k), blur_of(c, l), l.w, l.h};
        if (blur_multi_ok(f, target)) {
            if (bj.n == MAV_MAX_JOBS) flush_blur();
            static_cast<LayerTarget&>(bj.j[bj.n++]) = target;
        } else {
            // a long Gaussian (or an unaligned finest layer): launches of its own.  The two-pass scratch holds (group + 1) H x W floats;
            // a frame needs H x w of it
            ProfScope ps(c, K_BLUR_RESIZE, st);
            const size_t per = (size_t)c->H * l.w, cap_frames = (c->htmp_stride * (size_t)(c->group + 1)) / per;
            const int chunk = (int)(cap_frames < (size_t)F ? cap_frames : (size_t)F);
            for (int f0 = 0; f0 < F; f0 += chunk) {
                const int n = F - f0 < chunk ? F - f0 : chunk;
                const bool from2 = f.img2 && f0 >= f.split;
                const T* a = from2 ? f.img2 + (size_t)(f0 - f.split) * n0 : f.img + (size_t)f0 * n0;
                LayerTarget chunk_target = target;
                chunk_target.out += (size_t)f0 * sk(k);
                launch_blur_resize(st, FrameRun<T>{a, from2 ? nullptr : f.img2, from2 ? 0 : f.split - f0, n0, n, c->W, c->H}, chunk_target, {w.Htmp, per});
            }
        }
        if (pj.n == MAV_MAX_JOBS) { flush_blur(); flush_poly(); }
        PolyJob& P = pj.j[pj.n++];
        P.I = Ik(k); P.R = Rk(k); P.I_stride = sk(k); P.R_stride = 5 * sk(k); P.w = l.w; P.h = l.h;
    }
    flush_blur();
    flush_poly();
}

// Layers k_hi .. k_lo, top-down: `at(k)` makes layer k's expansions (unless they exist already) and says where they and the layer's
// flow lie; then the layer's initial M and sweeps (layer_sweeps), from the flow of the layer above.  src: where layer k_hi's initial
// flow comes from (top_flow at the top of the pyramid, else the flow of layer k_hi + 1: coarser_flow).
static FlowSource coarser_flow(const mav_ctx* c, int k_coarser, const float* flow, size_t stride)
{
    const Layer& l = c->layers[k_coarser];
    return FlowSource::coarser(flow, stride, l.w, l.h, (float)(1. / c->fb.pyr_scale));
}
// the top layer's: the call's initial flow (init_snap, the layer's own size) or zero
static FlowSource top_flow(const mav_ctx* c, const float* flow_init) { return flow_init ? FlowSource::field(flow_init, c->init_stride) : FlowSource{}; }
template <typename AtFn>
static int walk_layers(mav_ctx* c, hipStream_t st, int k_hi, int k_lo, AtFn at, const MBuffers& m, FlowSource src)
{
    for (int k = k_hi; k >= k_lo; k--) {
        const LayerIO io = at(k);
        CHK(layer_sweeps(c, st, io, src, m));
        src = coarser_flow(c, k, io.flow, io.fstride);
    }
    return MAV_OK;
}

// DEEP LAYERS (kd .. top) of D pairs at once, on the compute stream; the flow of layer kd lands in deep.f[kd & 1], slot stride
// 2 * c_stride[kd].  See mav_ctx::DeepSet.  Same tile functions on the same data as the per-group path: bit-identical flow.
// flow_init: the top layer's initial flow of the D pairs (init_snap) or nullptr.
template <typename T>
static int deep_layers(mav_ctx* c, hipStream_t st, const T* prev, const T* next, int D, bool seq, const float* flow_init = nullptr)
{
    const int L = (int)c->layers.size(), kd = c->kd;
    const int F = seq ? D + 1 : 2 * D;
    const size_t base = c->c_off[kd];
    auto Ik = [&](int k) { return c->deep.I + (size_t)F * (c->c_off[k] - base); };
    auto Rk = [&](int k) { return c->deep.R + 5 * (size_t)F * (c->c_off[k] - base); };
    auto sk = [&](int k) { return c->c_stride[k]; };
    pyramid_multi(c, st, FrameRun<T>{prev, seq ? nullptr : next, D, c->n0, F, c->W, c->H}, kd, L - 1, Ik, Rk, sk);
    auto at = [&](int k) {
        const size_t rs = 5 * sk(k);
        return LayerIO{k, D, Rk(k), Rk(k) + (seq ? rs : rs * (size_t)D), rs, c->deep.f[k & 1], 2 * sk(k), rs};
    };
    return walk_layers(c, st, L - 1, kd, at, {c->deep.Ma, c->deep.Mb}, top_flow(c, flow_init));
}

// One group of g pairs: every coarse layer completely (top layer first: images, expansions, initial M, sweeps), then the finest layer.
// deep_flow != nullptr: the layers from kd up have been computed already (deep_layers); the group starts at layer kd - 1 with
// deep_flow (this group's first pair; slot stride deep_stride) as its coarser layer.  flow_init: the top layer's initial flow of the g
// pairs (init_snap; only without deep_flow) or nullptr.
// SMALL GROUPS (is_small_group: one 1080p pair, two 720p pairs ...; BASELINE config 2) are a chain of ~30 dependent launches that
// each fill a fraction of the chip, ~4.5 us of boundary apiece.  For them the whole pyramid's layer images come from ONE launch and
// all expansions from ONE launch (k_blur_multi / k_polyexp_multi: the workgroups of several layers in one grid, every layer into a
// region of its own in Ic / Rc), instead of two launches per layer: the small layers ride along with the finest one.  Same tile
// functions on the same data: bit-identical flow (tests/test_gpu_flow.py).
// (Measured for such groups and not kept: the finest layer's images and expansions on a side stream underneath the coarse chain --
// every event record / wait costs ~6 us on the compute stream and the overlapped kernels slow the chain's own: 0.320 vs 0.306 ms per
// 1280x720 pair, profiles/r03/c2_side_stream.txt; all sweeps of a layer in one launch of resident workgroups that hand M' over through
// flags -- a cross-CU hand-off costs what the kernel boundary costs: 0.419 vs 0.305 ms, profiles/r03/c2_resident_sweeps.txt.  For big
// groups overlapping the finest layer's preparation with the coarse sweeps loses too: profiles/r02/ab_overlap_fine_prep_with_coarse_sweeps.log.)
template <typename T>
static int flow_group(mav_ctx* c, const T* prev, const T* next, int g, bool seq, float* flow_out, const float* deep_flow = nullptr,
                      size_t deep_stride = 0, const float* flow_init = nullptr)
{
    mav_ctx::WorkSet& w = c->ws;
    const hipStream_t st = c->stream;
    const int L = (int)c->layers.size();
    const size_t n0 = c->n0, fc_stride = 2 * (c->n1 ? c->n1 : 1);
    auto flow_of = [&](int k) { return k ? w.fc[k & 1] : flow_out; };
    auto fstride_of = [&](int k) { return k ? fc_stride : 2 * n0; };
    if (!deep_flow && is_small_group(c, g)) {
        const int F = seq ? g + 1 : 2 * g;                                // frames: one run of g + 1, or the prev run and the next run
        auto Ik = [&](int k) { return k ? w.Ic + (size_t)F * c->c_off[k] : w.I; };
        auto Rk = [&](int k) { return k ? w.Rc + 5 * (size_t)F * c->c_off[k] : w.R; };
        auto sk = [&](int k) { return k ? c->c_stride[k] : n0; };
        pyramid_multi(c, st, FrameRun<T>{prev, seq ? nullptr : next, g, n0, F, c->W, c->H}, 0, L - 1, Ik, Rk, sk);
        auto at = [&](int k) {
            const size_t rs = 5 * sk(k);
            return LayerIO{k, g, Rk(k), Rk(k) + (seq ? rs : rs * (size_t)g), rs, flow_of(k), fstride_of(k), 5 * n0};
        };
        return walk_layers(c, st, L - 1, 0, at, {w.Ma, w.Mb}, top_flow(c, flow_init));
    }
    auto at = [&](int k) {
        const float *r0 = nullptr, *r1 = nullptr;
        layer_expansions(c, st, k, prev, next, g, seq, w.I, w.R, &r0, &r1);
        return LayerIO{k, g, r0, r1, 5 * n0, flow_of(k), fstride_of(k), 5 * n0};
    };
    if (deep_flow) return walk_layers(c, st, c->kd - 1, 0, at, {w.Ma, w.Mb}, coarser_flow(c, c->kd, deep_flow, deep_stride));
    return walk_layers(c, st, L - 1, 0, at, {w.Ma, w.Mb}, top_flow(c, flow_init));
}

// does a call of `batch` pairs run its deep layers once for the whole call (deep_layers) instead of once per group?
static bool use_deep_batch(const mav_ctx* c, int batch) { return c->deep_batch && c->kd > 0 && batch > c->group; }

// OPTFLOW_USE_INITIAL_FLOW: init_snap for `pairs` pairs (grown on demand: the buffer it replaces may still be read by enqueued work).
static int ensure_init_snapshot(mav_ctx* c, int pairs)
{
    if (pairs <= c->init_cap) return MAV_OK;
    const Layer& l = c->layers.back();
    const size_t stride = ((size_t)2 * l.w * l.h + 63) & ~(size_t)63, bytes = sizeof(float) * stride * pairs;
    // the buffer it replaces may still be read on either stream; the new one first, so that a failed call leaves the context usable
    CHK(grow_buffer(c, &c->init_snap, nullptr, bytes, MEM_WORKSPACE, READ_ON_ALL, ALLOC_FIRST, "Farneback workspace: initial-flow snapshot"));
    c->init_cap = pairs; c->init_stride = stride;
    return MAV_OK;
}
// optflowgf.cpp at the top layer k = L - 1 with OPTFLOW_USE_INITIAL_FLOW: flow = resize(flow0, (w_k, h_k), INTER_AREA); flow *= scale_k,
// scale_k = pyr_scale^k as the repeated product -- for n pairs of flow0 (slot stride 2 W H) into init_snap.
static void snapshot_initial_flow(mav_ctx* c, const float* flow0, int n)
{
    const int top = (int)c->layers.size() - 1;
    const Layer& l = c->layers[top];
    double scale = 1;
    for (int i = 0; i < top; i++) scale *= c->fb.pyr_scale;
    ProfScope ps(c, K_MISC);
    launch_area_resize_flow(c->stream, flow0, 2 * c->n0, c->W, c->H, c->init_snap, c->init_stride, l.w, l.h, n, scale);
}

// flow_init == nullptr: every pair starts from zero (mav_farneback_dev).  Otherwise the top layer's initial M of pair i comes from
// flow_init[i] (mav_farneback_init_dev); every other layer as always.  The snapshot of a set of pairs is taken right before the first
// launch that reads it and after every launch that writes flow of an earlier set: flow_init may be flow.
template <typename T>
static int farneback_run(mav_ctx* c, const T* prev, const T* next, int batch, const float* flow_init, float* flow)
{
    CHK(ensure_workspace(c));
    // A frame SEQUENCE -- the caller's two batches are views of one run of batch + 1 consecutive frames, next = prev + one frame,
    // which is how a video goes through the reference's loop (src/farneback.py:76-80 with prevgray = the last call's frame) -- has
    // every inner frame in two pairs.  Each group then blurs and expands its g + 1 frames once instead of 2 g (same arithmetic per
    // frame: the flow is bit-identical to the two-batch form; tests/test_gpu_flow.py).  Option "share_frames" = 0 switches it off.
    const bool seq = c->share_frames && next == prev + c->n0;
    const bool deep = use_deep_batch(c, batch);
    if (deep) CHK(ensure_deep(c));
    const int chunk = deep ? c->deep_cap : batch;
    if (flow_init) {
        const int need = deep ? chunk : c->group;
        CHK(ensure_init_snapshot(c, need < batch ? need : batch));
    }
    for (int d0 = 0; d0 < batch; d0 += chunk) {
        const int D = batch - d0 < chunk ? batch - d0 : chunk;
        const size_t dstride = deep ? 2 * c->c_stride[c->kd] : 0;
        // (Measured and not kept: the deep chain on a stream of its own underneath the first group's top-layer images / expansions --
        // 592 vs 597 pairs/s at 3840x2160 / 5 layers / 16 pairs: the fork / join events cost more than the overlap hides.)
        if (deep) {
            if (flow_init) snapshot_initial_flow(c, flow_init + (size_t)d0 * 2 * c->n0, D);
            CHK(deep_layers(c, c->stream, prev + (size_t)d0 * c->n0, next + (size_t)d0 * c->n0, D, seq, flow_init ? c->init_snap : nullptr));
        }
        for (int g0 = d0; g0 < d0 + D; g0 += c->group) {
            const int g = d0 + D - g0 < c->group ? d0 + D - g0 : c->group;
            if (flow_init && !deep) snapshot_initial_flow(c, flow_init + (size_t)g0 * 2 * c->n0, g);
            CHK(flow_group(c, prev + (size_t)g0 * c->n0, next + (size_t)g0 * c->n0, g, seq, flow + (size_t)g0 * 2 * c->n0,
                           deep ? c->deep.f[c->kd & 1] + (size_t)(g0 - d0) * dstride : nullptr, dstride,
                           flow_init && !deep ? c->init_snap : nullptr));
            CHK(check_launch("farneback kernels"));
        }
    }
    c->last_flow = flow;
    c->last_render.batch = 0;        // the flow a previous detection call read may have been overwritten
    c->last_roc.batch = 0;
    c->gm.last.batch = 0;
    return MAV_OK;
}
// bytes per pixel of a MAV_DEPTH_* code; 0 for any other code
static int depth_esize(int depth)
{
    return depth == MAV_DEPTH_8U ? 1 : depth == MAV_DEPTH_16U ? 2 : depth == MAV_DEPTH_32F ? 4 : 0;
}
// f(tag) with a null pointer to the pixel type of a MAV_DEPTH_* code the caller has checked (depth_esize): the one depth dispatch
template <typename F>
static auto with_depth(int depth, F&& f)
{
    if (depth == MAV_DEPTH_16U) return f((const uint16_t*)nullptr);
    if (depth == MAV_DEPTH_32F) return f((const float*)nullptr);
    return f((const uint8_t*)nullptr);
}
// The three device-pointer entry points: fn = the name their messages start with; need_init: flow_init may not be NULL.
static int farneback_dev(mav_ctx* c, const char* fn, const void* prev, const void* next, int depth, int batch, const float* flow_init,
                         bool need_init, float* flow)
{
    if (!c || !prev || !next || !flow || (need_init && !flow_init)) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    if (!depth_esize(depth)) return fail(MAV_ERR_ARG, "%s: depth %d is none of MAV_DEPTH_8U / 16U / 32F", fn, depth);
    CHK(check_dev_call(c, batch, fn));
    if (flow_init) {
        const size_t n = (size_t)batch * 2 * c->n0;
        if (flow_init != flow && flow_init < flow + n && flow < flow_init + n)
            return fail(MAV_ERR_ARG, "%s: flow_init and flow overlap without being the same field", fn);
    }
    return with_depth(depth, [&](auto* px) { return farneback_run(c, (decltype(px))prev, (decltype(px))next, batch, flow_init, flow); });
}
extern "C" int mav_farneback_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, int batch, float* flow)
{
    return farneback_dev(c, "mav_farneback", prev, next, MAV_DEPTH_8U, batch, nullptr, false, flow);
}
extern "C" int mav_farneback_init_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, int batch, const float* flow_init, float* flow)
{
    return farneback_dev(c, "mav_farneback_init_dev", prev, next, MAV_DEPTH_8U, batch, flow_init, true, flow);
}
extern "C" int mav_farneback_ex_dev(mav_ctx* c, const void* prev, const void* next, int depth, int batch, const float* flow_init, float* flow)
{
    return farneback_dev(c, "mav_farneback_ex_dev", prev, next, depth, batch, flow_init, false, flow);
}
extern "C" const float* mav_last_flow_dev(const mav_ctx* c) { return c ? c->last_flow : nullptr; }

// The schedule a call of `batch` pairs takes with the options in effect, as one line of JSON (bench.py prints it and hashes it):
// every option of mav_set_option, the group split and, per layer, how its sweeps run.
static int schedule_info(mav_ctx* c, int batch, int esize, char* buf, size_t cap)
{
    if (!c || !buf || cap < 2) return fail(MAV_ERR_ARG, "mav_schedule_info: NULL argument");
    if (batch < 1 || batch > c->max_batch) return fail(MAV_ERR_ARG, "batch %d outside [1, %d]", batch, c->max_batch);
    std::string o = "{";
    char t[256];
    for (const Option& d : kOptions) {
        if (!d.in_schedule) continue;
        snprintf(t, sizeof(t), "\"%s\": %ld, ", d.name, option_value(c, d));
        o += t;
    }
    const int g = batch < c->group ? batch : c->group;
    const bool deep = use_deep_batch(c, batch);
    const int D = deep ? (batch < c->deep_cap ? batch : c->deep_cap) : 0;
    snprintf(t, sizeof(t), "\"pairs_per_group\": %d, \"pyramid_in_two_launches\": %s, \"deep_layers_from\": %d, \"deep_pairs\": %d, \"layers\": [", g,
             (!deep && is_small_group(c, g)) ? "true" : "false", deep ? c->kd : 0, D);
    o += t;
    for (int k = 0; k < (int)c->layers.size(); k++) {
        const Layer& l = c->layers[k];
        const SweepPlan p = plan_sweeps(c, k, (deep && k >= c->kd) ? D : g, l.w % 4 == 0 && c->fb.winsize / 2 == 6);
        snprintf(t, sizeof(t), "%s{\"layer\": %d, \"w\": %d, \"h\": %d, \"blur\": \"%s\", \"sweeps\": \"%s\", \"pairs_per_launch\": %d, \"bands\": %d}",
                 k ? ", " : "", k, l.w, l.h,
                 (l.w == c->W && l.h == c->H) ? "3x3" : (blur_resize_is_fused(c->W, c->H, l.w, l.h, l.ksize, esize) ? "fused" : "two-pass"),
                 p.name, p.per_launch, p.J);
        o += t;
    }
    o += c->window == MAV_WINDOW_GAUSSIAN ? "], \"window\": \"gaussian\"}" : "]}";
    if (o.size() + 1 > cap) return fail(MAV_ERR_ARG, "mav_schedule_info: buffer of %zu bytes too small (%zu needed)", cap, o.size() + 1);
    memcpy(buf, o.c_str(), o.size() + 1);
    return MAV_OK;
}
extern "C" int mav_schedule_info(mav_ctx* c, int batch, char* buf, size_t cap) { return schedule_info(c, batch, 1, buf, cap); }
extern "C" int mav_schedule_info_ex(mav_ctx* c, int batch, int depth, char* buf, size_t cap)
{
    if (!depth_esize(depth)) return fail(MAV_ERR_ARG, "mav_schedule_info_ex: depth %d is none of MAV_DEPTH_8U / 16U / 32F", depth);
    return schedule_info(c, batch, depth_esize(depth), buf, cap);
}

// ---- detection ---------------------------------------------------------------------------------------------
static int ensure_foe_scratch(mav_ctx* c, int N)
{
    if (N <= c->foe_sc_n) return MAV_OK;
    c->foe_sc_n = 0;
    CHK(grow_buffer(c, &c->foe_sc.cand, nullptr, sizeof(double) * 2 * (size_t)N * c->max_batch, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "FoE candidates"));
    c->foe_sc_n = N;
    return MAV_OK;
}
// The caller's FoE parameters (NULL: the defaults) judged, and the candidates' scratch there for them: what every call that estimates
// a FoE does once, before it enqueues anything.  A call refused here leaves the derotation block, the FoEs and the tickets that
// last_render / last_roc read as they were.
static int foe_checked(mav_ctx* c, const mav_foe_params* fp, mav_foe_params* f)
{
    CHK(foe_or_defaults(fp, f));
    return ensure_foe_scratch(c, f->n_pairs);
}

// Per-pair derotation constants.  Device pointers stay on the device (a tiny kernel packs them: no host round trip, the
// stream never drains); host pointers are packed here and copied.
static int upload_derot(mav_ctx* c, const double* omega, const double* dt, const uint8_t* frame0, int batch, bool host_ptrs,
                        const DerotParams** out, DerotParams* dst = nullptr /* c->derot_dev */)
{
    *out = nullptr;
    if (!omega && !frame0) return MAV_OK;
    if (!dst) dst = c->derot_dev;
    if (!host_ptrs) {
        launch_make_derot(c->stream, omega, dt, frame0, batch, c->W, c->H, dst);
        *out = dst;
        return MAV_OK;
    }
    std::vector<DerotParams> dp(batch);
    for (int b = 0; b < batch; b++) {
        const double d = dt ? dt[b] : 1.0;
        dp[b].o0 = omega ? omega[3 * b] : 0.0; dp[b].o1 = omega ? omega[3 * b + 1] : 0.0; dp[b].o2 = omega ? omega[3 * b + 2] : 0.0;
        dp[b].sx = c->W * d / 2;   // w * dt / 2   (detector.py:101)
        dp[b].sy = c->H * d / 2;
        dp[b].mode = (frame0 && frame0[b]) ? MAV_PAIR_FRAME0 : (omega ? MAV_PAIR_DEROTATE : MAV_PAIR_PROMOTE);
    }
    HIPCHK(hipMemcpyAsync(dst, dp.data(), sizeof(DerotParams) * batch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // dp is a local vector
    *out = dst;
    return MAV_OK;
}

// What one detection call reads and writes, all device pointers; whatever stays NULL is not there / not wanted.
struct DetectArgs {
    const float* flow32 = nullptr;           // the flow field: this one (float32 arithmetic for frame-0 pairs, derot says which) ...
    const double* flow64 = nullptr;          // ... or this one
    const DerotParams* derot = nullptr;
    const uint8_t* sky = nullptr;
    const uint32_t* samples = nullptr;       // given: the FoE is estimated from them with foe_par (NULL: the defaults) and goes to foe_out
    const mav_foe_params* foe_par = nullptr; // (what foe_checked filled in: detect_dev judges nothing); not given: the phi / mask stage reads
    const double* foe_in = nullptr;          // foe_in
    double* foe_out = nullptr;               // (NULL: the context's own buffer)
    const mav_thr_params* thr = nullptr;     // given: the phi / mask stage runs even if none of its outputs below is wanted
    double* phi = nullptr;
    uint8_t *mask_fixed = nullptr, *mask_dyn = nullptr;
    unsigned long long* max_phi_bits = nullptr;
    mav_result* results = nullptr;
    int32_t* box_out = nullptr;
    void set_flow(const float* f) { flow32 = f; }
    void set_flow(const double* f) { flow64 = f; }
};
static int detect_dev(mav_ctx* c, int batch, const DetectArgs& a)
{
    const int W = c->W, H = c->H;
    const double* foe = a.foe_in;
    const bool want_phi = a.thr || a.phi || a.mask_fixed || a.mask_dyn || a.results || a.box_out || a.max_phi_bits;
    if (a.samples) {
        const mav_foe_params& f = *a.foe_par;
        double* fo = a.foe_out ? a.foe_out : c->foe_dev;
        ProfScope ps(c, K_FOE);
        // the candidates kernel also initialises the pair's box accumulators and tickets, the vote's last workgroup writes the FoE:
        // two launches where round 2 had four (candidates, vote, FoE finalize, box init)
        int32_t* init_box = want_phi ? c->box_acc : nullptr;
        if (a.flow32)
            launch_foe_f32(c->stream, a.flow32, a.derot, a.samples, batch, W, H, f.n_pairs, sq_threshold(f.mag_threshold),
                           sq_threshold_f32(f.mag_threshold), sq_threshold(f.ransac_threshold), c->foe_sc, fo, init_box, a.max_phi_bits);
        else
            launch_foe_f64(c->stream, a.flow64, a.samples, batch, W, H, f.n_pairs, sq_threshold(f.mag_threshold),
                           sq_threshold(f.ransac_threshold), c->foe_sc, fo, init_box, a.max_phi_bits);
        foe = fo;
    }
    if (want_phi) {
        if (!foe) return fail(MAV_ERR_ARG, "phi/mask stage needs a FoE (samples or foe)");
        const mav_thr_params t = thr_or_defaults(a.thr);
        if (!a.samples) { ProfScope ps(c, K_MISC); launch_box_init(c->stream, c->box_acc, a.max_phi_bits, c->foe_sc.done, batch); }
        // the pair's record (box, FoE) is written by the phi kernel's last workgroup of the pair: no finalize launch
        PhiLaunch pl;
        pl.done = c->foe_sc.done; pl.results = a.results; pl.box_out = a.box_out; pl.screen = c->phi_screen; pl.yloop = c->phi_yloop;
        ProfScope ps(c, K_PHI);
        if (a.flow32)
            launch_phi_mask_f32(c->stream, a.flow32, a.derot, foe, a.sky, batch, W, H, t, a.phi, a.mask_fixed, a.mask_dyn, c->box_acc,
                                a.max_phi_bits, pl);
        else
            launch_phi_mask_f64(c->stream, a.flow64, foe, a.sky, batch, W, H, t, a.phi, a.mask_fixed, a.mask_dyn, c->box_acc, a.max_phi_bits, pl);
    }
    return check_launch("detection kernels");
}

// mav_detect_dev behind its checks (f: from foe_checked): the derotation block, the detection, the records of the readers
static int detect_checked(mav_ctx* c, const float* flow, const uint32_t* samples, const double* omega, const double* dt,
                          const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params& f,
                          const mav_thr_params* tp, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results)
{
    const mav_thr_params t = thr_or_defaults(tp);
    DetectArgs a;
    a.flow32 = flow; a.samples = samples; a.sky = sky; a.foe_par = &f; a.thr = &t;
    a.phi = phi; a.mask_fixed = mask_fixed; a.mask_dyn = mask_dyn; a.results = results;
    CHK(upload_derot(c, omega, dt, frame0, batch, false, &a.derot));
    CHK(detect_dev(c, batch, a));
    // what mav_last_render reads: the FoE went to the context's own buffer (detect_dev without foe_out)
    c->last_render.flow = flow; c->last_render.derot = a.derot; c->last_render.foe = c->foe_dev; c->last_render.sky = sky;
    c->last_render.thr = t; c->last_render.batch = batch; c->last_render.mask_fixed = mask_fixed;
    c->last_roc = mav_ctx::LastRoc{flow, false, a.derot, c->foe_dev, sky, batch};
    return MAV_OK;
}
extern "C" int mav_detect_dev(mav_ctx* c, const float* flow, const uint32_t* samples, const double* omega, const double* dt,
                              const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params* fp,
                              const mav_thr_params* tp, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results)
{
    if (!c || !flow || !samples || !results) return fail(MAV_ERR_ARG, "mav_detect_dev: NULL argument");
    CHK(check_dev_call(c, batch, "mav_detect_dev"));
    mav_foe_params f;
    CHK(foe_checked(c, fp, &f));                 // every argument is judged before anything is enqueued
    return detect_checked(c, flow, samples, omega, dt, frame0, sky, batch, f, tp, phi, mask_fixed, mask_dyn, results);
}

extern "C" int mav_process_batch_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const uint32_t* samples,
                                     const double* omega, const double* dt, const uint8_t* frame0, const uint8_t* sky, int batch,
                                     const mav_foe_params* fp, const mav_thr_params* tp, float* flow, double* phi,
                                     uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results)
{
    if (!c || !prev || !next || !samples || !results) return fail(MAV_ERR_ARG, "mav_process_batch: NULL argument");
    CHK(check_dev_call(c, batch, "mav_process_batch_dev"));
    mav_foe_params f;
    CHK(foe_checked(c, fp, &f));                 // (before the flow is enqueued: a refused call changes nothing)
    if (!flow) {
        CHK(ensure_flow_ws(c));
        flow = c->flow_ws;
    }
    CHK(mav_farneback_dev(c, prev, next, batch, flow));
    return detect_checked(c, flow, samples, omega, dt, frame0, sky, batch, f, tp, phi, mask_fixed, mask_dyn, results);
}

// ---- connected components (include/mavflow.h: mav_components) -----------------------------------------------------------------------
extern "C" void mav_cc_defaults(mav_cc_params* p)
{
    if (p) { p->connectivity = 8; p->min_area = 1; p->max_blobs = 256; }
}
// The caller's parameters (NULL = defaults), refused before anything is enqueued.
static int cc_params_checked(const mav_cc_params* pp, mav_cc_params* p, const char* fn)
{
    if (pp) *p = *pp; else mav_cc_defaults(p);
    if (p->connectivity != 4 && p->connectivity != 8) return fail(MAV_ERR_ARG, "%s: connectivity must be 4 or 8, got %d", fn, p->connectivity);
    if (p->min_area < 1) return fail(MAV_ERR_ARG, "%s: min_area must be at least 1, got %d", fn, p->min_area);
    if (p->max_blobs < 1 || p->max_blobs > MAV_CC_MAX_BLOBS) return fail(MAV_ERR_ARG, "%s: max_blobs %d outside [1, %d]", fn, p->max_blobs, (int)MAV_CC_MAX_BLOBS);
    return MAV_OK;
}
// Device pointers, checked parameters: the tables zeroed, then the passes over sub-batches of as many images as the workspace cap holds
// (at least one).  The workspace grows to that size once and is never sized by max_batch.
static int components_enqueue(mav_ctx* c, const uint8_t* mask, int batch, const mav_cc_params& p, int32_t* labels, mav_cc_counts* counts,
                              mav_blob* blobs)
{
    const size_t per = cc_workspace_per_image(c->W, c->H);
    size_t sub = ((size_t)c->cc_workspace_mb << 20) / per;
    sub = sub < 1 ? 1 : sub > (size_t)batch ? (size_t)batch : sub;
    CHK(grow_buffer(c, &c->cc_ws, &c->cc_ws_cap, per * sub, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "components workspace"));
    HIPCHK(hipMemsetAsync(blobs, 0, sizeof(mav_blob) * (size_t)p.max_blobs * batch, c->stream));
    ProfScope ps(c, K_COMPONENTS);
    for (size_t b0 = 0; b0 < (size_t)batch; b0 += sub) {
        const int g = (int)((size_t)batch - b0 < sub ? (size_t)batch - b0 : sub);
        launch_components(c->stream, CcArgs{mask + b0 * c->n0, g, c->W, c->H, p.connectivity, p.min_area, p.max_blobs, c->cc_ws,
                                            labels ? labels + b0 * c->n0 : nullptr, counts + b0, blobs + b0 * (size_t)p.max_blobs});
    }
    return check_launch("components");
}
extern "C" int mav_components_dev(mav_ctx* c, const uint8_t* mask, int batch, const mav_cc_params* pp, int32_t* labels, mav_cc_counts* counts,
                                  mav_blob* blobs)
{
    if (!c || !mask || !counts || !blobs) return fail(MAV_ERR_ARG, "mav_components_dev: NULL argument");
    mav_cc_params p;
    CHK(cc_params_checked(pp, &p, "mav_components_dev"));
    CHK(check_dev_call(c, batch, "mav_components_dev"));
    return components_enqueue(c, mask, batch, p, labels, counts, blobs);
}

// ---- threshold sweep (include/mavflow.h: mav_roc_sweep) ---------------------------------------------------------------------------
// The caller's lists, refused before anything is enqueued or written: each 1 .. max entries, finite, >= 0, strictly increasing.
static int roc_list_checked(const double* v, int n, int max, const char* what, const char* fn)
{
    if (n < 1 || n > max) return fail(MAV_ERR_ARG, "%s: %d %s outside [1, %d]", fn, n, what, max);
    if (!v) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, what);
    for (int i = 0; i < n; i++) {
        if (!(v[i] >= 0.0) || !std::isfinite(v[i])) return fail(MAV_ERR_ARG, "%s: %s[%d] = %g is not a finite value >= 0", fn, what, i, v[i]);
        if (i && !(v[i] > v[i - 1])) return fail(MAV_ERR_ARG, "%s: %s must be strictly increasing (entry %d)", fn, what, i);
    }
    return MAV_OK;
}
// Every entry point calls this BEFORE it looks at the context, so that a refused list is refused whatever the context is: the order is
// load-bearing for tests/test_abi_roc.py, which passes refused lists with a handle that must never be dereferenced.
static int roc_params_checked(const mav_roc_params* p, RocThr* t, const char* fn)
{
    if (!p) return fail(MAV_ERR_ARG, "%s: NULL parameters", fn);
    CHK(roc_list_checked(p->angles, p->n_angles, MAV_ROC_MAX_ANGLES, "angles", fn));
    CHK(roc_list_checked(p->mags, p->n_mags, MAV_ROC_MAX_MAGS, "mags", fn));
    *t = RocThr{};
    t->ka = p->n_angles; t->km = p->n_mags;
    for (int i = 0; i < t->ka; i++) { t->ang[i] = p->angles[i]; t->ang32[i] = (float)p->angles[i]; }
    for (int j = 0; j < t->km; j++) { t->mag[j] = p->mags[j]; t->mag32[j] = (float)p->mags[j]; }
    // a lower bound of mag[0]^2: the product is within half an ulp of it, so one step towards zero is below or on it
    const double sq = t->mag[0] * t->mag[0];
    t->mag0_sq_lo = std::isfinite(sq) ? nextafter(sq, 0.0) : 0.0;
    return MAV_OK;
}
// Device pointers, checked lists.  Of the thresholds nothing is read: the lists replace the fixed mask's two, the dynamic ones are ignored.
static int roc_enqueue(mav_ctx* c, const void* flow, bool f64, const DerotParams* derot, const double* foe, const uint8_t* sky, const uint8_t* gt,
                       int gt_images, int batch, const RocThr& t, int64_t* table)
{
    const size_t stride = gt_images == 1 && batch > 1 ? 0 : c->n0;
    ProfScope ps(c, K_MISC);
    HIPCHK(launch_roc_sweep(c->stream, flow, f64, derot, foe, sky, gt, stride, batch, c->W, c->H, t, (unsigned long long*)table));
    return check_launch("roc sweep");
}

// ---- one iteration of the reference's loop as one call (include/mavflow.h: mav_frame_step) ---------------------------------------
static int frame_step_body(mav_ctx* c, const mav_frame_step* s, bool* started);
static int frame_step_enqueue(mav_ctx* c, const mav_frame_step* s)
{
    bool started = false;
    const int rc = frame_step_body(c, s, &started);
    if (rc != MAV_OK && started) {
        // the step failed part-way (a refused argument inside the detection, say) after some of it had been enqueued: its gathers may
        // still be reading host sources the caller holds (MAV_GATHER_SOURCES_HELD).  Every marker of the step is recorded behind
        // what was enqueued, so that whoever waits for them before giving those sources back still waits for the transfers.
        const std::string err = g_err;
        (void)mav_upload_fence(c);
        for (int i = 0; i < s->n_record_after_flow; i++)
            if (s->record_after_flow[i]) (void)hipEventRecord((hipEvent_t)s->record_after_flow[i], c->stream);
        if (s->record_done) (void)hipEventRecord((hipEvent_t)s->record_done, c->stream);
        (void)hipGetLastError();
        g_err = err;
    }
    return rc;
}
static int frame_step_body(mav_ctx* c, const mav_frame_step* s, bool* started)
{
    if (s->n < 1 || s->n > c->max_batch) return fail(MAV_ERR_ARG, "mav_frame_step: n %d outside [1, %d]", s->n, c->max_batch);
    if (s->n_gather < 0 || s->n_gather > MAV_STEP_MAX_GATHER) return fail(MAV_ERR_ARG, "mav_frame_step: n_gather %d outside [0, %d]", s->n_gather, (int)MAV_STEP_MAX_GATHER);
    if (s->n_wait_before < 0 || s->n_record_after_flow < 0 || (s->n_wait_before && !s->wait_before) || (s->n_record_after_flow && !s->record_after_flow))
        return fail(MAV_ERR_ARG, "mav_frame_step: marker list without markers");
    if (s->compute_flow && (!s->prev_dev || !s->next_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: compute_flow needs prev_dev and next_dev");
    if (s->detect && ((!s->flow_dev && !s->compute_flow) || !s->par_dev || !s->out_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: detect needs a flow, par_dev and out_dev");
    if (s->detect && s->gt_dev && (!s->mask_fixed_dev || !s->mask_dyn_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: the counts need both masks");
    if (s->n_bgr && (!s->bgr_dev || !s->gray_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: n_bgr without bgr_dev / gray_dev");
    if (s->out_bytes && (!s->out_host || !s->out_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: out_bytes without out_host / out_dev");
    if (s->par_bytes && (!s->par_host || !s->par_dev)) return fail(MAV_ERR_ARG, "mav_frame_step: par_bytes without par_host / par_dev");
    mav_cc_params cc{};
    if (s->cc.max_blobs) {
        if (!s->detect || !s->mask_fixed_dev || !s->out_dev) return fail(MAV_ERR_ARG, "mav_frame_step: cc needs detect, mask_fixed_dev and out_dev");
        if (s->off_cc_counts % alignof(mav_cc_counts) || s->off_cc_blobs % alignof(mav_blob))
            return fail(MAV_ERR_ARG, "mav_frame_step: off_cc_counts must be a multiple of 4 and off_cc_blobs of 8");
        CHK(cc_params_checked(&s->cc, &cc, "mav_frame_step"));
    }
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < s->n_wait_before; i++)
        if (s->wait_before[i]) HIPCHK(hipEventSynchronize((hipEvent_t)s->wait_before[i]));
    *started = true;                             // from here on a failure may leave work of this step enqueued
    const bool roc = c->roc_armed && s->detect && s->gt_dev;
    const size_t roc_bytes = roc ? sizeof(int64_t) * MAV_ROC_TABLE_WORDS(c->roc_thr.ka, c->roc_thr.km) * (size_t)s->n : 0;
    if (roc && s->out_host && s->out_bytes < c->roc_off + roc_bytes)      // refused like any parameter; the step's markers still fire
        return fail(MAV_ERR_ARG, "mav_frame_step: out_bytes %zu does not hold the armed sweep's tables (%zu bytes at offset %zu)", s->out_bytes,
                    roc_bytes, c->roc_off);
    if (s->par_bytes) {
        CHK(mav_upload_async_unordered(c, s->par_dev, s->par_host, s->par_bytes));
    }
    for (int i = 0; i < s->n_gather; i++)
        CHK(mav_upload_gather(c, s->gather[i].dst_dev, s->gather[i].src_host, s->gather[i].count, s->gather[i].bytes_each, MAV_GATHER_SOURCES_HELD));
    CHK(mav_upload_fence(c));
    if (s->n_bgr) CHK(mav_bgr2gray_dev(c, s->bgr_dev, s->n_bgr, s->gray_dev));
    float* flow = s->flow_dev;
    if (s->compute_flow) {
        if (!flow) {                             // nobody wants to see the flow: the context's own buffer, as mav_process_batch_dev
            CHK(ensure_flow_ws(c));
            flow = c->flow_ws;
        }
        CHK(mav_farneback_dev(c, s->prev_dev, s->next_dev, s->n, flow));
    }
    for (int i = 0; i < s->n_record_after_flow; i++)
        if (s->record_after_flow[i]) HIPCHK(hipEventRecord((hipEvent_t)s->record_after_flow[i], c->stream));
    if (s->detect) {
        const char* par = (const char*)s->par_dev;
        CHK(mav_detect_dev(c, flow, (const uint32_t*)(par + s->off_samples), s->has_omega ? (const double*)(par + s->off_omega) : nullptr,
                           s->has_omega ? (const double*)(par + s->off_dt) : nullptr, s->has_frame0 ? (const uint8_t*)(par + s->off_frame0) : nullptr,
                           s->sky_dev, s->n, &s->foe, &s->thr, nullptr, s->mask_fixed_dev, s->mask_dyn_dev, (mav_result*)s->out_dev));
        if (s->gt_dev)
            CHK(mav_tpr_fpr_counts_dev(c, s->gt_dev, s->gt_images, s->mask_fixed_dev, s->mask_dyn_dev, 255, s->n,
                                       (int64_t*)((char*)s->out_dev + s->off_counts_fixed), (int64_t*)((char*)s->out_dev + s->off_counts_dyn)));
        if (cc.max_blobs)
            CHK(components_enqueue(c, s->mask_fixed_dev, s->n, cc, nullptr, (mav_cc_counts*)((char*)s->out_dev + s->off_cc_counts),
                                   (mav_blob*)((char*)s->out_dev + s->off_cc_blobs)));
        if (roc) {                               // on what the detection above read: its flow, derotation block, FoE, sky and thresholds
            const mav_ctx::LastRender& r = c->last_render;
            CHK(roc_enqueue(c, r.flow, false, r.derot, r.foe, r.sky, s->gt_dev, s->gt_images, s->n, c->roc_thr, (int64_t*)((char*)s->out_dev + c->roc_off)));
        }
    }
    if (s->out_bytes) CHK(mav_download_async(c, s->out_host, s->out_dev, s->out_bytes));
    if (s->record_done) HIPCHK(hipEventRecord((hipEvent_t)s->record_done, c->stream));
    return MAV_OK;
}

extern "C" int mav_frame_step_dev(mav_ctx* c, const mav_frame_step* s)
{
    if (!c || !s) return fail(MAV_ERR_ARG, "mav_frame_step_dev: NULL argument");
    CHK(mav_worker_drain(c));
    return frame_step_enqueue(c, s);
}

// The worker: one thread per context that has been posted to.  A context is single-threaded; while steps are posted the worker IS
// that thread (the poster touches nothing of the context but this queue).  Three lanes = three workers enqueueing side by side
// while the loop's own thread draws samples and fills in FrameResults.
struct StepJob {
    mav_frame_step s;
    std::vector<const void*> src[MAV_STEP_MAX_GATHER];
    std::vector<void*> wait_before, record_after;
    uint64_t ticket = 0;
};
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    std::deque<StepJob> q;
    uint64_t posted = 0, done = 0;
    bool stop = false;
    // failures by ticket, until mav_frame_step_wait delivers them.  mav_worker_drain reports the earliest one after `drained` (the
    // last ticket a drain has covered): a failure is reported once by a drain, and never by a drain once its own ticket has told it
    std::map<uint64_t, std::pair<int, std::string>> failed;
    uint64_t drained = 0;
};
static void worker_main(mav_ctx* c)
{
    Worker* w = c->worker;
    (void)hipSetDevice(c->device);
    std::unique_lock<std::mutex> lk(w->m);
    for (;;) {
        w->cv_job.wait(lk, [&] { return w->stop || !w->q.empty(); });
        if (w->stop) {
            // mav_destroy: steps nobody waited for are DROPPED, not enqueued -- the host buffers they point to may be gone with
            // whoever posted them; their tickets report MAV_ERR_STATE to a waiter that is still there
            for (StepJob& j : w->q) w->failed[j.ticket] = {MAV_ERR_STATE, "the context was destroyed before this step was enqueued"};
            if (!w->q.empty()) w->done = w->q.back().ticket;
            w->q.clear();
            w->cv_done.notify_all();
            return;
        }
        StepJob job = std::move(w->q.front());
        w->q.pop_front();
        lk.unlock();
        const int rc = frame_step_enqueue(c, &job.s);
        lk.lock();
        if (rc != MAV_OK) w->failed[job.ticket] = {rc, g_err};
        w->done = job.ticket;
        w->cv_done.notify_all();
    }
}
static void stop_worker(mav_ctx* c)
{
    if (!c->worker) return;
    { std::lock_guard<std::mutex> lk(c->worker->m); c->worker->stop = true; }
    c->worker->cv_job.notify_all();
    c->worker->th.join();
    delete c->worker;
    c->worker = nullptr;
}
extern "C" int mav_frame_step_post(mav_ctx* c, const mav_frame_step* s, uint64_t* ticket)
{
    if (!c || !s || !ticket) return fail(MAV_ERR_ARG, "mav_frame_step_post: NULL argument");
    if (s->n_gather < 0 || s->n_gather > MAV_STEP_MAX_GATHER || s->n_wait_before < 0 || s->n_record_after_flow < 0)
        return fail(MAV_ERR_ARG, "mav_frame_step_post: list length out of range");
    if (!c->worker) {
        c->worker = new Worker();
        c->worker->th = std::thread(worker_main, c);
    }
    Worker* w = c->worker;
    StepJob job;
    job.s = *s;
    for (int i = 0; i < s->n_gather; i++) {
        if (s->gather[i].count < 1 || !s->gather[i].src_host) return fail(MAV_ERR_ARG, "mav_frame_step_post: gather list %d is empty", i);
        job.src[i].assign(s->gather[i].src_host, s->gather[i].src_host + s->gather[i].count);
        job.s.gather[i].src_host = job.src[i].data();          // (heap blocks: they keep their address when the job moves)
    }
    if (s->n_wait_before) { job.wait_before.assign(s->wait_before, s->wait_before + s->n_wait_before); job.s.wait_before = job.wait_before.data(); }
    if (s->n_record_after_flow) {
        job.record_after.assign(s->record_after_flow, s->record_after_flow + s->n_record_after_flow);
        job.s.record_after_flow = job.record_after.data();
    }
    {
        std::lock_guard<std::mutex> lk(w->m);
        job.ticket = *ticket = ++w->posted;
        w->q.push_back(std::move(job));
    }
    w->cv_job.notify_one();
    return MAV_OK;
}
extern "C" int mav_frame_step_wait(mav_ctx* c, uint64_t ticket, void* marker)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_frame_step_wait: NULL context");
    Worker* w = c->worker;
    if (!w || ticket == 0) return fail(MAV_ERR_ARG, "mav_frame_step_wait: no such ticket");
    {
        std::unique_lock<std::mutex> lk(w->m);
        if (ticket > w->posted) return fail(MAV_ERR_ARG, "mav_frame_step_wait: ticket %llu was never posted", (unsigned long long)ticket);
        w->cv_done.wait(lk, [&] { return w->done >= ticket; });
        auto it = w->failed.find(ticket);
        if (it != w->failed.end()) {
            const int rc = it->second.first;
            const std::string err = it->second.second;
            w->failed.erase(it);
            lk.unlock();
            // a step that failed part-way recorded its marker behind what it had enqueued (frame_step_enqueue): that has finished too
            // when this returns; a step refused before it enqueued anything left the marker as it was
            if (marker) (void)hipEventSynchronize((hipEvent_t)marker);
            (void)hipGetLastError();
            g_err = err;
            return rc;
        }
    }
    if (marker) HIPCHK(hipEventSynchronize((hipEvent_t)marker));
    return MAV_OK;
}
extern "C" int mav_worker_wait_enqueued(mav_ctx* c, uint64_t ticket)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_worker_wait_enqueued: NULL context");
    Worker* w = c->worker;
    if (!w || ticket == 0) return MAV_OK;
    std::unique_lock<std::mutex> lk(w->m);
    if (ticket > w->posted) return fail(MAV_ERR_ARG, "mav_worker_wait_enqueued: ticket %llu was never posted", (unsigned long long)ticket);
    w->cv_done.wait(lk, [&] { return w->done >= ticket; });
    return MAV_OK;
}
extern "C" int mav_worker_drain(mav_ctx* c)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_worker_drain: NULL context");
    Worker* w = c->worker;
    if (!w) return MAV_OK;
    std::unique_lock<std::mutex> lk(w->m);
    w->cv_done.wait(lk, [&] { return w->done == w->posted; });
    auto it = w->failed.upper_bound(w->drained);
    w->drained = w->posted;
    if (it == w->failed.end()) return MAV_OK;
    g_err = it->second.second;
    return it->second.first;
}

// ---- host-pointer wrappers -----------------------------------------------------------------------------------
static int download(mav_ctx* c, void* dst, const void* src, size_t bytes)
{
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return MAV_OK;
}
// One host-pointer call: its staging blocks and uploads, and the downloads and the one synchronisation it ends in.
// A block is the context's next scratch block (grown when too small, never shrunk or freed before mav_destroy): once a call shape has
// been seen the staged path allocates nothing.  The host entry points are synchronous (finish() ends in mav_sync), so a block is idle
// again when the next call takes it.  Errors stick: after the first failure in() / out() / scratch() / fetch() do nothing and return
// NULL, and staged() / finish() return its code -- a call site asks once, before it launches.
struct HostCall {
    mav_ctx* const c;
    const char* const fn;            // the entry point, for messages
    int rc = MAV_OK;
    HostCall(mav_ctx* c_, const char* fn_) : c(c_), fn(fn_) {}
    HostCall(const HostCall&) = delete;
    ~HostCall() { if (appended) c->scratch_next = mark; }     // synchronous: an appending call's blocks are free again on return

    // Two ways to begin.  A fresh call (of `batch` pairs or images, where it has a batch) starts again at block 0 ...
    int fresh(int batch = 1)
    {
        if ((rc = check_dev_call(c, batch, fn)) != MAV_OK) return rc;
        c->scratch_next = 0;
        c->last_mf = c->last_md = nullptr; c->last_mask_batch = 0;     // ... and may overwrite the previous call's masks
        c->last_render.batch = 0;                                       // ... and its flow, FoE and sky
        c->last_roc.batch = 0;
        c->gm.last.batch = 0;                                           // ... and the flow and matrix of a global-motion call
        return MAV_OK;
    }
    int fresh_layer(int k, const Layer** l)      // ... a stage hook on layer k
    {
        if (!c) return rc = fail(MAV_ERR_ARG, "%s: NULL context", fn);
        if (k < 0 || k >= (int)c->layers.size()) return rc = fail(MAV_ERR_ARG, "%s: layer %d out of range", fn, k);
        *l = &c->layers[k];
        return fresh();
    }
    // A call that reads what the last call left resident takes the NEXT free blocks: the last call's blocks (its flow, sky and masks
    // among them) and the last_* state stay untouched, and the blocks go back when this object does, whichever way the call ends.
    int after_last()
    {
        if ((rc = check_dev_call(c, 1, fn)) != MAV_OK) return rc;
        mark = c->scratch_next;
        appended = true;
        return MAV_OK;
    }

    // A call that neither reads nor replaces anything resident (include/mavflow_truth.h), of `batch` pairs: the next free blocks as well,
    // given back in the same way.
    int beside(int batch)
    {
        if ((rc = check_dev_call(c, batch, fn)) != MAV_OK) return rc;
        mark = c->scratch_next;
        appended = true;
        return MAV_OK;
    }

    // Staging, each returning the device pointer.  A NULL host pointer takes no block, registers nothing and returns NULL.
    template <typename T> T* scratch(size_t bytes) { return (T*)block(bytes); }              // a block
    template <typename T> T* in(const T* host, size_t bytes)                                 // a block, filled from the host now
    {
        T* d = host ? (T*)block(bytes) : nullptr;
        if (d) rc = upload(d, host, bytes);
        return rc == MAV_OK ? d : nullptr;
    }
    template <typename T> T* out(T* host, size_t bytes)                                      // a block, brought to the host by finish()
    {
        T* d = host ? (T*)block(bytes) : nullptr;
        fetch(host, d, bytes);
        return d;
    }
    void fetch(void* host, const void* dev, size_t bytes)       // any device memory, brought to the host by finish()
    {
        if (rc != MAV_OK || !host) return;
        assert(n_down < MAX_DOWN);
        down[n_down++] = {host, dev, bytes};
    }
    int staged() const { return rc; }
    // the registered downloads, in the order they were registered, and the call's one synchronisation
    int finish()
    {
        CHK(rc);
        const int n = n_down;
        n_down = 0;
        for (int i = 0; i < n; i++) CHK(download(c, down[i].host, down[i].dev, down[i].bytes));
        return mav_sync(c);
    }

private:
    enum { MAX_DOWN = 6 };
    struct Down { void* host; const void* dev; size_t bytes; } down[MAX_DOWN];
    int n_down = 0;
    size_t mark = 0;
    bool appended = false;
    void* block(size_t bytes)
    {
        if (rc != MAV_OK) return nullptr;
        if (c->scratch_next == c->scratch.size()) c->scratch.emplace_back();
        mav_ctx::Block& b = c->scratch[c->scratch_next++];
        rc = grow_buffer(c, &b.p, &b.cap, bytes ? bytes : 1, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "staging block");
        return rc == MAV_OK ? b.p : nullptr;
    }
    int upload(void* dst, const void* src, size_t bytes)
    {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        return MAV_OK;
    }
};
// The two frame batches of a host-pointer call -> device.  When the caller's batches are views of one run of batch + 1 frames
// (next == prev + one frame) the run crosses PCIe once and keeps that layout on the device, which mav_farneback_dev recognises.
// esize: bytes per pixel (the frame run is recognised in bytes, whatever the depth).
static void upload_frames(HostCall& h, const void* prev, const void* next, int batch, int esize, const void** dprev, const void** dnext)
{
    const size_t fb = h.c->n0 * esize, n = fb * batch;
    if ((const char*)next == (const char*)prev + fb) {
        *dprev = h.in(prev, n + fb);
        h.scratch<void>(1);                               // keeps the staging slots of the two call forms aligned
        *dnext = (const char*)*dprev + fb;
        return;
    }
    *dprev = h.in(prev, n);
    *dnext = h.in(next, n);
}

// The three host-pointer entry points: frames (and the initial flow, if any) up, farneback_dev in place on the device, flow down.
static int farneback_host(mav_ctx* c, const char* fn, const void* prev, const void* next, int depth, int batch, const float* flow_init,
                          bool need_init, float* flow)
{
    if (c && !depth_esize(depth)) return fail(MAV_ERR_ARG, "%s: depth %d is none of MAV_DEPTH_8U / 16U / 32F", fn, depth);
    HostCall h(c, fn);
    CHK(h.fresh(batch));
    if (!prev || !next || !flow || (need_init && !flow_init)) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    const size_t bytes = c->n0 * batch * 2 * sizeof(float);
    const void *dprev, *dnext;
    upload_frames(h, prev, next, batch, depth_esize(depth), &dprev, &dnext);
    float* df = flow_init ? h.in(flow_init, bytes) : h.scratch<float>(bytes);
    h.fetch(flow, df, bytes);
    CHK(h.staged());
    CHK(farneback_dev(c, fn, dprev, dnext, depth, batch, flow_init ? df : nullptr, false, df));
    return h.finish();
}
extern "C" int mav_farneback(mav_ctx* c, const uint8_t* prev, const uint8_t* next, int batch, float* flow)
{
    return farneback_host(c, "mav_farneback", prev, next, MAV_DEPTH_8U, batch, nullptr, false, flow);
}
extern "C" int mav_farneback_init(mav_ctx* c, const uint8_t* prev, const uint8_t* next, int batch, const float* flow_init, float* flow)
{
    return farneback_host(c, "mav_farneback_init", prev, next, MAV_DEPTH_8U, batch, flow_init, true, flow);
}
extern "C" int mav_farneback_ex(mav_ctx* c, const void* prev, const void* next, int depth, int batch, const float* flow_init, float* flow)
{
    return farneback_host(c, "mav_farneback_ex", prev, next, depth, batch, flow_init, false, flow);
}
extern "C" int mav_derotate(mav_ctx* c, const float* flow, const double* omega, const double* dt, int batch, double* flow_out)
{
    HostCall h(c, "mav_derotate");
    CHK(h.fresh(batch));
    if (!flow || !omega || !flow_out) return fail(MAV_ERR_ARG, "mav_derotate: NULL argument");
    const size_t n = c->n0 * batch * 2;
    const float* df = h.in(flow, n * sizeof(float));
    double* dout = h.out(flow_out, n * sizeof(double));
    CHK(h.staged());
    const DerotParams* derot = nullptr;
    CHK(upload_derot(c, omega, dt, nullptr, batch, true, &derot));
    launch_derotate(c->stream, df, derot, batch, c->W, c->H, dout);
    CHK(check_launch("derotate"));
    return h.finish();
}

// ---- FoE and phi / masks of a flow array: float64 (a derotated field), or float32 (the reference's frame index 0: float32 arithmetic) --
static int frame0_params(mav_ctx* c, int batch, const DerotParams** out)
{
    std::vector<uint8_t> all(batch, 1);
    return upload_derot(c, nullptr, nullptr, all.data(), batch, true, out);
}

template <typename T>                // double: mav_foe_dense; float: mav_foe_dense_f32
static int foe_dense_host(mav_ctx* c, const char* fn, const T* flow, const uint32_t* samples, int batch, const mav_foe_params* fp, double* foe)
{
    HostCall h(c, fn);
    CHK(h.fresh(batch));
    if (!flow || !samples || !foe) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    mav_foe_params f;
    CHK(foe_checked(c, fp, &f));
    DetectArgs a;
    a.set_flow(h.in(flow, c->n0 * batch * 2 * sizeof(T)));
    a.samples = h.in(samples, sizeof(uint32_t) * 4 * (size_t)f.n_pairs * batch);
    a.foe_out = h.out(foe, sizeof(double) * 2 * batch);
    a.foe_par = &f;
    CHK(h.staged());
    if constexpr (sizeof(T) == sizeof(float)) CHK(frame0_params(c, batch, &a.derot));
    CHK(detect_dev(c, batch, a));
    return h.finish();
}
extern "C" int mav_foe_dense(mav_ctx* c, const double* flow, const uint32_t* samples, int batch, const mav_foe_params* fp, double* foe)
{
    return foe_dense_host(c, "mav_foe_dense", flow, samples, batch, fp, foe);
}
extern "C" int mav_foe_dense_f32(mav_ctx* c, const float* flow, const uint32_t* samples, int batch, const mav_foe_params* fp, double* foe)
{
    return foe_dense_host(c, "mav_foe_dense_f32", flow, samples, batch, fp, foe);
}

// T = double: mav_phi_mask.  T = float: mav_phi_mask_f32 -- the kernel stores the float32 angles widened to double (one phi layout
// for both arithmetic types), so they come down as doubles and are narrowed back, exactly, once the call has finished.
template <typename T>
static int phi_mask_host(mav_ctx* c, const char* fn, const T* flow, const double* foe, const uint8_t* sky, int batch, const mav_thr_params* tp,
                         T* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, T* max_phi)
{
    constexpr bool f32 = sizeof(T) == sizeof(float);
    HostCall h(c, fn);
    CHK(h.fresh(batch));
    if (!flow || !foe) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    const size_t n = c->n0 * batch;
    const mav_thr_params t = thr_or_defaults(tp);
    std::vector<double> wide(f32 && phi ? n : 0), mx(f32 && max_phi ? batch : 0);
    double* const hphi = !f32 ? (double*)phi : phi ? wide.data() : nullptr;          // where the doubles land on the host
    double* const hmax = !f32 ? (double*)max_phi : max_phi ? mx.data() : nullptr;
    DetectArgs a;
    a.set_flow(h.in(flow, n * 2 * sizeof(T)));
    a.foe_in = h.in(foe, sizeof(double) * 2 * batch);
    a.sky = h.in(sky, n);
    a.phi = h.out(hphi, n * sizeof(double));
    a.mask_fixed = h.out(mask_fixed, n);
    a.mask_dyn = h.out(mask_dyn, n);
    a.max_phi_bits = max_phi ? c->u64_scratch : nullptr;
    h.fetch(hmax, c->u64_scratch, sizeof(double) * batch);       // same bits
    a.thr = &t;
    CHK(h.staged());
    if constexpr (f32) CHK(frame0_params(c, batch, &a.derot));
    CHK(detect_dev(c, batch, a));
    c->last_mf = a.mask_fixed; c->last_md = a.mask_dyn; c->last_mask_batch = batch;
    c->last_roc = mav_ctx::LastRoc{f32 ? (const void*)a.flow32 : (const void*)a.flow64, !f32, a.derot, a.foe_in, a.sky, batch};
    CHK(h.finish());
    if (f32 && phi) for (size_t i = 0; i < n; i++) phi[i] = (T)wide[i];
    if (f32 && max_phi) for (int b = 0; b < batch; b++) max_phi[b] = (T)mx[b];
    return MAV_OK;
}
extern "C" int mav_phi_mask(mav_ctx* c, const double* flow, const double* foe, const uint8_t* sky, int batch, const mav_thr_params* tp,
                            double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, double* max_phi)
{
    return phi_mask_host(c, "mav_phi_mask", flow, foe, sky, batch, tp, phi, mask_fixed, mask_dyn, max_phi);
}
extern "C" int mav_phi_mask_f32(mav_ctx* c, const float* flow, const double* foe, const uint8_t* sky, int batch,
                                const mav_thr_params* tp, float* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, float* max_phi)
{
    return phi_mask_host(c, "mav_phi_mask_f32", flow, foe, sky, batch, tp, phi, mask_fixed, mask_dyn, max_phi);
}

extern "C" int mav_bbox(mav_ctx* c, const uint8_t* img, int batch, int32_t* box)
{
    HostCall h(c, "mav_bbox");
    CHK(h.fresh(batch));
    if (!img || !box) return fail(MAV_ERR_ARG, "mav_bbox: NULL argument");
    const uint8_t* di = h.in(img, c->n0 * batch);
    int32_t* db = h.out(box, sizeof(int32_t) * 4 * batch);
    CHK(h.staged());
    launch_box_init(c->stream, c->box_acc, nullptr, nullptr, batch);
    launch_bbox_u8(c->stream, di, batch, c->W, c->H, c->i32_scratch, c->box_acc);
    launch_box_finalize(c->stream, c->box_acc, batch, db);
    CHK(check_launch("bbox"));
    return h.finish();
}

extern "C" int mav_bgr2gray(mav_ctx* c, const uint8_t* bgr, int batch, uint8_t* gray)
{
    HostCall h(c, "mav_bgr2gray");
    CHK(h.fresh(batch));
    if (!bgr || !gray) return fail(MAV_ERR_ARG, "mav_bgr2gray: NULL argument");
    const size_t n = c->n0 * batch;
    const uint8_t* di = h.in(bgr, 3 * n);
    uint8_t* dg = h.out(gray, n);
    CHK(h.staged());
    launch_bgr2gray(c->stream, di, n, dg);
    CHK(check_launch("bgr2gray"));
    return h.finish();
}

extern "C" int mav_bgr2gray_dev(mav_ctx* c, const uint8_t* bgr, int batch, uint8_t* gray)
{
    if (!c || !bgr || !gray) return fail(MAV_ERR_ARG, "mav_bgr2gray_dev: NULL argument");
    if (batch < 1) return fail(MAV_ERR_ARG, "mav_bgr2gray_dev: batch %d < 1", batch);
    HIPCHK(hipSetDevice(c->device));
    ProfScope ps(c, K_MISC);
    launch_bgr2gray(c->stream, bgr, c->n0 * (size_t)batch, gray);
    return check_launch("bgr2gray");
}

// ---- frame decode, host side: the un-filtering pass of a PNG image ------------------------------------------------------------------
// `raw` is the inflated IDAT stream of a non-interlaced image: per row one filter-type byte followed by `stride` bytes; bpp = bytes per
// complete pixel (1 for depths below 8).  Filters 0 - 4 of the PNG specification (None, Sub, Up, Average, Paeth), arithmetic modulo 256.
// Sub / Average / Paeth are recurrences along the row, Up / Average / Paeth along the column: inherently serial per image, a few
// milliseconds of plain C for a 1080p frame (a numpy formulation needs a Python-level loop per pixel for two of the five filters).
extern "C" int mav_png_unfilter(const uint8_t* raw, int rows, size_t stride, int bpp, uint8_t* out)
{
    if (!raw || !out || rows < 0 || bpp < 1 || bpp > 8) return fail(MAV_ERR_ARG, "mav_png_unfilter: bad argument");
    const uint8_t* prev = nullptr;
    for (int y = 0; y < rows; y++) {
        const uint8_t ft = raw[(size_t)y * (stride + 1)];
        const uint8_t* in = raw + (size_t)y * (stride + 1) + 1;
        uint8_t* o = out + (size_t)y * stride;
        const size_t b = (size_t)bpp;
        switch (ft) {
        case 0: memcpy(o, in, stride); break;
        case 1:
            for (size_t i = 0; i < stride; i++) o[i] = (uint8_t)(in[i] + (i >= b ? o[i - b] : 0));
            break;
        case 2:
            for (size_t i = 0; i < stride; i++) o[i] = (uint8_t)(in[i] + (prev ? prev[i] : 0));
            break;
        case 3:
            for (size_t i = 0; i < stride; i++) {
                const unsigned a = i >= b ? o[i - b] : 0, up = prev ? prev[i] : 0;
                o[i] = (uint8_t)(in[i] + ((a + up) >> 1));
            }
            break;
        case 4:
            for (size_t i = 0; i < stride; i++) {
                const int a = i >= b ? o[i - b] : 0, up = prev ? prev[i] : 0, ul = (prev && i >= b) ? prev[i - b] : 0;
                const int p = a + up - ul, pa = abs(p - a), pb = abs(p - up), pc = abs(p - ul);
                const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? up : ul);
                o[i] = (uint8_t)(in[i] + pred);
            }
            break;
        default: return fail(MAV_ERR_ARG, "mav_png_unfilter: row %d has filter type %d (valid: 0 - 4)", y, (int)ft);
        }
        prev = o;
    }
    return MAV_OK;
}

extern "C" int mav_ransac(mav_ctx* c, const double* estimates, int count, double ransac_threshold, double* foe)
{
    if (!c || !foe || (count > 0 && !estimates)) return fail(MAV_ERR_ARG, "mav_ransac: NULL argument");
    if (count < 0 || count > 4096) return fail(MAV_ERR_ARG, "mav_ransac: count %d outside [0, 4096]", count);
    HIPCHK(hipSetDevice(c->device));
    const int N = count > 0 ? count : 1;
    CHK(ensure_foe_scratch(c, N));
    if (count > 0) HIPCHK(hipMemcpyAsync(c->foe_sc.cand, estimates, sizeof(double) * 2 * count, hipMemcpyHostToDevice, c->stream));
    double* const vote = c->foe_dev + 2 * (size_t)c->max_batch;       // its own two doubles: the pairs' FoEs stay resident
    launch_ransac_only(c->stream, c->foe_sc, count, c->foe_sc_n, sq_threshold(ransac_threshold), vote);
    CHK(check_launch("ransac"));
    CHK(download(c, foe, vote, sizeof(double) * 2));
    return mav_sync(c);
}

extern "C" int mav_window_max(mav_ctx* c, const uint8_t* img, int batch, int64_t* out)
{
    HostCall h(c, "mav_window_max");
    CHK(h.fresh(batch));
    if (!img || !out) return fail(MAV_ERR_ARG, "mav_window_max: NULL argument");
    const uint8_t* di = h.in(img, c->n0 * batch);
    int64_t* dout = h.out(out, sizeof(int64_t) * 3 * batch);
    CHK(h.staged());
    launch_window_max(c->stream, di, batch, c->W, c->H, c->u64_scratch, dout);
    CHK(check_launch("window_max"));
    return h.finish();
}

// ---- window search: analyze_pyramid / optimize_window -----------------------------------------------------------
// Level sizes exactly as the reference derives them (im_helpers.py:28-33 + imutils.resize): w' = int(w / scale),
// r = w' / float(w), h' = int(h * r); stop when a side drops below 30.
static int pyr_plan(const mav_ctx* c, double scale, int batch_cap, PyrPlan* p)
{
    if (!(scale > 1.0)) return fail(MAV_ERR_ARG, "pyramid scale %g must be > 1", scale);
    int w = c->W, h = c->H;
    size_t off = 0;
    unsigned base = 0;
    p->n = 0;
    for (;;) {
        if (p->n == MAV_PYR_MAX) return fail(MAV_ERR_ARG, "pyramid scale %g gives more than %d levels", scale, MAV_PYR_MAX);
        const int n = p->n++;
        p->w[n] = w; p->h[n] = h; p->base[n] = base; p->off[n] = off;
        if (w >= 64 && h >= 64) base += (unsigned)(((w - 64) / 16 + 1) * ((h - 64) / 16 + 1));
        if (n > 0) off += ((size_t)w * h * batch_cap + 255) & ~(size_t)255;
        const int wn = (int)((double)w / scale);
        if (wn < 1) break;
        const double r = (double)wn / (double)w;
        const int hn = (int)((double)h * r);
        if (hn < 30 || wn < 30) break;
        // cv2.resize takes its integer-ratio "fast area" path when both ratios are whole numbers; only the general path is restated
        const double sx = 1.0 / ((double)wn / w), sy = 1.0 / ((double)hn / h);
        if (fabs(sx - (int)sx) < DBL_EPSILON && fabs(sy - (int)sy) < DBL_EPSILON)
            return fail(MAV_ERR_ARG, "pyramid level %d -> %d has an integer ratio (%dx%d -> %dx%d): OpenCV's fast-area path is not implemented",
                        n, n + 1, w, h, wn, hn);
        w = wn; h = hn;
    }
    p->base[p->n] = base;
    return MAV_OK;
}
static size_t pyr_bytes(const PyrPlan& p, int batch_cap)
{
    size_t total = 0;
    for (int l = 1; l < p.n; l++) total += ((size_t)p.w[l] * p.h[l] * batch_cap + 255) & ~(size_t)255;
    return total ? total : 256;
}
static int ensure_pyr_ws(mav_ctx* c, const PyrPlan& p)
{
    return grow_buffer(c, &c->pyr_ws, &c->pyr_ws_cap, pyr_bytes(p, c->max_batch), MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "pyramid workspace");
}
// levels 1 .. upto of `batch` images (device pointer img0) into the workspace
static void build_pyramid(mav_ctx* c, const PyrPlan& p, const uint8_t* img0, int batch, int upto)
{
    for (int l = 1; l <= upto && l < p.n; l++) {
        const uint8_t* src = l == 1 ? img0 : c->pyr_ws + p.off[l - 1];
        launch_area_resize(c->stream, src, (size_t)p.w[l - 1] * p.h[l - 1], p.w[l - 1], p.h[l - 1], c->pyr_ws + p.off[l],
                           (size_t)p.w[l] * p.h[l], p.w[l], p.h[l], batch);
    }
}

extern "C" int mav_pyramid_levels(const mav_ctx* c, double scale)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_pyramid_levels: NULL context");
    PyrPlan p;
    CHK(pyr_plan(c, scale, 1, &p));
    return p.n;
}
extern "C" int mav_pyramid_dims(const mav_ctx* c, double scale, int level, int* w, int* h)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_pyramid_dims: NULL context");
    PyrPlan p;
    CHK(pyr_plan(c, scale, 1, &p));
    if (level < 0 || level >= p.n) return fail(MAV_ERR_ARG, "pyramid level %d outside [0, %d)", level, p.n);
    if (w) *w = p.w[level];
    if (h) *h = p.h[level];
    return MAV_OK;
}

extern "C" int mav_analyze_pyramid(mav_ctx* c, const uint8_t* img, int batch, double scale, int64_t* out)
{
    HostCall h(c, "mav_analyze_pyramid");
    CHK(h.fresh(batch));
    if (!img || !out) return fail(MAV_ERR_ARG, "mav_analyze_pyramid: NULL argument");
    PyrPlan p;
    CHK(pyr_plan(c, scale, c->max_batch, &p));
    CHK(ensure_pyr_ws(c, p));
    const uint8_t* di = h.in(img, c->n0 * batch);
    int64_t* dout = h.out(out, sizeof(int64_t) * 6 * batch);
    CHK(h.staged());
    HIPCHK(hipMemsetAsync(c->u64_scratch, 0, sizeof(unsigned long long) * batch, c->stream));
    build_pyramid(c, p, di, batch, p.n - 1);
    for (int l = 0; l < p.n; l++)
        launch_level_scan(c->stream, l == 0 ? di : c->pyr_ws + p.off[l], (size_t)p.w[l] * p.h[l], batch, p.w[l], p.h[l], p.base[l],
                          c->u64_scratch);
    launch_pyramid_finalize(c->stream, c->u64_scratch, p, di, c->pyr_ws, batch, dout);
    CHK(check_launch("analyze_pyramid"));
    return h.finish();
}

extern "C" int mav_stage_pyramid_level(mav_ctx* c, const uint8_t* img, double scale, int level, uint8_t* out)
{
    HostCall h(c, "mav_stage_pyramid_level");
    CHK(h.fresh());
    if (!img || !out) return fail(MAV_ERR_ARG, "mav_stage_pyramid_level: NULL argument");
    PyrPlan p;
    CHK(pyr_plan(c, scale, c->max_batch, &p));
    if (level < 0 || level >= p.n) return fail(MAV_ERR_ARG, "pyramid level %d outside [0, %d)", level, p.n);
    CHK(ensure_pyr_ws(c, p));
    const uint8_t* di = h.in(img, c->n0);
    CHK(h.staged());
    build_pyramid(c, p, di, 1, level);
    CHK(check_launch("area_resize"));
    h.fetch(out, level == 0 ? di : c->pyr_ws + p.off[level], (size_t)p.w[level] * p.h[level]);
    return h.finish();
}

extern "C" int mav_optimize_window(mav_ctx* c, const uint8_t* img, int batch, const int32_t* window_in, int64_t* score,
                                   int32_t* window_out)
{
    HostCall h(c, "mav_optimize_window");
    CHK(h.fresh(batch));
    if (!img || !window_in || !score || !window_out) return fail(MAV_ERR_ARG, "mav_optimize_window: NULL argument");
    if (!c->sat) CHK(c->mem.alloc(&c->sat, sizeof(unsigned long long) * (size_t)(c->W + 1) * (c->H + 1) * c->max_batch, MEM_OTHER, "summed-area tables"));
    const uint8_t* di = h.in(img, c->n0 * batch);
    const int32_t* dw = h.in(window_in, sizeof(int32_t) * 4 * batch);
    int64_t* ds = h.out(score, sizeof(int64_t) * batch);
    int32_t* dwo = h.out(window_out, sizeof(int32_t) * 4 * batch);
    CHK(h.staged());
    launch_optimize_window(c->stream, di, batch, c->W, c->H, c->sat, dw, ds, dwo);
    CHK(check_launch("optimize_window"));
    return h.finish();
}

// ---- global-motion subtraction: get_transformation_matrix / flow_vec_subtract (include/mavflow.h) ------------------------------------
static int ensure_render(mav_ctx* c);
static int ensure_motion(mav_ctx* c)
{
    if (c->gm.H) return MAV_OK;
    const size_t B = (size_t)c->max_batch;
    return c->mem.alloc_set({{&c->gm.H, sizeof(double) * 9 * B}, {&c->gm.ok, sizeof(int) * B}, {&c->gm.pyr, sizeof(int64_t) * 6 * B},
                             {&c->gm.win, sizeof(int32_t) * 4 * B}, {&c->gm.opt_win, sizeof(int32_t) * 4 * B},
                             {&c->gm.opt_score, sizeof(int64_t) * B}, {&c->gm.key, sizeof(unsigned long long) * 2 * B}},
                            MEM_OTHER, "global-motion scratch");
}
// the pair buffers for n pairs per item
static int ensure_pairs(mav_ctx* c, int n)
{
    CHK(ensure_motion(c));
    if ((size_t)n <= c->gm.pairs_cap) return MAV_OK;
    c->gm.pairs_cap = 0;
    const size_t items = (size_t)n * c->max_batch;
    CHK(grow_buffer(c, &c->gm.src, nullptr, sizeof(double) * 2 * items, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "homography pairs"));
    CHK(grow_buffer(c, &c->gm.dst, nullptr, sizeof(double) * 2 * items, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "homography pairs"));
    CHK(grow_buffer(c, &c->gm.work, nullptr, sizeof(double) * homography_work_doubles(n) * c->max_batch, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST,
                    "homography workspace"));
    CHK(grow_buffer(c, &c->gm.coords, nullptr, sizeof(int32_t) * 2 * (size_t)n, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "sample coordinates"));
    c->gm.pairs_cap = (size_t)n;
    return MAV_OK;
}
static int check_pairs(const char* fn, int n)
{
    if (n < 4 || n > MAV_HOMOGRAPHY_MAX_PAIRS) return fail(MAV_ERR_ARG, "%s: %d pairs outside [4, %d]", fn, n, MAV_HOMOGRAPHY_MAX_PAIRS);
    return MAV_OK;
}
extern "C" int mav_find_homography_dev(mav_ctx* c, const double* src, const double* dst, int n, int batch, double* H, int32_t* ok)
{
    CHK(check_dev_call(c, batch, "mav_find_homography_dev"));
    if (!src || !dst || !H || !ok) return fail(MAV_ERR_ARG, "mav_find_homography_dev: NULL argument");
    CHK(check_pairs("mav_find_homography_dev", n));
    CHK(ensure_pairs(c, n));
    launch_homography_fit(c->stream, src, dst, n, batch, c->gm.work, H, ok);
    return check_launch("homography_fit");
}
extern "C" int mav_find_homography(mav_ctx* c, const double* src, const double* dst, int n, int batch, double* H, int32_t* ok)
{
    HostCall h(c, "mav_find_homography");
    CHK(h.fresh(batch));
    if (!src || !dst || !H || !ok) return fail(MAV_ERR_ARG, "mav_find_homography: NULL argument");
    CHK(check_pairs("mav_find_homography", n));
    const size_t bytes = sizeof(double) * 2 * (size_t)n * batch;
    const double *ds = h.in(src, bytes), *dd = h.in(dst, bytes);
    double* dH = h.out(H, sizeof(double) * 9 * batch);
    int32_t* dok = h.out(ok, sizeof(int32_t) * batch);
    CHK(h.staged());
    CHK(mav_find_homography_dev(c, ds, dd, n, batch, dH, dok));
    return h.finish();
}
// n and the coords (host) of a call that samples a flow field: the pair count, every sample inside the frame
static int check_coords(const mav_ctx* c, const char* fn, const int32_t* coords, int n)
{
    CHK(check_pairs(fn, n));
    for (int i = 0; i < n; i++)
        if (coords[2 * i] < 0 || coords[2 * i] >= c->W || coords[2 * i + 1] < 0 || coords[2 * i + 1] >= c->H)
            return fail(MAV_ERR_ARG, "%s: sample %d = (%d, %d) lies outside the %dx%d frame", fn, i, coords[2 * i], coords[2 * i + 1], c->W, c->H);
    return MAV_OK;
}
// coords (host) range-checked and brought to the context's buffer, then the pairs of `flow` gathered into the context's pair buffers
static int gather_pairs(mav_ctx* c, const char* fn, const float* flow, const int32_t* coords, int n, int batch)
{
    CHK(check_coords(c, fn, coords, n));
    CHK(ensure_pairs(c, n));
    HIPCHK(hipMemcpyAsync(c->gm.coords, coords, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    launch_pair_gather(c->stream, flow, c->gm.coords, n, batch, c->W, c->H, c->gm.src, c->gm.dst);
    return check_launch("pair_gather");
}
extern "C" int mav_flow_homography_dev(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, double* H, int32_t* ok)
{
    CHK(check_dev_call(c, batch, "mav_flow_homography_dev"));
    if (!flow || !coords || !H || !ok) return fail(MAV_ERR_ARG, "mav_flow_homography_dev: NULL argument");
    CHK(gather_pairs(c, "mav_flow_homography_dev", flow, coords, n, batch));
    launch_homography_fit(c->stream, c->gm.src, c->gm.dst, n, batch, c->gm.work, H, ok);
    return check_launch("homography_fit");
}
extern "C" int mav_flow_homography(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, double* H, int32_t* ok, double* pairs_dst)
{
    HostCall h(c, "mav_flow_homography");
    CHK(h.fresh(batch));
    if (!flow || !coords || !H || !ok) return fail(MAV_ERR_ARG, "mav_flow_homography: NULL argument");
    CHK(check_pairs("mav_flow_homography", n));
    CHK(ensure_pairs(c, n));
    const float* df = h.in(flow, c->n0 * batch * 2 * sizeof(float));
    double* dH = h.out(H, sizeof(double) * 9 * batch);
    int32_t* dok = h.out(ok, sizeof(int32_t) * batch);
    h.fetch(pairs_dst, c->gm.dst, sizeof(double) * 2 * (size_t)n * batch);
    CHK(h.staged());
    CHK(mav_flow_homography_dev(c, df, coords, n, batch, dH, dok));
    return h.finish();
}
// passes A and B, the window search and the records, all on the compute stream.  M: item b's matrix at M + b * m_stride; ok: null, or
// the fit's flags (a failed item's record is zeroed).
static int global_motion_enqueue(mav_ctx* c, const char* fn, const float* flow, const double* M, int m_stride, const int* ok, int batch, double scale,
                                 int optimize, float* warped, float* mag, uint8_t* gray, mav_motion_result* results)
{
    if (!flow || !M || !results) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    PyrPlan p;
    CHK(pyr_plan(c, scale, c->max_batch, &p));
    CHK(ensure_pyr_ws(c, p));
    CHK(ensure_motion(c));
    if (optimize && !c->sat) CHK(c->mem.alloc(&c->sat, sizeof(unsigned long long) * (size_t)(c->W + 1) * (c->H + 1) * c->max_batch, MEM_OTHER, "summed-area tables"));
    if (!gray) {
        if (!c->gm.gray) CHK(c->mem.alloc(&c->gm.gray, c->n0 * c->max_batch, MEM_OTHER, "global-motion image"));
        gray = c->gm.gray;
    }
    unsigned long long *kmax = c->gm.key, *kwin = c->gm.key + batch;
    HIPCHK(hipMemsetAsync(c->gm.key, 0, sizeof(unsigned long long) * 2 * batch, c->stream));
    launch_motion_pass_a(c->stream, flow, M, m_stride, batch, c->W, c->H, warped, mag, nullptr, kmax);
    launch_motion_pass_b(c->stream, flow, M, m_stride, batch, c->W, c->H, kmax, gray);
    build_pyramid(c, p, gray, batch, p.n - 1);
    for (int l = 0; l < p.n; l++)
        launch_level_scan(c->stream, l == 0 ? gray : c->pyr_ws + p.off[l], (size_t)p.w[l] * p.h[l], batch, p.w[l], p.h[l], p.base[l], kwin);
    launch_pyramid_finalize(c->stream, kwin, p, gray, c->pyr_ws, batch, c->gm.pyr);
    launch_motion_window(c->stream, c->gm.pyr, batch, c->gm.win);
    if (optimize) launch_optimize_window(c->stream, gray, batch, c->W, c->H, c->sat, c->gm.win, c->gm.opt_score, c->gm.opt_win);
    launch_motion_pack(c->stream, kmax, c->gm.pyr, c->gm.win, optimize ? c->gm.opt_score : nullptr, optimize ? c->gm.opt_win : nullptr, ok, batch,
                       c->W, results);
    CHK(check_launch("global_motion"));
    c->gm.last.flow = flow; c->gm.last.M = M; c->gm.last.m_stride = m_stride; c->gm.last.batch = batch;
    return MAV_OK;
}
extern "C" int mav_global_motion_dev(mav_ctx* c, const float* flow, const double* M, int batch, double scale, int optimize, float* warped,
                                     float* mag, uint8_t* gray, mav_motion_result* results)
{
    CHK(check_dev_call(c, batch, "mav_global_motion_dev"));
    return global_motion_enqueue(c, "mav_global_motion_dev", flow, M, 6, nullptr, batch, scale, optimize, warped, mag, gray, results);
}
extern "C" int mav_global_motion(mav_ctx* c, const float* flow, const double* M, int batch, double scale, int optimize, float* warped, float* mag,
                                 uint8_t* gray, mav_motion_result* results)
{
    HostCall h(c, "mav_global_motion");
    CHK(h.fresh(batch));
    if (!flow || !M || !results) return fail(MAV_ERR_ARG, "mav_global_motion: NULL argument");
    PyrPlan p;
    CHK(pyr_plan(c, scale, c->max_batch, &p));           // (before anything is staged)
    const size_t n = c->n0 * batch;
    const float* df = h.in(flow, n * 2 * sizeof(float));
    const double* dM = h.in(M, sizeof(double) * 6 * batch);
    mav_motion_result* dres = h.out(results, sizeof(mav_motion_result) * batch);
    float* dw = h.out(warped, n * 2 * sizeof(float));
    float* dm = h.out(mag, n * sizeof(float));
    uint8_t* dg = h.out(gray, n);
    CHK(h.staged());
    CHK(global_motion_enqueue(c, "mav_global_motion", df, dM, 6, nullptr, batch, scale, optimize, dw, dm, dg, dres));
    return h.finish();
}
extern "C" int mav_global_motion_step_dev(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, double scale, int optimize,
                                          double* H, int32_t* ok, uint8_t* gray, mav_motion_result* results)
{
    CHK(check_dev_call(c, batch, "mav_global_motion_step_dev"));
    if (!flow || !coords || !results) return fail(MAV_ERR_ARG, "mav_global_motion_step_dev: NULL argument");
    PyrPlan p;
    CHK(pyr_plan(c, scale, c->max_batch, &p));           // (before anything is enqueued)
    CHK(gather_pairs(c, "mav_global_motion_step_dev", flow, coords, n, batch));
    if (!H) H = c->gm.H;
    if (!ok) ok = c->gm.ok;
    launch_homography_fit(c->stream, c->gm.src, c->gm.dst, n, batch, c->gm.work, H, ok);
    return global_motion_enqueue(c, "mav_global_motion_step_dev", flow, H, 9, ok, batch, scale, optimize, nullptr, nullptr, gray, results);
}
// The fused call of the branch: everything mav_farneback_dev and the step would refuse is refused here, before either enqueues anything.
static int check_motion_batch(mav_ctx* c, const char* fn, const void* prev, const void* next, const int32_t* coords, int n, double scale,
                              const void* results)
{
    if (!prev || !next || !coords || !results) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    CHK(check_coords(c, fn, coords, n));
    PyrPlan p;
    return pyr_plan(c, scale, c->max_batch, &p);
}
extern "C" int mav_global_motion_batch_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const int32_t* coords, int n, int batch,
                                           double scale, int optimize, float* flow, double* H, int32_t* ok, uint8_t* gray,
                                           mav_motion_result* results)
{
    CHK(check_dev_call(c, batch, "mav_global_motion_batch_dev"));
    CHK(check_motion_batch(c, "mav_global_motion_batch_dev", prev, next, coords, n, scale, results));
    if (!flow) {
        CHK(ensure_flow_ws(c));
        flow = c->flow_ws;
    }
    CHK(mav_farneback_dev(c, prev, next, batch, flow));
    return mav_global_motion_step_dev(c, flow, coords, n, batch, scale, optimize, H, ok, gray, results);
}
extern "C" int mav_global_motion_batch(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const int32_t* coords, int n, int batch, double scale,
                                       int optimize, float* flow, double* H, int32_t* ok, uint8_t* gray, mav_motion_result* results)
{
    HostCall h(c, "mav_global_motion_batch");
    CHK(h.fresh(batch));
    CHK(check_motion_batch(c, "mav_global_motion_batch", prev, next, coords, n, scale, results));     // (before anything is staged)
    const size_t px = c->n0 * batch;
    const void *dprev, *dnext;
    upload_frames(h, prev, next, batch, 1, &dprev, &dnext);
    float* df = h.out(flow, px * 2 * sizeof(float));
    double* dH = h.out(H, sizeof(double) * 9 * batch);
    int32_t* dok = h.out(ok, sizeof(int32_t) * batch);
    uint8_t* dg = h.out(gray, px);
    mav_motion_result* dres = h.out(results, sizeof(mav_motion_result) * batch);
    CHK(h.staged());
    CHK(mav_global_motion_batch_dev(c, (const uint8_t*)dprev, (const uint8_t*)dnext, coords, n, batch, scale, optimize, df, dH, dok, dg, dres));
    return h.finish();
}
extern "C" int mav_last_global_motion_render(mav_ctx* c, int batch, uint8_t* img_warped, uint8_t* img_global)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_last_global_motion_render: NULL context");
    if (!c->gm.last.batch || batch != c->gm.last.batch)
        return fail(MAV_ERR_STATE, "mav_last_global_motion_render: no flow of a %d-item global-motion call is resident", batch);
    HostCall h(c, "mav_last_global_motion_render");
    CHK(h.after_last());
    if (!img_warped && !img_global) return MAV_OK;
    const size_t n = c->n0 * batch;
    float* field = h.scratch<float>(n * 2 * sizeof(float));
    uint8_t *dw = h.out(img_warped, n * 3), *dg = h.out(img_global, n * 3);
    CHK(h.staged());
    CHK(ensure_render(c));
    const DerotParams* derot = nullptr;                  // float32 fields: numpy's float32 arithmetic, i.e. the frame-0 form
    std::vector<uint8_t> all(batch, 1);
    CHK(upload_derot(c, nullptr, nullptr, all.data(), batch, true, &derot, c->render_derot));
    const mav_ctx::Motion::Last& l = c->gm.last;
    for (int k = 0; k < 2; k++) {
        uint8_t* img = k == 0 ? dw : dg;
        if (!img) continue;
        launch_motion_pass_a(c->stream, l.flow, l.M, l.m_stride, batch, c->W, c->H, k == 0 ? field : nullptr, nullptr, k == 1 ? field : nullptr, nullptr);
        launch_render_f32(c->stream, field, derot, nullptr, nullptr, batch, c->W, c->H, mav_thr_params{}, c->render_max, nullptr, img, nullptr);
    }
    CHK(check_launch("global_motion render"));
    return h.finish();
}

extern "C" int mav_tpr_fpr_counts(mav_ctx* c, const uint8_t* gt, const uint8_t* mask, int mask_value, int batch, int64_t* counts)
{
    HostCall h(c, "mav_tpr_fpr_counts");
    CHK(h.fresh(batch));
    if (!gt || !mask || !counts) return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts: NULL argument");
    if (mask_value < 1 || mask_value > 65535) return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts: mask_value %d outside [1, 65535]", mask_value);
    const uint8_t* dg = h.in(gt, c->n0 * batch);
    const uint8_t* dm = h.in(mask, c->n0 * batch);
    h.fetch(counts, c->u64_scratch, sizeof(int64_t) * 4 * batch);
    CHK(h.staged());
    launch_tpr_fpr(c->stream, dg, dm, (unsigned)mask_value, batch, c->W, c->H, c->u64_scratch);
    CHK(check_launch("tpr_fpr"));
    return h.finish();
}

// frames (mav_process_batch) or a float32 flow field (mav_detect) in, masks and records out: one body for both
struct ProcessArgs {
    const uint8_t *prev = nullptr, *next = nullptr;      // the frames ...
    const float* flow_in = nullptr;                      // ... or their flow
    const uint32_t* samples = nullptr;
    const double *omega = nullptr, *dt = nullptr;
    const uint8_t *frame0 = nullptr, *sky = nullptr;
    const mav_foe_params* foe_par = nullptr;
    const mav_thr_params* thr = nullptr;
    float* flow_out = nullptr;                           // outputs: only the records are always wanted
    double* phi = nullptr;
    uint8_t *mask_fixed = nullptr, *mask_dyn = nullptr;
    mav_result* results = nullptr;
};
static int process_host(mav_ctx* c, const char* fn, int batch, const ProcessArgs& a)
{
    HostCall h(c, fn);
    CHK(h.fresh(batch));
    if ((!a.flow_in && (!a.prev || !a.next)) || !a.samples || !a.results) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    mav_foe_params f;
    CHK(foe_checked(c, a.foe_par, &f));
    const size_t n = c->n0 * batch, flow_bytes = n * 2 * sizeof(float);
    const void *dprev = nullptr, *dnext = nullptr;
    float* dflow;                                        // the always-present buffers take the first blocks
    if (a.flow_in) dflow = h.in(a.flow_in, flow_bytes);
    else {
        upload_frames(h, a.prev, a.next, batch, 1, &dprev, &dnext);
        dflow = h.scratch<float>(flow_bytes);
    }
    h.fetch(a.flow_out, dflow, flow_bytes);
    const uint32_t* ds = h.in(a.samples, sizeof(uint32_t) * 4 * (size_t)f.n_pairs * batch);
    mav_result* dres = h.out(a.results, sizeof(mav_result) * batch);
    uint8_t* dmf = h.out(a.mask_fixed, n);
    uint8_t* dmd = h.out(a.mask_dyn, n);
    const uint8_t* dsky = h.in(a.sky, n);
    const double* dom = h.in(a.omega, sizeof(double) * 3 * batch);
    const double* ddt = h.in(a.omega ? a.dt : nullptr, sizeof(double) * batch);
    const uint8_t* df0 = h.in(a.frame0, batch);
    double* dphi = h.out(a.phi, n * sizeof(double));
    CHK(h.staged());
    if (!a.flow_in) CHK(mav_farneback_dev(c, (const uint8_t*)dprev, (const uint8_t*)dnext, batch, dflow));
    CHK(detect_checked(c, dflow, ds, dom, ddt, df0, dsky, batch, f, a.thr, dphi, dmf, dmd, dres));
    c->last_mf = dmf; c->last_md = dmd; c->last_mask_batch = batch;
    return h.finish();
}

extern "C" int mav_last_masks_tpr_fpr(mav_ctx* c, const uint8_t* gt, int mask_value, int batch, int64_t* counts_fixed, int64_t* counts_dyn)
{
    if (!c || !gt) return fail(MAV_ERR_ARG, "mav_last_masks_tpr_fpr: NULL argument");
    if (mask_value < 1 || mask_value > 65535) return fail(MAV_ERR_ARG, "mav_last_masks_tpr_fpr: mask_value %d outside [1, 65535]", mask_value);
    if (!c->last_mask_batch || batch != c->last_mask_batch || (counts_fixed && !c->last_mf) || (counts_dyn && !c->last_md))
        return fail(MAV_ERR_STATE, "mav_last_masks_tpr_fpr: no masks of a %d-pair detection call are resident", batch);
    HostCall h(c, "mav_last_masks_tpr_fpr");
    CHK(h.after_last());
    if (!counts_fixed && !counts_dyn) return MAV_OK;
    const uint8_t* dg = h.in(gt, c->n0 * batch);
    // one pass over the ground truth for both masks
    unsigned long long *c0 = c->u64_scratch, *c1 = c->u64_scratch + 4 * (size_t)batch;
    const uint8_t* m0 = counts_fixed ? c->last_mf : c->last_md;
    const uint8_t* m1 = (counts_fixed && counts_dyn) ? c->last_md : nullptr;
    h.fetch(counts_fixed ? counts_fixed : counts_dyn, c0, sizeof(int64_t) * 4 * batch);
    h.fetch(m1 ? counts_dyn : nullptr, c1, sizeof(int64_t) * 4 * batch);
    CHK(h.staged());
    launch_tpr_fpr2(c->stream, dg, c->n0, m0, m1, (unsigned)mask_value, batch, c->W, c->H, c0, m1 ? c1 : nullptr);
    CHK(check_launch("tpr_fpr"));
    return h.finish();
}

// mask == NULL: the resident mask `resident` of the last detection call (the call appends its blocks behind that call's)
static int components_host(mav_ctx* c, const char* fn, const uint8_t* mask, const uint8_t* resident, int batch, const mav_cc_params* pp,
                           int32_t* labels, mav_cc_counts* counts, mav_blob* blobs)
{
    mav_cc_params p;
    CHK(cc_params_checked(pp, &p, fn));
    HostCall h(c, fn);
    if (resident) CHK(h.after_last()); else CHK(h.fresh(batch));
    const size_t n = c->n0 * batch;
    const uint8_t* dm = resident ? resident : h.in(mask, n);
    int32_t* dl = h.out(labels, n * sizeof(int32_t));
    mav_cc_counts* dc = h.out(counts, sizeof(mav_cc_counts) * batch);
    mav_blob* db = h.out(blobs, sizeof(mav_blob) * (size_t)p.max_blobs * batch);
    CHK(h.staged());
    CHK(components_enqueue(c, dm, batch, p, dl, dc, db));
    return h.finish();
}
extern "C" int mav_components(mav_ctx* c, const uint8_t* mask, int batch, const mav_cc_params* pp, int32_t* labels, mav_cc_counts* counts,
                              mav_blob* blobs)
{
    if (!c || !mask || !counts || !blobs) return fail(MAV_ERR_ARG, "mav_components: NULL argument");
    return components_host(c, "mav_components", mask, nullptr, batch, pp, labels, counts, blobs);
}
extern "C" int mav_last_masks_components(mav_ctx* c, int which, int batch, const mav_cc_params* pp, int32_t* labels, mav_cc_counts* counts,
                                         mav_blob* blobs)
{
    if (!c || !counts || !blobs) return fail(MAV_ERR_ARG, "mav_last_masks_components: NULL argument");
    if (which != 0 && which != 1) return fail(MAV_ERR_ARG, "mav_last_masks_components: which must be 0 (fixed) or 1 (dynamic), got %d", which);
    const uint8_t* m = which == 0 ? c->last_mf : c->last_md;
    if (!c->last_mask_batch || batch != c->last_mask_batch || !m)
        return fail(MAV_ERR_STATE, "mav_last_masks_components: no %s mask of a %d-pair detection call is resident", which ? "dynamic" : "fixed", batch);
    return components_host(c, "mav_last_masks_components", nullptr, m, batch, pp, labels, counts, blobs);
}

// calculate_tpr_fpr of one or two device-resident masks against a device-resident ground truth, counts left on the device: the
// validation tail of a batch [src/processor.py:350-351] as two more launches behind mav_process_batch_dev, no transfer, no sync.
extern "C" int mav_tpr_fpr_counts_dev(mav_ctx* c, const uint8_t* gt, int gt_images, const uint8_t* mask_fixed, const uint8_t* mask_dyn,
                                      int mask_value, int batch, int64_t* counts_fixed, int64_t* counts_dyn)
{
    if (!c || !gt) return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts_dev: NULL argument");
    CHK(check_dev_call(c, batch, "mav_tpr_fpr_counts_dev"));
    if (gt_images != 1 && gt_images != batch) return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts_dev: gt_images must be 1 (shared) or batch (%d), got %d", batch, gt_images);
    if (mask_value < 1 || mask_value > 65535) return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts_dev: mask_value %d outside [1, 65535]", mask_value);
    if ((mask_fixed && !counts_fixed) || (mask_dyn && !counts_dyn) || (!mask_fixed && !mask_dyn))
        return fail(MAV_ERR_ARG, "mav_tpr_fpr_counts_dev: every mask needs its counts buffer, and at least one mask");
    const size_t stride = gt_images == 1 && batch > 1 ? 0 : c->n0;
    const uint8_t* m0 = mask_fixed ? mask_fixed : mask_dyn;
    const uint8_t* m1 = (mask_fixed && mask_dyn) ? mask_dyn : nullptr;
    ProfScope ps(c, K_MISC);
    launch_tpr_fpr2(c->stream, gt, stride, m0, m1, (unsigned)mask_value, batch, c->W, c->H,
                    (unsigned long long*)(mask_fixed ? counts_fixed : counts_dyn), (unsigned long long*)(m1 ? counts_dyn : nullptr));
    return check_launch("tpr_fpr");
}

// ---- result images (include/mavflow.h: mav_render) ----------------------------------------------------------------------------
static int ensure_render(mav_ctx* c)
{
    if (c->render_max) return MAV_OK;
    return c->mem.alloc_set({{&c->render_max, sizeof(unsigned long long) * c->max_batch}, {&c->render_derot, sizeof(DerotParams) * c->max_batch}},
                            MEM_OTHER, "render scratch");
}
static int render_enqueue(mav_ctx* c, const float* flow, const DerotParams* derot, const double* foe, const uint8_t* sky, int batch,
                          const mav_thr_params& t, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi)
{
    CHK(ensure_render(c));
    ProfScope ps(c, K_MISC);
    launch_render_f32(c->stream, flow, derot, foe, sky, batch, c->W, c->H, t, c->render_max, img_result, img_flow, img_phi);
    return check_launch("render");
}

extern "C" int mav_render_dev(mav_ctx* c, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                              const uint8_t* sky, int batch, const mav_thr_params* tp, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi)
{
    if (!c || !flow || ((img_result || img_phi) && !foe)) return fail(MAV_ERR_ARG, "mav_render_dev: NULL argument");
    CHK(check_dev_call(c, batch, "mav_render_dev"));
    CHK(ensure_render(c));
    const DerotParams* derot = nullptr;
    CHK(upload_derot(c, omega, dt, frame0, batch, false, &derot, c->render_derot));
    return render_enqueue(c, flow, derot, foe, sky, batch, thr_or_defaults(tp), img_result, img_flow, img_phi);
}

extern "C" int mav_render(mav_ctx* c, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                          const uint8_t* sky, int batch, const mav_thr_params* tp, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi)
{
    HostCall h(c, "mav_render");
    CHK(h.fresh(batch));
    if (!flow || ((img_result || img_phi) && !foe)) return fail(MAV_ERR_ARG, "mav_render: NULL argument");
    if (!img_result && !img_flow && !img_phi) return MAV_OK;
    const size_t n = c->n0 * batch;
    const float* df = h.in(flow, n * 2 * sizeof(float));
    const double* dfoe = h.in(foe, sizeof(double) * 2 * batch);
    const uint8_t* dsky = h.in(sky, n);
    const double* dom = h.in(omega, sizeof(double) * 3 * batch);
    const double* ddt = h.in(omega ? dt : nullptr, sizeof(double) * batch);
    const uint8_t* df0 = h.in(frame0, batch);
    uint8_t *dres = h.out(img_result, n * 3), *dfl = h.out(img_flow, n * 3), *dphi = h.out(img_phi, n * 3);   // each (batch, H, W, 3)
    CHK(h.staged());
    CHK(mav_render_dev(c, df, dfoe, dom, ddt, df0, dsky, batch, tp, dres, dfl, dphi));
    return h.finish();
}

extern "C" int mav_last_render(mav_ctx* c, int batch, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_last_render: NULL context");
    if (!c->last_render.batch || batch != c->last_render.batch)
        return fail(MAV_ERR_STATE, "mav_last_render: no flow of a %d-pair detection call is resident", batch);
    HostCall h(c, "mav_last_render");
    CHK(h.after_last());
    if (!img_result && !img_flow && !img_phi) return MAV_OK;
    const size_t bytes = c->n0 * 3 * batch;
    uint8_t *dres = h.out(img_result, bytes), *dfl = h.out(img_flow, bytes), *dphi = h.out(img_phi, bytes);
    CHK(h.staged());
    const mav_ctx::LastRender& r = c->last_render;
    CHK(render_enqueue(c, r.flow, r.derot, r.foe, r.sky, batch, r.thr, dres, dfl, dphi));
    return h.finish();
}

// ---- threshold sweep: the entry points (the core is in front of the frame step) -------------------------------------------------------
static int roc_gt_images_checked(int gt_images, int batch, const char* fn)
{
    if (gt_images != 1 && gt_images != batch) return fail(MAV_ERR_ARG, "%s: gt_images must be 1 (shared) or batch (%d), got %d", fn, batch, gt_images);
    return MAV_OK;
}
extern "C" int mav_roc_sweep_dev(mav_ctx* c, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                                 const uint8_t* sky, const uint8_t* gt, int gt_images, int batch, const mav_thr_params* tp,
                                 const mav_roc_params* rp, int64_t* table)
{
    (void)tp;                                    // nothing of it is read: the lists replace its fixed fields, the dynamic ones are ignored
    if (!c || !flow || !foe || !gt || !table) return fail(MAV_ERR_ARG, "mav_roc_sweep_dev: NULL argument");
    RocThr t;
    CHK(roc_params_checked(rp, &t, "mav_roc_sweep_dev"));
    CHK(check_dev_call(c, batch, "mav_roc_sweep_dev"));
    CHK(roc_gt_images_checked(gt_images, batch, "mav_roc_sweep_dev"));
    CHK(ensure_render(c));
    const DerotParams* derot = nullptr;
    CHK(upload_derot(c, omega, dt, frame0, batch, false, &derot, c->render_derot));
    return roc_enqueue(c, flow, false, derot, foe, sky, gt, gt_images, batch, t, table);
}
extern "C" int mav_roc_sweep(mav_ctx* c, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                             const uint8_t* sky, const uint8_t* gt, int gt_images, int batch, const mav_thr_params* tp,
                             const mav_roc_params* rp, int64_t* table)
{
    if (!c || !flow || !foe || !gt || !table) return fail(MAV_ERR_ARG, "mav_roc_sweep: NULL argument");
    RocThr t;
    CHK(roc_params_checked(rp, &t, "mav_roc_sweep"));
    HostCall h(c, "mav_roc_sweep");
    CHK(h.fresh(batch));
    CHK(roc_gt_images_checked(gt_images, batch, "mav_roc_sweep"));
    const size_t n = c->n0 * batch;
    const float* df = h.in(flow, n * 2 * sizeof(float));
    const double* dfoe = h.in(foe, sizeof(double) * 2 * batch);
    const uint8_t* dsky = h.in(sky, n);
    const uint8_t* dgt = h.in(gt, c->n0 * gt_images);
    const double* dom = h.in(omega, sizeof(double) * 3 * batch);
    const double* ddt = h.in(omega ? dt : nullptr, sizeof(double) * batch);
    const uint8_t* df0 = h.in(frame0, batch);
    int64_t* dtab = h.out(table, sizeof(int64_t) * MAV_ROC_TABLE_WORDS(t.ka, t.km) * batch);
    CHK(h.staged());
    CHK(mav_roc_sweep_dev(c, df, dfoe, dom, ddt, df0, dsky, dgt, gt_images, batch, tp, rp, dtab));
    return h.finish();
}
extern "C" int mav_last_roc_sweep(mav_ctx* c, const uint8_t* gt, int gt_images, int batch, const mav_roc_params* rp, int64_t* table)
{
    if (!c || !gt || !table) return fail(MAV_ERR_ARG, "mav_last_roc_sweep: NULL argument");
    RocThr t;
    CHK(roc_params_checked(rp, &t, "mav_last_roc_sweep"));
    if (!c->last_roc.batch || batch != c->last_roc.batch)
        return fail(MAV_ERR_STATE, "mav_last_roc_sweep: no flow of a %d-pair detection call is resident", batch);
    CHK(roc_gt_images_checked(gt_images, batch, "mav_last_roc_sweep"));
    HostCall h(c, "mav_last_roc_sweep");
    CHK(h.after_last());
    const uint8_t* dgt = h.in(gt, c->n0 * gt_images);
    int64_t* dtab = h.out(table, sizeof(int64_t) * MAV_ROC_TABLE_WORDS(t.ka, t.km) * batch);
    CHK(h.staged());
    const mav_ctx::LastRoc& r = c->last_roc;
    CHK(roc_enqueue(c, r.flow, r.f64, r.derot, r.foe, r.sky, dgt, gt_images, batch, t, dtab));
    return h.finish();
}
extern "C" int mav_roc_arm(mav_ctx* c, const mav_roc_params* rp, size_t off_table)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_roc_arm: NULL context");
    RocThr t;
    if (rp) CHK(roc_params_checked(rp, &t, "mav_roc_arm"));
    if (rp && off_table % 8) return fail(MAV_ERR_ARG, "mav_roc_arm: off_table %zu is not a multiple of 8", off_table);
    CHK(mav_worker_drain(c));                    // the worker reads this state while it enqueues posted steps (as mav_frame_step_dev drains)
    if (!rp) { c->roc_armed = false; return MAV_OK; }
    c->roc_thr = t; c->roc_off = off_table; c->roc_armed = true;
    return MAV_OK;
}

// ---- flow history (include/mavflow.h: mav_history_*) -------------------------------------------------------------------------------------
extern "C" void mav_history_defaults(mav_history_params* p) { *p = mav_history_params{20, MAV_DEPTH_32F, 0}; }
// Detector.get_history's loop (detector.py:376-385) taken literally.  k moves through 0 .. L - 1 cyclically and the target is one of
// those values, so the walk ends within L - 1 steps for every L >= 3.
extern "C" int mav_history_schedule(int length, int index, int* slots, int* n)
{
    if (length < 3 || length > MAV_HISTORY_MAX_LENGTH) return fail(MAV_ERR_ARG, "mav_history_schedule: length %d outside [3, %d]", length, MAV_HISTORY_MAX_LENGTH);
    if (index < 0 || index >= length) return fail(MAV_ERR_ARG, "mav_history_schedule: index %d outside [0, %d]", index, length - 1);
    if (!slots || !n) return fail(MAV_ERR_ARG, "mav_history_schedule: NULL slots or n");
    int cnt = 0;
    for (int k = (index + 1) % (length - 1); k != index % (length - 1); k = (k + 1) % length) slots[cnt++] = k;
    *n = cnt;
    return MAV_OK;
}
static size_t depth_bytes(int depth) { return depth == MAV_DEPTH_64F ? sizeof(double) : sizeof(float); }
static int history_owned(mav_ctx* c, const mav_history* h, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!h) return fail(MAV_ERR_ARG, "%s: NULL history", fn);
    if (std::find(c->histories.begin(), c->histories.end(), h) == c->histories.end())
        return fail(MAV_ERR_ARG, "%s: history is not one of this context's", fn);
    return MAV_OK;
}
extern "C" int mav_history_create(mav_ctx* c, const mav_history_params* pp, mav_history** out)
{
    if (!c || !out) return fail(MAV_ERR_ARG, "mav_history_create: NULL %s", !c ? "context" : "out");
    mav_history_params p;
    if (pp) p = *pp; else mav_history_defaults(&p);
    if (p.length < 3 || p.length > MAV_HISTORY_MAX_LENGTH) return fail(MAV_ERR_ARG, "mav_history_create: length %d outside [3, %d]", p.length, MAV_HISTORY_MAX_LENGTH);
    if (p.depth != MAV_DEPTH_32F && p.depth != MAV_DEPTH_64F) return fail(MAV_ERR_ARG, "mav_history_create: depth %d is neither MAV_DEPTH_32F nor MAV_DEPTH_64F", p.depth);
    if (p.flags & ~MAV_HISTORY_AXES_XY) return fail(MAV_ERR_ARG, "mav_history_create: unknown flags 0x%x", p.flags);
    HIPCHK(hipSetDevice(c->device));
    mav_history* h = new mav_history;
    h->length = p.length; h->depth = p.depth; h->flags = p.flags;
    h->ring_bytes = (size_t)p.length * c->n0 * 2 * depth_bytes(p.depth);
    int rc = c->mem.alloc(&h->ring, h->ring_bytes, MEM_OTHER, "flow history ring");
    if (rc == MAV_OK && hipMemsetAsync(h->ring, 0, h->ring_bytes, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        c->mem.release(h->ring);
        rc = fail(MAV_ERR_HIP, "mav_history_create: zeroing the ring failed");
    }
    if (rc != MAV_OK) { delete h; return rc; }
    c->histories.push_back(h);
    *out = h;
    return MAV_OK;
}
extern "C" int mav_history_destroy(mav_ctx* c, mav_history* h)
{
    CHK(history_owned(c, h, "mav_history_destroy"));
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));       // enqueued pushes may still read the ring
    c->mem.release(h->ring);
    c->histories.erase(std::find(c->histories.begin(), c->histories.end(), h));
    delete h;
    return MAV_OK;
}
extern "C" int mav_history_reset(mav_ctx* c, mav_history* h)
{
    CHK(history_owned(c, h, "mav_history_reset"));
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(h->ring, 0, h->ring_bytes, c->stream));
    h->index = 0;
    h->pushes = 0;
    return MAV_OK;
}
extern "C" int mav_history_info(mav_ctx* c, const mav_history* h, int* index, long* pushes, size_t* ring_bytes)
{
    CHK(history_owned(c, h, "mav_history_info"));
    if (index) *index = h->index;
    if (pushes) *pushes = h->pushes;
    if (ring_bytes) *ring_bytes = h->ring_bytes;
    return MAV_OK;
}
// Everything a push can be refused for, host or device pointers alike: nothing has been enqueued or changed when this fails.  What can
// be judged from the arguments alone comes before the context or the history is looked at (tests/test_abi_history.py passes handles
// that must never be dereferenced).
static int history_push_checked(mav_ctx* c, const mav_history* h, const void* flow, int flow_depth, int count, int out_form, const void* out,
                                const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!h) return fail(MAV_ERR_ARG, "%s: NULL history", fn);
    if (!flow) return fail(MAV_ERR_ARG, "%s: NULL flow", fn);
    if (!out) return fail(MAV_ERR_ARG, "%s: NULL out", fn);
    if (flow_depth != MAV_DEPTH_32F && flow_depth != MAV_DEPTH_64F) return fail(MAV_ERR_ARG, "%s: flow_depth %d is neither MAV_DEPTH_32F nor MAV_DEPTH_64F", fn, flow_depth);
    if (out_form != MAV_HISTORY_OUT_REFERENCE && out_form != MAV_HISTORY_OUT_FLOW_F32) return fail(MAV_ERR_ARG, "%s: unknown out_form %d", fn, out_form);
    if (count < 1) return fail(MAV_ERR_ARG, "%s: count %d is less than 1", fn, count);
    const size_t fe = depth_bytes(flow_depth), oe = out_form == MAV_HISTORY_OUT_FLOW_F32 ? sizeof(float) : sizeof(double);
    if ((uintptr_t)flow % fe) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its %zu-byte elements", fn, fe);
    if ((uintptr_t)out % oe) return fail(MAV_ERR_ARG, "%s: out is not aligned to its %zu-byte elements", fn, oe);
    CHK(history_owned(c, h, fn));
    if (flow_depth == MAV_DEPTH_64F && h->depth == MAV_DEPTH_32F)
        return fail(MAV_ERR_ARG, "%s: flow_depth: a float64 field would be rounded into this float32 ring", fn);
    if ((size_t)count * c->n0 > MAV_MAX_BATCH_PIXELS) return fail(MAV_ERR_ARG, "%s: count %d above %zu fields of this size", fn, count, MAV_MAX_BATCH_PIXELS / c->n0);
    const uintptr_t f0 = (uintptr_t)flow, f1 = f0 + (size_t)count * c->n0 * 2 * fe, o0 = (uintptr_t)out, o1 = o0 + (size_t)count * c->n0 * 2 * oe;
    if (f0 < o1 && o0 < f1) return fail(MAV_ERR_ARG, "%s: flow and out overlap", fn);
    return MAV_OK;
}
extern "C" int mav_history_push_dev(mav_ctx* c, mav_history* h, const void* flow, int flow_depth, int count, int out_form, void* out)
{
    CHK(history_push_checked(c, h, flow, flow_depth, count, out_form, out, "mav_history_push_dev"));
    HIPCHK(hipSetDevice(c->device));
    const bool ring64 = h->depth == MAV_DEPTH_64F, flow64 = flow_depth == MAV_DEPTH_64F, out32 = out_form == MAV_HISTORY_OUT_FLOW_F32;
    const size_t field = c->n0 * 2, slot_bytes = field * depth_bytes(h->depth);
    for (int t = 0; t < count; t++) {
        int slots[MAV_HISTORY_MAX_LENGTH], n = 0;
        CHK(mav_history_schedule(h->length, h->index, slots, &n));
        HistSlots hs{};
        hs.n = n;
        for (int i = 0; i < n; i++) hs.w[i >> 2] |= (unsigned)slots[i] << ((i & 3) * 8);
        {
            ProfScope ps(c, K_HISTORY_PUT);
            launch_history_put(c->stream, (const char*)flow + (size_t)t * field * depth_bytes(flow_depth), flow64, (char*)h->ring + h->index * slot_bytes, ring64, c->W, c->H);
        }
        {
            ProfScope ps(c, K_HISTORY_TRACE);
            launch_history_trace(c->stream, h->ring, ring64, hs, c->W, c->H, (h->flags & MAV_HISTORY_AXES_XY) != 0, out32,
                                 (char*)out + (size_t)t * field * (out32 ? sizeof(float) : sizeof(double)));
        }
        h->index = (h->index + 1) % h->length;
        h->pushes++;
    }
    return check_launch("flow history");
}
extern "C" int mav_history_push(mav_ctx* c, mav_history* hist, const void* flow, int flow_depth, int count, int out_form, void* out)
{
    CHK(history_push_checked(c, hist, flow, flow_depth, count, out_form, out, "mav_history_push"));
    HostCall h(c, "mav_history_push");
    CHK(h.fresh());
    const size_t field = c->n0 * 2 * (size_t)count;
    const char* dflow = h.in((const char*)flow, field * depth_bytes(flow_depth));
    char* dout = h.out((char*)out, field * (out_form == MAV_HISTORY_OUT_FLOW_F32 ? sizeof(float) : sizeof(double)));
    CHK(h.staged());
    CHK(mav_history_push_dev(c, hist, dflow, flow_depth, count, out_form, dout));
    return h.finish();
}
extern "C" int mav_stage_remap_linear(mav_ctx* c, const void* src, int depth, const float* map_x, const float* map_y, double* out)
{
    if (!c || !src || !map_x || !map_y || !out) return fail(MAV_ERR_ARG, "mav_stage_remap_linear: NULL argument");
    if (depth != MAV_DEPTH_32F && depth != MAV_DEPTH_64F) return fail(MAV_ERR_ARG, "mav_stage_remap_linear: depth %d is neither MAV_DEPTH_32F nor MAV_DEPTH_64F", depth);
    HostCall h(c, "mav_stage_remap_linear");
    CHK(h.fresh());
    const char* dsrc = h.in((const char*)src, c->n0 * 2 * depth_bytes(depth));
    const float *dmx = h.in(map_x, c->n0 * sizeof(float)), *dmy = h.in(map_y, c->n0 * sizeof(float));
    double* dout = h.out(out, c->n0 * 2 * sizeof(double));
    CHK(h.staged());
    launch_remap_linear(c->stream, dsrc, depth == MAV_DEPTH_64F, dmx, dmy, c->W, c->H, dout);
    CHK(check_launch("remap"));
    return h.finish();
}

extern "C" int mav_flow_to_color(mav_ctx* c, const void* flow, int f64, int batch, uint8_t* img)
{
    HostCall h(c, "mav_flow_to_color");
    CHK(h.fresh(batch));
    if (!flow || !img) return fail(MAV_ERR_ARG, "mav_flow_to_color: NULL argument");
    const size_t n = c->n0 * batch;
    const void* df = h.in(flow, n * 2 * (f64 ? sizeof(double) : sizeof(float)));
    uint8_t* dimg = h.out(img, n * 3);
    CHK(h.staged());
    CHK(ensure_render(c));
    const DerotParams* derot = nullptr;
    if (!f64) {                      // a float32 field: numpy's float32 arithmetic, i.e. the frame-0 form
        std::vector<uint8_t> all(batch, 1);
        CHK(upload_derot(c, nullptr, nullptr, all.data(), batch, true, &derot, c->render_derot));
    }
    {
        ProfScope ps(c, K_MISC);
        if (f64) launch_render_f64(c->stream, (const double*)df, batch, c->W, c->H, c->render_max, dimg);
        else launch_render_f32(c->stream, (const float*)df, derot, nullptr, nullptr, batch, c->W, c->H, mav_thr_params{}, c->render_max, nullptr,
                               dimg, nullptr);
    }
    CHK(check_launch("render"));
    return h.finish();
}

extern "C" int mav_colormap_jet(mav_ctx* c, const uint8_t* gray, size_t n, uint8_t* bgr)
{
    if (!c || !gray || !bgr) return fail(MAV_ERR_ARG, "mav_colormap_jet: NULL argument");
    HostCall h(c, "mav_colormap_jet");
    CHK(h.fresh());
    if (!n) return MAV_OK;
    const uint8_t* dg = h.in(gray, n);
    uint8_t* dout = h.out(bgr, n * 3);
    CHK(h.staged());
    launch_colormap_jet(c->stream, dg, n, dout);
    CHK(check_launch("colormap"));
    return h.finish();
}

// ---- the processed.mp4 frame (include/mavflow.h: mav_overlay) ---------------------------------------------------------------------
static int check_radius(int radius, const char* fn)
{
    if (radius < 0 || radius > MAV_OVERLAY_MAX_RADIUS) return fail(MAV_ERR_ARG, "%s: radius %d outside [0, %d]", fn, radius, MAV_OVERLAY_MAX_RADIUS);
    return MAV_OK;
}
// FoEs in host memory: a NaN coordinate is where the reference's int() raises (|v| > 1e9, infinities included, is just not drawn)
static int check_foe_host(const double* foe, int batch, const char* what, const char* fn)
{
    for (int i = 0; i < 2 * batch; i++)
        if (std::isnan(foe[i])) return fail(MAV_ERR_ARG, "%s: %s[%d][%d] is NaN (int(nan) raises in the reference)", fn, what, i / 2, i % 2);
    return MAV_OK;
}

extern "C" int mav_overlay_dev(mav_ctx* c, const uint8_t* frames, const uint8_t* mask_fixed, const double* foe, const double* foe_gt,
                               int batch, int radius, uint8_t* overlay, uint8_t* written)
{
    if (!c || !frames || !mask_fixed || !foe || !foe_gt || !overlay || !written) return fail(MAV_ERR_ARG, "mav_overlay_dev: NULL argument");
    CHK(check_dev_call(c, batch, "mav_overlay_dev"));
    CHK(check_radius(radius, "mav_overlay_dev"));
    ProfScope ps(c, K_MISC);
    launch_overlay(c->stream, frames, mask_fixed, foe, foe_gt, batch, c->W, c->H, radius, overlay, written);
    return check_launch("overlay");
}

extern "C" int mav_overlay(mav_ctx* c, const uint8_t* frames, const uint8_t* mask_fixed, const double* foe, const double* foe_gt, int batch,
                           int radius, uint8_t* overlay, uint8_t* written)
{
    HostCall h(c, "mav_overlay");
    CHK(h.fresh(batch));
    if (!frames || !mask_fixed || !foe || !foe_gt || !overlay || !written) return fail(MAV_ERR_ARG, "mav_overlay: NULL argument");
    CHK(check_radius(radius, "mav_overlay"));
    CHK(check_foe_host(foe, batch, "foe", "mav_overlay"));
    CHK(check_foe_host(foe_gt, batch, "foe_gt", "mav_overlay"));
    const size_t n = c->n0 * batch;
    const uint8_t* df = h.in(frames, n * 3);
    const uint8_t* dm = h.in(mask_fixed, n);
    const double* dfoe = h.in(foe, sizeof(double) * 2 * batch);
    const double* dgt = h.in(foe_gt, sizeof(double) * 2 * batch);
    uint8_t* dout = h.out(overlay, n * 3);
    uint8_t* dw = h.out(written, batch);
    CHK(h.staged());
    CHK(mav_overlay_dev(c, df, dm, dfoe, dgt, batch, radius, dout, dw));
    return h.finish();
}

extern "C" int mav_last_overlay(mav_ctx* c, const uint8_t* frames, const double* foe_gt, int batch, int radius, uint8_t* overlay, uint8_t* written)
{
    if (!c || !frames || !foe_gt || !overlay || !written) return fail(MAV_ERR_ARG, "mav_last_overlay: NULL argument");
    CHK(check_dev_call(c, batch, "mav_last_overlay"));
    if (!c->last_render.batch || batch != c->last_render.batch || !c->last_render.mask_fixed)
        return fail(MAV_ERR_STATE, "mav_last_overlay: no fixed mask of a %d-pair detection call is resident", batch);
    CHK(check_radius(radius, "mav_last_overlay"));
    CHK(check_foe_host(foe_gt, batch, "foe_gt", "mav_last_overlay"));
    HostCall h(c, "mav_last_overlay");
    CHK(h.after_last());
    const size_t n = c->n0 * batch;
    const uint8_t* df = h.in(frames, n * 3);
    const double* dgt = h.in(foe_gt, sizeof(double) * 2 * batch);
    uint8_t* dout = h.out(overlay, n * 3);
    uint8_t* dw = h.out(written, batch);
    CHK(h.staged());
    const mav_ctx::LastRender& r = c->last_render;
    CHK(mav_overlay_dev(c, df, r.mask_fixed, r.foe, dgt, batch, radius, dout, dw));
    return h.finish();
}

// ---- PNG files of device-resident images (include/mavflow.h: mav_png_encode) -------------------------------------------------------
static size_t png_raw(int W, int H, int channels) { return (size_t)H * ((size_t)W * channels + 1); }
extern "C" size_t mav_png_bound(int W, int H, int channels)
{
    if (W < 1 || H < 1 || (channels != 1 && channels != 3 && channels != 4)) return 0;
    const size_t raw = png_raw(W, H, channels);
    return raw + 5 * png_segments(raw) + 6;
}
static int check_png_args(mav_ctx* c, const char* fn, int count, int channels, size_t out_bytes, bool need_bound)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (channels != 1 && channels != 3 && channels != 4) return fail(MAV_ERR_ARG, "%s: channels %d is none of 1 (gray), 3 (BGR), 4 (BGRA)", fn, channels);
    if (count < 1) return fail(MAV_ERR_ARG, "%s: count %d < 1", fn, count);
    if ((size_t)c->W * channels >= ((size_t)1 << 31) - 1) return fail(MAV_ERR_ARG, "%s: a row of %d x %d bytes is too long", fn, c->W, channels);
    const size_t bound = mav_png_bound(c->W, c->H, channels);
    if (need_bound && out_bytes / bound < (size_t)count)
        return fail(MAV_ERR_ARG, "%s: out_bytes %zu < count x mav_png_bound = %d x %zu", fn, out_bytes, count, bound);
    return MAV_OK;
}
// The encoder's workspace holds the segments of one CHUNK of images (at most kPngChunkBytes, one image at least): a call of many
// images runs the launch chain once per chunk, every chunk packing its streams behind the previous one's.
static const size_t kPngChunkBytes = (size_t)256 << 20;
extern "C" int mav_png_encode_dev(mav_ctx* c, const uint8_t* imgs, int count, int channels, uint8_t* out, size_t out_bytes, uint64_t* index)
{
    CHK(check_png_args(c, "mav_png_encode_dev", count, channels, out_bytes, true));
    if (!imgs || !out || !index) return fail(MAV_ERR_ARG, "mav_png_encode_dev: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t per = (png_workspace_per_image(png_raw(c->W, c->H, channels)) + 15) & ~(size_t)15;
    size_t chunk = kPngChunkBytes / per;
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)count) chunk = count;
    if (chunk > 65535) chunk = 65535;
    CHK(grow_buffer(c, &c->png_ws, &c->png_ws_cap, chunk * per, MEM_OTHER, READ_ON_COMPUTE, RELEASE_FIRST, "PNG encoder workspace"));
    ProfScope ps(c, K_MISC);
    for (int i0 = 0; i0 < count; i0 += (int)chunk) {
        const int n = count - i0 < (int)chunk ? count - i0 : (int)chunk;
        launch_png_encode(c->stream, imgs, i0, n, c->W, c->H, channels, c->png_ws, out, (unsigned long long*)index);
    }
    return check_launch("png_encode");
}
// The tail of the PNG calls: the index -> host and the stream drained, so that the host knows how long the streams (packed from offset
// 0) of the `count` encoded images are; then those.
static int download_png(HostCall& h, int count, const uint8_t* dout, const uint64_t* didx, uint8_t* out_host, size_t out_bytes, uint64_t* index)
{
    h.fetch(index, didx, sizeof(uint64_t) * 2 * count);
    CHK(h.finish());
    const size_t total = (size_t)(index[2 * (count - 1)] + index[2 * (count - 1) + 1]);
    if (total > out_bytes) return fail(MAV_ERR_ARG, "%s: out_bytes %zu, the %d streams take %zu", h.fn, out_bytes, count, total);
    h.fetch(out_host, dout, total);
    return h.finish();
}
extern "C" int mav_png_encode(mav_ctx* c, const uint8_t* imgs, int count, int channels, uint8_t* out_host, size_t out_bytes, uint64_t* index)
{
    CHK(check_png_args(c, "mav_png_encode", count, channels, out_bytes, false));
    if (!imgs || !out_host || !index) return fail(MAV_ERR_ARG, "mav_png_encode: NULL argument");
    HostCall h(c, "mav_png_encode");
    CHK(h.fresh());
    const size_t bound = mav_png_bound(c->W, c->H, channels) * count;
    const uint8_t* di = h.in(imgs, c->n0 * channels * count);
    uint8_t* dout = h.scratch<uint8_t>(bound);
    uint64_t* didx = h.scratch<uint64_t>(sizeof(uint64_t) * 2 * count);
    CHK(h.staged());
    CHK(mav_png_encode_dev(c, di, count, channels, dout, bound, didx));
    return download_png(h, count, dout, didx, out_host, out_bytes, index);
}

extern "C" int mav_last_render_png(mav_ctx* c, int batch, int want_result, int want_flow, int want_phi, uint8_t* out_host, size_t out_bytes,
                                   uint64_t* index)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_last_render_png: NULL context");
    if (!c->last_render.batch || batch != c->last_render.batch)
        return fail(MAV_ERR_STATE, "mav_last_render_png: no flow of a %d-pair detection call is resident", batch);
    HostCall h(c, "mav_last_render_png");
    CHK(h.after_last());
    const int want[3] = {want_result != 0, want_flow != 0, want_phi != 0}, nimg = want[0] + want[1] + want[2];
    if (!nimg) return MAV_OK;
    if (!out_host || !index) return fail(MAV_ERR_ARG, "mav_last_render_png: NULL argument");
    const size_t per = c->n0 * 3 * batch, bound = mav_png_bound(c->W, c->H, 3) * nimg * batch;
    uint8_t* dimg = h.scratch<uint8_t>(per * nimg);
    uint8_t* dout = h.scratch<uint8_t>(bound);
    uint64_t* didx = h.scratch<uint64_t>(sizeof(uint64_t) * 2 * nimg * batch);
    CHK(h.staged());
    uint8_t* dev[3] = {nullptr, nullptr, nullptr};
    for (int k = 0, j = 0; k < 3; k++)
        if (want[k]) dev[k] = dimg + per * j++;
    const mav_ctx::LastRender& r = c->last_render;
    CHK(render_enqueue(c, r.flow, r.derot, r.foe, r.sky, batch, r.thr, dev[0], dev[1], dev[2]));
    CHK(mav_png_encode_dev(c, dimg, nimg * batch, 3, dout, bound, didx));
    return download_png(h, nimg * batch, dout, didx, out_host, out_bytes, index);
}

extern "C" int mav_last_overlay_png(mav_ctx* c, const uint8_t* frames, const double* foe_gt, int batch, int radius, uint8_t* out_host,
                                    size_t out_bytes, uint64_t* index, uint8_t* written)
{
    if (!c || !frames || !foe_gt || !out_host || !index || !written) return fail(MAV_ERR_ARG, "mav_last_overlay_png: NULL argument");
    CHK(check_dev_call(c, batch, "mav_last_overlay_png"));
    if (!c->last_render.batch || batch != c->last_render.batch || !c->last_render.mask_fixed)
        return fail(MAV_ERR_STATE, "mav_last_overlay_png: no fixed mask of a %d-pair detection call is resident", batch);
    CHK(check_radius(radius, "mav_last_overlay_png"));
    CHK(check_foe_host(foe_gt, batch, "foe_gt", "mav_last_overlay_png"));
    HostCall h(c, "mav_last_overlay_png");
    CHK(h.after_last());
    const size_t n = c->n0 * batch, bound = mav_png_bound(c->W, c->H, 3) * batch;
    const uint8_t* df = h.in(frames, n * 3);
    const double* dgt = h.in(foe_gt, sizeof(double) * 2 * batch);
    uint8_t* dimg = h.scratch<uint8_t>(n * 3);
    uint8_t* dw = h.out(written, batch);
    uint8_t* dout = h.scratch<uint8_t>(bound);
    uint64_t* didx = h.scratch<uint64_t>(sizeof(uint64_t) * 2 * batch);
    CHK(h.staged());
    const mav_ctx::LastRender& r = c->last_render;
    CHK(mav_overlay_dev(c, df, r.mask_fixed, r.foe, dgt, batch, radius, dimg, dw));
    CHK(mav_png_encode_dev(c, dimg, batch, 3, dout, bound, didx));
    return download_png(h, batch, dout, didx, out_host, out_bytes, index);
}

extern "C" int mav_process_batch(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const uint32_t* samples, const double* omega,
                                 const double* dt, const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params* fp,
                                 const mav_thr_params* tp, float* flow, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                                 mav_result* results)
{
    ProcessArgs a;
    a.prev = prev; a.next = next; a.samples = samples; a.omega = omega; a.dt = dt; a.frame0 = frame0; a.sky = sky; a.foe_par = fp; a.thr = tp;
    a.flow_out = flow; a.phi = phi; a.mask_fixed = mask_fixed; a.mask_dyn = mask_dyn; a.results = results;
    return process_host(c, "mav_process_batch", batch, a);
}

extern "C" int mav_detect(mav_ctx* c, const float* flow, const uint32_t* samples, const double* omega, const double* dt,
                          const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params* fp, const mav_thr_params* tp,
                          double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results)
{
    if (!flow) return fail(MAV_ERR_ARG, "mav_detect: NULL flow");
    ProcessArgs a;
    a.flow_in = flow; a.samples = samples; a.omega = omega; a.dt = dt; a.frame0 = frame0; a.sky = sky; a.foe_par = fp; a.thr = tp;
    a.phi = phi; a.mask_fixed = mask_fixed; a.mask_dyn = mask_dyn; a.results = results;
    return process_host(c, "mav_detect", batch, a);
}

// ---- stage hooks -------------------------------------------------------------------------------------------------
extern "C" int mav_stage_phi_mask(mav_ctx* c, const float* flow, const double* foe, const double* omega, const double* dt,
                                  const uint8_t* sky, int batch, const mav_thr_params* tp, double* phi, uint8_t* mask_fixed,
                                  uint8_t* mask_dyn, int32_t* box)
{
    HostCall h(c, "mav_stage_phi_mask");
    CHK(h.fresh(batch));
    if (!flow || !foe) return fail(MAV_ERR_ARG, "mav_stage_phi_mask: NULL argument");
    const size_t n = c->n0 * batch;
    const mav_thr_params t = thr_or_defaults(tp);
    DetectArgs a;
    a.flow32 = h.in(flow, n * 2 * sizeof(float));
    a.foe_in = h.in(foe, sizeof(double) * 2 * batch);
    a.sky = h.in(sky, n);
    a.phi = h.out(phi, n * sizeof(double));
    a.mask_fixed = h.out(mask_fixed, n);
    a.mask_dyn = h.out(mask_dyn, n);
    a.box_out = h.out(box, sizeof(int32_t) * 4 * batch);
    a.thr = &t;
    CHK(h.staged());
    CHK(upload_derot(c, omega, dt, nullptr, batch, true, &a.derot));
    CHK(detect_dev(c, batch, a));
    return h.finish();
}

extern "C" int mav_stage_coefficients(mav_ctx* c, int k, float* g, float* xg, float* xxg, float* ig, float* blur_taps)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_stage_coefficients: NULL context");
    const int n = c->pc.n;
    for (int i = 0; i <= n; i++) {
        if (g) g[i] = c->pc.g[i];
        if (xg) xg[i] = c->pc.xg[i];
        if (xxg) xxg[i] = c->pc.xxg[i];
    }
    if (ig) { ig[0] = c->pc.ig11; ig[1] = c->pc.ig03; ig[2] = c->pc.ig33; ig[3] = c->pc.ig55; }
    if (blur_taps) {
        HostCall h(c, "mav_stage_coefficients");
        const Layer* l;
        CHK(h.fresh_layer(k, &l));
        HIPCHK(hipMemcpy(blur_taps, l->g, sizeof(float) * l->ksize, hipMemcpyDeviceToHost));   // what the kernels actually read
    }
    return MAV_OK;
}

static int stage_blur_resize(mav_ctx* c, const void* img, int depth, int k, bool two_pass, float* out)
{
    if (c && !depth_esize(depth)) return fail(MAV_ERR_ARG, "mav_stage_blur_resize_ex: depth %d is none of MAV_DEPTH_8U / 16U / 32F", depth);
    HostCall h(c, "mav_stage_blur_resize");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!img || !out) return fail(MAV_ERR_ARG, "mav_stage_blur_resize: NULL argument");
    const size_t n = (size_t)l->w * l->h;
    // the two-pass form's H x w scratch (one frame: 4 bytes per pixel) is a staging block of this call: a diagnostic hook never
    // allocates the Farneback workspace (GBs at 1080p / 4K) nor freezes "deep_frac"
    const void* di = h.in(img, c->n0 * depth_esize(depth));
    float* dout = h.out(out, n * sizeof(float));
    float* dtmp = h.scratch<float>(c->htmp_stride * sizeof(float));
    CHK(h.staged());
    with_depth(depth, [&](auto* px) {
        typedef std::remove_const_t<std::remove_pointer_t<decltype(px)>> T;
        launch_blur_resize(c->stream, FrameRun<T>{(const T*)di, nullptr, 0, c->n0, 1, c->W, c->H}, {dout, n, blur_of(c, *l), l->w, l->h},
                           {dtmp, c->htmp_stride, two_pass});
    });
    CHK(check_launch("blur_resize"));
    return h.finish();
}
extern "C" int mav_stage_blur_resize(mav_ctx* c, const uint8_t* img, int k, float* out) { return stage_blur_resize(c, img, MAV_DEPTH_8U, k, false, out); }
extern "C" int mav_stage_blur_resize_two_pass(mav_ctx* c, const uint8_t* img, int k, float* out) { return stage_blur_resize(c, img, MAV_DEPTH_8U, k, true, out); }
extern "C" int mav_stage_blur_resize_ex(mav_ctx* c, const void* img, int depth, int k, int two_pass, float* out)
{
    return stage_blur_resize(c, img, depth, k, two_pass != 0, out);
}
extern "C" int mav_stage_polyexp(mav_ctx* c, const float* I, int k, float* R)
{
    HostCall h(c, "mav_stage_polyexp");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!I || !R) return fail(MAV_ERR_ARG, "mav_stage_polyexp: NULL argument");
    const size_t n = (size_t)l->w * l->h;
    const float* di = h.in(I, n * sizeof(float));
    std::vector<float> e(5 * n); float* dr = h.out(e.data(), 5 * n * sizeof(float));      // (h, w, 5), as the kernel writes it
    CHK(h.staged());
    launch_polyexp(c->stream, di, n, 1, l->w, l->h, c->pc, dr, 5 * n);
    CHK(check_launch("polyexp"));
    return planes_of_expansion(h.finish(), e, n, R);      // R takes its planes
}
extern "C" int mav_stage_update_matrices(mav_ctx* c, const float* R0, const float* R1, const float* flow, int k, float* M)
{
    HostCall h(c, "mav_stage_update_matrices");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!R0 || !R1 || !flow || !M) return fail(MAV_ERR_ARG, "mav_stage_update_matrices: NULL argument");
    const size_t n = (size_t)l->w * l->h;
    const std::vector<float> e0 = expansion_of_planes(R0, n), e1 = expansion_of_planes(R1, n);      // the caller's planes as (h, w, 5)
    const float *d0 = h.in(e0.data(), 5 * n * sizeof(float)), *d1 = h.in(e1.data(), 5 * n * sizeof(float));
    const float* df = h.in(flow, 2 * n * sizeof(float));
    float* dm = h.out(M, 5 * n * sizeof(float));
    CHK(h.staged());
    launch_initial_m(c->stream, {{d0, d1, 5 * n, 1, l->w, l->h}, dm, 5 * n}, FlowSource::field(df, 2 * n));
    CHK(check_launch("update_matrices"));
    return h.finish();
}
// The initial M as layer_sweeps builds it for layer k: from the coarser layer's flow (layer k + 1's size, upsampled and times
// 1 / pyr_scale inside the kernel) or, flow_coarse == NULL, from a zero flow.
extern "C" int mav_stage_update_matrices_from(mav_ctx* c, const float* R0, const float* R1, const float* flow_coarse, int k, float* M)
{
    HostCall h(c, "mav_stage_update_matrices_from");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!R0 || !R1 || !M) return fail(MAV_ERR_ARG, "mav_stage_update_matrices_from: NULL argument");
    if (flow_coarse && k + 1 >= (int)c->layers.size())
        return fail(MAV_ERR_ARG, "mav_stage_update_matrices_from: layer %d is the top layer, it has no coarser flow", k);
    const size_t n = (size_t)l->w * l->h;
    const size_t nc = flow_coarse ? (size_t)c->layers[k + 1].w * c->layers[k + 1].h : 0;
    const std::vector<float> e0 = expansion_of_planes(R0, n), e1 = expansion_of_planes(R1, n);      // the caller's planes as (h, w, 5)
    const float *d0 = h.in(e0.data(), 5 * n * sizeof(float)), *d1 = h.in(e1.data(), 5 * n * sizeof(float));
    const float* df = h.in(flow_coarse, 2 * nc * sizeof(float));
    float* dm = h.out(M, 5 * n * sizeof(float));
    CHK(h.staged());
    launch_initial_m(c->stream, {{d0, d1, 5 * n, 1, l->w, l->h}, dm, 5 * n}, flow_coarse ? coarser_flow(c, k + 1, df, 2 * nc) : FlowSource{});
    CHK(check_launch("update_matrices"));
    return h.finish();
}
// The initial flow of layer k from a frame-size field as snapshot_initial_flow computes it for the top layer: INTER_AREA resize,
// then times pyr_scale^k (the repeated product).
extern "C" int mav_stage_initial_flow(mav_ctx* c, const float* flow0, int k, float* out)
{
    HostCall h(c, "mav_stage_initial_flow");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!flow0 || !out) return fail(MAV_ERR_ARG, "mav_stage_initial_flow: NULL argument");
    const size_t n = (size_t)l->w * l->h;
    double scale = 1;
    for (int i = 0; i < k; i++) scale *= c->fb.pyr_scale;
    const float* di = h.in(flow0, 2 * c->n0 * sizeof(float));
    float* dout = h.out(out, 2 * n * sizeof(float));
    CHK(h.staged());
    launch_area_resize_flow(c->stream, di, 2 * c->n0, c->W, c->H, dout, 2 * n, l->w, l->h, 1, scale);
    CHK(check_launch("area_resize_flow"));
    return h.finish();
}
extern "C" int mav_stage_blur_iter(mav_ctx* c, const float* R0, const float* R1, const float* M, int k, int update, float* flow, float* M_out)
{
    HostCall h(c, "mav_stage_blur_iter");
    const Layer* l;
    CHK(h.fresh_layer(k, &l));
    if (!R0 || !R1 || !M || !flow || (update && !M_out)) return fail(MAV_ERR_ARG, "mav_stage_blur_iter: NULL argument");
    const size_t n = (size_t)l->w * l->h;
    const std::vector<float> e0 = expansion_of_planes(R0, n), e1 = expansion_of_planes(R1, n);      // the caller's planes as (h, w, 5)
    const float *d0 = h.in(e0.data(), 5 * n * sizeof(float)), *d1 = h.in(e1.data(), 5 * n * sizeof(float));
    const float* dm = h.in(M, 5 * n * sizeof(float));
    float* dmo = h.scratch<float>(5 * n * sizeof(float));
    float* df = h.out(flow, 2 * n * sizeof(float));
    h.fetch(update ? M_out : nullptr, dmo, 5 * n * sizeof(float));
    CHK(h.staged());
    SweepArgs a{{d0, d1, 5 * n, 1, l->w, l->h}, dm, dmo, 5 * n, c->fb.winsize, df, 2 * n, update, 1};
    a.strip = c->strip; a.gauss = window_taps(c);
    launch_blur_iter(c->stream, a);
    CHK(check_launch("blur_iter"));
    return h.finish();
}

// ---- RCCL (loaded lazily so the single-GPU path carries no collective library) ----------------------------------------
typedef int (*nccl_get_uid_t)(void*);
struct uid128 { char b[128]; };  // ncclUniqueId is passed by value: 128 bytes
typedef int (*nccl_init_rank2_t)(void**, int, uid128, int);
typedef int (*nccl_destroy_t)(void*);
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef const char* (*nccl_errstr_t)(int);
static void* g_rccl = nullptr;
static int rccl_sym(const char* name, void** fn)
{
    if (!g_rccl) {
        g_rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!g_rccl) g_rccl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!g_rccl) return fail(MAV_ERR_STATE, "cannot load RCCL: %s", dlerror());
    }
    *fn = dlsym(g_rccl, name);
    if (!*fn) return fail(MAV_ERR_STATE, "RCCL symbol %s missing", name);
    return MAV_OK;
}
// Versions at the seam where this library meets a runtime somebody else loaded: in the multi-GPU bench torch has already mapped its
// own HIP runtime and RCCL (same SONAMEs), so libmavflow -- built by this tree's hipcc -- binds to those.
typedef int (*nccl_get_version_t)(int*);
extern "C" int mav_runtime_info(char* buf, size_t cap)
{
    if (!buf || cap < 16) return fail(MAV_ERR_ARG, "mav_runtime_info: NULL argument");
    int rt = 0, drv = 0, nccl = 0;
    if (hipRuntimeGetVersion(&rt) != hipSuccess) rt = -1;
    if (hipDriverGetVersion(&drv) != hipSuccess) drv = -1;
    void* fn = nullptr;
    if (g_rccl && (fn = dlsym(g_rccl, "ncclGetVersion"))) ((nccl_get_version_t)fn)(&nccl);
    snprintf(buf, cap, "{\"built_with_hip\": \"%d.%d.%d\", \"hip_runtime\": %d, \"hip_runtime_major\": %d, \"hip_driver\": %d, \"rccl\": %d}",
             HIP_VERSION_MAJOR, HIP_VERSION_MINOR, HIP_VERSION_PATCH, rt, rt > 0 ? rt / 10000000 : -1, drv, nccl);
    return MAV_OK;
}
extern "C" int mav_comm_unique_id(void* id128)
{
    if (!id128) return fail(MAV_ERR_ARG, "mav_comm_unique_id: NULL");
    void* fn;
    CHK(rccl_sym("ncclGetUniqueId", &fn));
    int rc = ((nccl_get_uid_t)fn)(id128);
    return rc ? fail(MAV_ERR_HIP, "ncclGetUniqueId failed: %d", rc) : MAV_OK;
}
extern "C" int mav_comm_init(mav_ctx* c, const void* id128, int rank, int nranks, void** comm_out)
{
    if (!c || !id128 || !comm_out) return fail(MAV_ERR_ARG, "mav_comm_init: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    // the collective runs on this context's stream inside whatever HIP runtime the process loaded first: refuse a runtime of another
    // major version than the one the kernels' host code was compiled against (launch ABI, stream handles) instead of finding out later
    int rt = 0;
    HIPCHK(hipRuntimeGetVersion(&rt));
    if (rt / 10000000 != HIP_VERSION_MAJOR)
        return fail(MAV_ERR_STATE, "mav_comm_init: libmavflow was built with HIP %d.%d but the process runs HIP runtime %d (major %d): rebuild against "
                    "the runtime the launcher loads", HIP_VERSION_MAJOR, HIP_VERSION_MINOR, rt, rt / 10000000);
    void* fn;
    CHK(rccl_sym("ncclCommInitRank", &fn));
    uid128 id;
    memcpy(&id, id128, sizeof(id));
    int rc = ((nccl_init_rank2_t)fn)(comm_out, nranks, id, rank);
    return rc ? fail(MAV_ERR_HIP, "ncclCommInitRank failed: %d", rc) : MAV_OK;
}
typedef int (*nccl_comm_count_t)(void*, int*);
extern "C" int mav_comm_count(void* comm, int* nranks)
{
    if (!comm || !nranks) return fail(MAV_ERR_ARG, "mav_comm_count: NULL argument");
    void* fn;
    CHK(rccl_sym("ncclCommCount", &fn));
    int rc = ((nccl_comm_count_t)fn)(comm, nranks);
    return rc ? fail(MAV_ERR_HIP, "ncclCommCount failed: %d", rc) : MAV_OK;
}
extern "C" int mav_comm_destroy(void* comm)
{
    if (!comm) return MAV_OK;
    void* fn;
    CHK(rccl_sym("ncclCommDestroy", &fn));
    ((nccl_destroy_t)fn)(comm);
    return MAV_OK;
}
extern "C" int mav_allgather_results(mav_ctx* c, void* comm, const void* local_dev, size_t bytes_per_rank, void* all_dev)
{
    if (!c || !comm || !local_dev || !all_dev) return fail(MAV_ERR_ARG, "mav_allgather_results: NULL argument");
    void* fn;
    CHK(rccl_sym("ncclAllGather", &fn));
    int rc = ((nccl_allgather_t)fn)(local_dev, all_dev, bytes_per_rank, /* ncclInt8 */ 0, comm, c->stream);
    return rc ? fail(MAV_ERR_HIP, "ncclAllGather failed: %d", rc) : MAV_OK;
}

// ---- sparse optical flow: Shi-Tomasi corners + pyramidal Lucas-Kanade (kernels_lk.hip) ---------------------------------------------
extern "C" void mav_gftt_defaults(mav_gftt_params* p) { *p = mav_gftt_params{2000, 0.2, 7.0, 7}; }
extern "C" void mav_lk_defaults(mav_lk_params* p) { *p = mav_lk_params{21, 21, 3, 30, 0.01, 1e-4}; }
extern "C" void mav_corner_score_defaults(mav_corner_score* s) { *s = mav_corner_score{0, 0.04}; }

static void lk_level_dims(int W, int H, LkLevels* lv)
{
    size_t off = 0;
    int w = W, h = H;
    lv->n = 0;
    for (int l = 0; l <= MAV_LK_MAX_LEVEL; l++) {
        lv->w[l] = w; lv->h[l] = h; lv->off[l] = (unsigned)off;
        lv->n = l + 1;
        off += ((size_t)w * h + 63) & ~(size_t)63;
        if (w == 1 && h == 1) break;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    for (int l = lv->n; l < MAV_LK_MAX_LEVELS; l++) { lv->w[l] = lv->h[l] = 0; lv->off[l] = 0; }
}
extern "C" int mav_lk_level_dims(const mav_ctx* c, int level, int* w, int* h)
{
    if (!c) return fail(MAV_ERR_ARG, "mav_lk_level_dims: NULL context");
    LkLevels lv;
    lk_level_dims(c->W, c->H, &lv);
    if (level < 0 || level >= lv.n) return fail(MAV_ERR_ARG, "mav_lk_level_dims: level %d outside [0, %d]", level, lv.n - 1);
    if (w) *w = lv.w[level]; if (h) *h = lv.h[level];
    return MAV_OK;
}

// Argument checks that need no device (and no context): refused before anything is touched.
static int check_gftt_params(const mav_gftt_params& p, const char* fn)
{
    if (p.max_corners < 1 || p.max_corners > MAV_LK_MAX_POINTS)
        return fail(MAV_ERR_ARG, "%s: max_corners %d outside [1, %d]", fn, p.max_corners, MAV_LK_MAX_POINTS);
    if (!(p.quality_level > 0) || !std::isfinite(p.quality_level)) return fail(MAV_ERR_ARG, "%s: quality_level %g must be positive", fn, p.quality_level);
    if (!(p.min_distance >= 0) || !std::isfinite(p.min_distance)) return fail(MAV_ERR_ARG, "%s: min_distance %g must be >= 0", fn, p.min_distance);
    if (p.block_size < 1 || p.block_size > 15 || p.block_size % 2 == 0)
        return fail(MAV_ERR_ARG, "%s: block_size %d must be odd and in [1, 15] (the tile's halo in LDS)", fn, p.block_size);
    return MAV_OK;
}
static int check_corner_score(const mav_corner_score* sp, mav_corner_score* s, const char* fn)
{
    if (sp) *s = *sp; else mav_corner_score_defaults(s);
    if (!std::isfinite(s->k)) return fail(MAV_ERR_ARG, "%s: k %g must be finite", fn, s->k);
    return MAV_OK;
}
static int check_lk_params(mav_lk_params& p, int n, const char* fn)
{
    if (p.win_w < 3 || p.win_h < 3 || p.win_w % 2 == 0 || p.win_h % 2 == 0)
        return fail(MAV_ERR_ARG, "%s: window %d x %d must be odd and at least 3 x 3", fn, p.win_w, p.win_h);
    if (p.win_w > MAV_LK_MAX_WIN || p.win_h > MAV_LK_MAX_WIN)
        return fail(MAV_ERR_ARG, "%s: window %d x %d exceeds %d x %d (a point's window lives in LDS, four points per workgroup)", fn, p.win_w, p.win_h,
                    MAV_LK_MAX_WIN, MAV_LK_MAX_WIN);
    if (p.max_level < 0 || p.max_level > MAV_LK_MAX_LEVEL) return fail(MAV_ERR_ARG, "%s: max_level %d outside [0, %d]", fn, p.max_level, MAV_LK_MAX_LEVEL);
    if (n < 0 || n > MAV_LK_MAX_POINTS) return fail(MAV_ERR_ARG, "%s: %d points outside [0, %d]", fn, n, MAV_LK_MAX_POINTS);
    if (std::isnan(p.epsilon) || std::isnan(p.min_eig_threshold)) return fail(MAV_ERR_ARG, "%s: epsilon / min_eig_threshold is NaN", fn);
    p.max_count = std::min(std::max(p.max_count, 0), 100);            // cv2's own clamps of the termination criteria
    p.epsilon = std::min(std::max(p.epsilon, 0.), 10.);
    return MAV_OK;
}

static int ensure_lk(mav_ctx* c)
{
    LkState& k = c->lk;
    if (k.status) return MAV_OK;                  // (all or nothing: any one of the set tells)
    lk_level_dims(c->W, c->H, &k.dims);
    k.pyr_elems = (size_t)k.dims.off[k.dims.n - 1] + (((size_t)k.dims.w[k.dims.n - 1] * k.dims.h[k.dims.n - 1] + 63) & ~(size_t)63);
    const size_t pts = (size_t)MAV_LK_MAX_POINTS * 2 * sizeof(float);
    // the pick's grid at its largest: cells of 1 (1 slot), 2 (2 slots) or 3 pixels (4 slots); W * H unless the frame is one pixel wide
    const size_t W = c->W, H = c->H;
    k.eig_words = std::max({c->n0, 2 * ((W + 1) / 2) * ((H + 1) / 2), 4 * ((W + 2) / 3) * ((H + 2) / 3)});
    CHK(c->mem.alloc_set({{&k.pyr[0], k.pyr_elems}, {&k.pyr[1], k.pyr_elems}, {&k.deriv, k.pyr_elems * sizeof(short2)}, {&k.eig, k.eig_words * sizeof(float)},
                          {&k.cand, (size_t)MAV_GFTT_MAX_CANDIDATES * sizeof(uint2)}, {&k.counters, LK_CNT_N * sizeof(unsigned)},
                          {&k.pts, pts}, {&k.out, pts}, {&k.status, (size_t)MAV_LK_MAX_POINTS}}, MEM_OTHER, "sparse optical flow workspace"));
    return MAV_OK;
}

// levels in use for a window: building stops before the first level whose width <= win_w or height <= win_h
static int lk_levels_for(const LkState& k, const mav_lk_params& p)
{
    int n = 1;
    while (n <= p.max_level && n < k.dims.n && k.dims.w[n] > p.win_w && k.dims.h[n] > p.win_h) n++;
    return n;
}
// a frame into a slot: level 0 only; the coarser levels come with lk_build
static int lk_load(mav_ctx* c, int slot, const uint8_t* img, bool host)
{
    LkState& k = c->lk;
    HIPCHK(hipMemcpyAsync(k.pyr[slot], img, c->n0, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    k.built[slot] = 1;
    if (k.deriv_slot == slot) { k.deriv_slot = -1; k.deriv_levels = 0; }
    return MAV_OK;
}
static void lk_build(mav_ctx* c, int slot, int levels)
{
    LkState& k = c->lk;
    if (k.built[slot] >= levels) return;
    ProfScope ps(c, K_LK_PYRAMID);
    for (int l = k.built[slot]; l < levels; l++)
        launch_lk_pyrdown(c->stream, k.pyr[slot] + k.dims.off[l - 1], k.dims.w[l - 1], k.dims.h[l - 1], k.pyr[slot] + k.dims.off[l], k.dims.w[l], k.dims.h[l]);
    k.built[slot] = levels;
}
static void lk_derivatives(mav_ctx* c, int slot, int levels)
{
    LkState& k = c->lk;
    if (k.deriv_slot == slot && k.deriv_levels >= levels) return;
    ProfScope ps(c, K_LK_PYRAMID);
    launch_lk_scharr(c->stream, k.pyr[slot], k.dims, levels, k.deriv);
    k.deriv_slot = slot; k.deriv_levels = levels;
}

// The sort and the pick of cand[0 .. counters[1]) into corners / count (device memory), enqueue only.
static int corner_pick_enqueue(mav_ctx* c, const mav_gftt_params& p, float* corners, int* count)
{
    LkState& k = c->lk;
    LkPickArgs a;
    a.cand = k.cand; a.n_ptr = k.counters + 1; a.cap = MAV_GFTT_MAX_CANDIDATES;
    a.W = c->W; a.max_corners = p.max_corners;
    a.pick = p.min_distance >= 1;
    // cells of ceil(min_distance) pixels, as many as the frame needs; one cell when min_distance exceeds the frame
    const double cd = std::min(ceil(p.min_distance), (double)std::max(c->W, c->H));
    a.cell = a.pick ? (int)cd : std::max(c->W, c->H);
    a.gw = (c->W + a.cell - 1) / a.cell; a.gh = (c->H + a.cell - 1) / a.cell;
    a.slots = a.cell == 1 ? 1 : a.cell == 2 ? 2 : 4;
    a.md2 = p.min_distance * p.min_distance;
    a.grid = reinterpret_cast<unsigned*>(k.eig);
    a.corners = corners; a.count = count; a.stats = k.counters + LK_CNT_STATS;
    const size_t words = (size_t)a.gw * a.gh * a.slots;
    if (words > k.eig_words) return fail(MAV_ERR_STATE, "corner pick: a grid of %zu words in a buffer of %zu", words, k.eig_words);
    ProfScope ps(c, K_LK_PICK);
    if (a.pick) HIPCHK(hipMemsetAsync(a.grid, 0, words * sizeof(unsigned), c->stream));
    launch_pick_sort(c->stream, k.cand, a.n_ptr, a.cap);
    launch_corner_pick(c->stream, a);
    return check_launch("corner pick");
}
// The score map of slot `slot` into k.eig and its (masked) maximum into counters[0]: min-eigenvalue, or the Harris response.
static void corner_map_enqueue(mav_ctx* c, int slot, const uint8_t* mask, int block_size, const mav_corner_score& sc)
{
    LkState& k = c->lk;
    const float s = (float)(1.0 / (4.0 * block_size * 255.0)), s2 = s * s;
    if (sc.use_harris) launch_harris(c->stream, k.pyr[slot], mask, c->W, c->H, block_size, s2, (float)sc.k, k.eig, k.counters);
    else launch_min_eig(c->stream, k.pyr[slot], mask, c->W, c->H, block_size, s2, k.eig, k.counters);
}
// Corner detection on slot `slot`, enqueue only: score map, candidates, sort, pick.  mask / corners / count: device memory.
static int good_features_enqueue(mav_ctx* c, int slot, const uint8_t* mask, const mav_gftt_params& p, const mav_corner_score& sc, float* corners,
                                 int* count)
{
    LkState& k = c->lk;
    const int W = c->W, H = c->H;
    {
        ProfScope ps(c, K_LK_CORNERS);
        HIPCHK(hipMemsetAsync(k.counters, 0, 2 * sizeof(unsigned), c->stream));
        corner_map_enqueue(c, slot, mask, p.block_size, sc);
        launch_corner_candidates(c->stream, k.eig, mask, W, H, k.counters, p.quality_level, k.cand, k.counters + 1, MAV_GFTT_MAX_CANDIDATES);
    }
    CHK(check_launch("corner detection"));
    return corner_pick_enqueue(c, p, corners, count);
}
// The host forms' end: the count and count x 8 bytes come back; one synchronisation.  A negative count is an overflow.
static int corner_pick_fetch(mav_ctx* c, const mav_gftt_params& p, float* corners, int* count, const char* fn)
{
    LkState& k = c->lk;
    // the count and the corners in one stream-ordered pair of copies: the corners' size is max_corners, known to the host
    std::vector<float>& buf = k.fetch;
    if (buf.size() < (size_t)p.max_corners * 2) buf.resize((size_t)p.max_corners * 2);
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, k.counters + LK_CNT_PICKED, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(buf.data(), k.out, (size_t)p.max_corners * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n < 0)
        return fail(MAV_ERR_ARG, "%s: the frame has %u corner candidates, the buffer holds %d (raise quality_level)", fn, (unsigned)-(long long)n,
                    MAV_GFTT_MAX_CANDIDATES);
    memcpy(corners, buf.data(), (size_t)n * 2 * sizeof(float));
    *count = n;
    return MAV_OK;
}
static int good_features_entry(mav_ctx* c, const uint8_t* gray, const uint8_t* mask, bool host, bool host_out, const mav_gftt_params* pp,
                               float* corners, int* count, const char* fn, const mav_corner_score* scp = nullptr)
{
    mav_gftt_params p;
    mav_corner_score sc;
    if (pp) p = *pp; else mav_gftt_defaults(&p);
    CHK(check_gftt_params(p, fn));
    CHK(check_corner_score(scp, &sc, fn));
    if (!c || !corners || !count) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    HIPCHK(hipSetDevice(c->device));
    if (!gray && c->lk.cur < 0) return fail(MAV_ERR_STATE, "%s: gray is NULL and no frame is resident", fn);
    CHK(ensure_lk(c));
    LkState& k = c->lk;
    if (gray) {
        const int slot = k.cur < 0 ? 0 : k.cur;          // replaces the resident frame
        CHK(lk_load(c, slot, gray, host));
        k.cur = slot;
    }
    if (mask && host) {
        // a host mask is staged in the other frame slot: no call reads that slot's frame again (a track call loads `next` into it)
        const int other = 1 - k.cur;
        HIPCHK(hipMemcpyAsync(k.pyr[other], mask, c->n0, hipMemcpyHostToDevice, c->stream));
        k.built[other] = 0;
        if (k.deriv_slot == other) { k.deriv_slot = -1; k.deriv_levels = 0; }
        mask = k.pyr[other];
    }
    if (!host_out) return good_features_enqueue(c, k.cur, mask, p, sc, corners, count);
    CHK(good_features_enqueue(c, k.cur, mask, p, sc, k.out, reinterpret_cast<int*>(k.counters + LK_CNT_PICKED)));
    return corner_pick_fetch(c, p, corners, count, fn);
}
extern "C" int mav_good_features(mav_ctx* c, const uint8_t* gray, const mav_gftt_params* p, float* corners, int* count)
{
    return good_features_entry(c, gray, nullptr, true, true, p, corners, count, "mav_good_features");
}
extern "C" int mav_good_features_dev(mav_ctx* c, const uint8_t* gray, const mav_gftt_params* p, float* corners, int* count)
{
    return good_features_entry(c, gray, nullptr, false, true, p, corners, count, "mav_good_features_dev");
}
extern "C" int mav_good_features_ex(mav_ctx* c, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params* p, float* corners, int* count)
{
    return good_features_entry(c, gray, mask, true, true, p, corners, count, "mav_good_features_ex");
}
extern "C" int mav_good_features_ex_dev(mav_ctx* c, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params* p, float* corners,
                                        int32_t* count)
{
    return good_features_entry(c, gray, mask, false, false, p, corners, count, "mav_good_features_ex_dev");
}
extern "C" int mav_good_features_score(mav_ctx* c, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params* p, const mav_corner_score* sc,
                                       float* corners, int* count)
{
    return good_features_entry(c, gray, mask, true, true, p, corners, count, "mav_good_features_score", sc);
}
extern "C" int mav_good_features_score_dev(mav_ctx* c, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params* p,
                                           const mav_corner_score* sc, float* corners, int32_t* count)
{
    return good_features_entry(c, gray, mask, false, false, p, corners, count, "mav_good_features_score_dev", sc);
}
extern "C" int mav_gftt_last_pick(mav_ctx* c, uint32_t* stats)
{
    if (!c || !stats) return fail(MAV_ERR_ARG, "mav_gftt_last_pick: NULL argument");
    if (!c->lk.counters) return fail(MAV_ERR_STATE, "mav_gftt_last_pick: no corner call precedes");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(stats, c->lk.counters + LK_CNT_STATS, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    return mav_sync(c);
}

// prev (or the resident frame) and next into the two slots, pyramids, derivatives, one tracker launch.  pts / out / status: device.
// ext: the tracker's second form (mav_lk_track_err*), with its flags and err (device, may be null).
struct LkErrOut { int flags; float* err; };
static int lk_track_enqueue(mav_ctx* c, const uint8_t* prev, const uint8_t* next, bool host, const float* pts, int n, const mav_lk_params& p,
                            float* out, uint8_t* status, const int* n_dev = nullptr, const LkErrOut* ext = nullptr)
{
    LkState& k = c->lk;
    int sp;
    if (prev) { sp = k.cur < 0 ? 0 : k.cur; CHK(lk_load(c, sp, prev, host)); }
    else sp = k.cur;
    const int sn = 1 - sp;
    k.cur = -1;                                           // until everything below has been enqueued
    CHK(lk_load(c, sn, next, host));
    const int levels = lk_levels_for(k, p);
    lk_build(c, sp, levels);
    lk_build(c, sn, levels);
    lk_derivatives(c, sp, levels);
    HIPCHK(hipMemsetAsync(k.counters + 2, 0, MAV_LK_HIST * sizeof(unsigned), c->stream));
    LkTrackErrArgs a{};
    a.I = k.pyr[sp]; a.J = k.pyr[sn]; a.D = k.deriv; a.lv = k.dims; a.lv.n = levels;
    a.pts = pts; a.n = n; a.win_w = p.win_w; a.win_h = p.win_h; a.max_count = p.max_count;
    a.eps2 = p.epsilon * p.epsilon; a.min_eig = (float)p.min_eig_threshold;
    a.out = out; a.status = status; a.iter_hist = k.counters + 2; a.n_dev = n_dev;
    {
        ProfScope ps(c, K_LK_TRACK);
        if (ext) { a.flags = ext->flags; a.err = ext->err; launch_lk_track_err(c->stream, a); }
        else launch_lk_track(c->stream, a);
    }
    CHK(check_launch("lk_track"));
    k.cur = sn; k.hist_valid = true;
    return MAV_OK;
}
static int lk_track_check(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const void* pts, int n, const mav_lk_params* pp, const void* out,
                          const void* status, mav_lk_params* p, const char* fn)
{
    if (pp) *p = *pp; else mav_lk_defaults(p);
    CHK(check_lk_params(*p, n, fn));
    if (!c || !next || (n > 0 && (!pts || !out || !status))) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    HIPCHK(hipSetDevice(c->device));
    if (!prev && c->lk.cur < 0) return fail(MAV_ERR_STATE, "%s: prev is NULL and no frame is resident", fn);
    return ensure_lk(c);
}
extern "C" int mav_lk_track(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const float* pts, int n, const mav_lk_params* pp, float* next_pts,
                            uint8_t* status)
{
    mav_lk_params p;
    CHK(lk_track_check(c, prev, next, pts, n, pp, next_pts, status, &p, "mav_lk_track"));
    LkState& k = c->lk;
    if (n) HIPCHK(hipMemcpyAsync(k.pts, pts, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(lk_track_enqueue(c, prev, next, true, k.pts, n, p, k.out, k.status));
    if (n) {
        HIPCHK(hipMemcpyAsync(next_pts, k.out, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status, k.status, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    return mav_sync(c);
}
extern "C" int mav_lk_track_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const float* pts, int n, const mav_lk_params* pp,
                                float* next_pts, uint8_t* status)
{
    mav_lk_params p;
    CHK(lk_track_check(c, prev, next, pts, n, pp, next_pts, status, &p, "mav_lk_track_dev"));
    return lk_track_enqueue(c, prev, next, false, pts, n, p, next_pts, status);
}
extern "C" int mav_lk_track_ex_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const float* pts, int n_max, const int32_t* n_dev,
                                   const mav_lk_params* pp, float* next_pts, uint8_t* status)
{
    mav_lk_params p;
    CHK(lk_track_check(c, prev, next, pts, n_max, pp, next_pts, status, &p, "mav_lk_track_ex_dev"));
    if (!n_dev) return fail(MAV_ERR_ARG, "mav_lk_track_ex_dev: NULL argument");
    return lk_track_enqueue(c, prev, next, false, pts, n_max, p, next_pts, status, n_dev);
}
static int lk_err_flags_check(int flags, int n, const void* next_pts, const char* fn)
{
    if (flags & ~(MAV_OPTFLOW_USE_INITIAL_FLOW | MAV_OPTFLOW_LK_GET_MIN_EIGENVALS))
        return fail(MAV_ERR_ARG, "%s: flags %d: only MAV_OPTFLOW_USE_INITIAL_FLOW (4) and MAV_OPTFLOW_LK_GET_MIN_EIGENVALS (8) are known", fn, flags);
    if ((flags & MAV_OPTFLOW_USE_INITIAL_FLOW) && n > 0 && !next_pts)
        return fail(MAV_ERR_ARG, "%s: MAV_OPTFLOW_USE_INITIAL_FLOW needs the starting positions in next_pts", fn);
    return MAV_OK;
}
extern "C" int mav_lk_track_err(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const float* pts, int n, const mav_lk_params* pp, int flags,
                                float* next_pts, uint8_t* status, float* err)
{
    mav_lk_params p;
    CHK(lk_err_flags_check(flags, n, next_pts, "mav_lk_track_err"));
    CHK(lk_track_check(c, prev, next, pts, n, pp, next_pts, status, &p, "mav_lk_track_err"));
    LkState& k = c->lk;
    const size_t pb = (size_t)n * 2 * sizeof(float);
    // err is staged in the candidate buffer: dead once a pick has run, and every use is ordered on the one stream
    static_assert((size_t)MAV_GFTT_MAX_CANDIDATES * sizeof(uint2) >= (size_t)MAV_LK_MAX_POINTS * sizeof(float), "err staging");
    const LkErrOut ext{flags, err ? reinterpret_cast<float*>(k.cand) : nullptr};
    if (n) HIPCHK(hipMemcpyAsync(k.pts, pts, pb, hipMemcpyHostToDevice, c->stream));
    if (n && (flags & MAV_OPTFLOW_USE_INITIAL_FLOW)) HIPCHK(hipMemcpyAsync(k.out, next_pts, pb, hipMemcpyHostToDevice, c->stream));
    CHK(lk_track_enqueue(c, prev, next, true, k.pts, n, p, k.out, k.status, nullptr, &ext));
    if (n) {
        HIPCHK(hipMemcpyAsync(next_pts, k.out, pb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status, k.status, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (err) HIPCHK(hipMemcpyAsync(err, ext.err, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    return mav_sync(c);
}
extern "C" int mav_lk_track_err_dev(mav_ctx* c, const uint8_t* prev, const uint8_t* next, const float* pts, int n_max, const int32_t* n_dev,
                                    const mav_lk_params* pp, int flags, float* next_pts, uint8_t* status, float* err)
{
    mav_lk_params p;
    CHK(lk_err_flags_check(flags, n_max, next_pts, "mav_lk_track_err_dev"));
    CHK(lk_track_check(c, prev, next, pts, n_max, pp, next_pts, status, &p, "mav_lk_track_err_dev"));
    const LkErrOut ext{flags, err};
    return lk_track_enqueue(c, prev, next, false, pts, n_max, p, next_pts, status, n_dev, &ext);
}
extern "C" int mav_lk_last_iterations(mav_ctx* c, uint32_t* hist)
{
    if (!c || !hist) return fail(MAV_ERR_ARG, "mav_lk_last_iterations: NULL argument");
    if (!c->lk.hist_valid) return fail(MAV_ERR_STATE, "mav_lk_last_iterations: no track call precedes");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(hist, c->lk.counters + 2, MAV_LK_HIST * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    return mav_sync(c);
}

// stage hooks: one image through slot 0; the resident frame is dropped
static int lk_stage_begin(mav_ctx* c, const uint8_t* img, const void* out, const char* fn)
{
    if (!c || !img || !out) return fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_lk(c));
    c->lk.cur = -1; c->lk.built[1] = 0;
    return lk_load(c, 0, img, true);
}
static int lk_stage_level(mav_ctx* c, int level, const char* fn)
{
    if (level < 0 || level >= c->lk.dims.n) return fail(MAV_ERR_ARG, "%s: level %d outside [0, %d]", fn, level, c->lk.dims.n - 1);
    return MAV_OK;
}
extern "C" int mav_stage_lk_pyramid(mav_ctx* c, const uint8_t* img, int level, uint8_t* out)
{
    CHK(lk_stage_begin(c, img, out, "mav_stage_lk_pyramid"));
    CHK(lk_stage_level(c, level, "mav_stage_lk_pyramid"));
    LkState& k = c->lk;
    lk_build(c, 0, level + 1);
    CHK(check_launch("lk pyramid"));
    CHK(download(c, out, k.pyr[0] + k.dims.off[level], (size_t)k.dims.w[level] * k.dims.h[level]));
    const int rc = mav_sync(c);
    k.built[0] = 0;
    return rc;
}
extern "C" int mav_stage_lk_scharr(mav_ctx* c, const uint8_t* img, int level, int16_t* out)
{
    CHK(lk_stage_begin(c, img, out, "mav_stage_lk_scharr"));
    CHK(lk_stage_level(c, level, "mav_stage_lk_scharr"));
    LkState& k = c->lk;
    lk_build(c, 0, level + 1);
    lk_derivatives(c, 0, level + 1);
    CHK(check_launch("lk scharr"));
    CHK(download(c, out, k.deriv + k.dims.off[level], (size_t)k.dims.w[level] * k.dims.h[level] * sizeof(short2)));
    const int rc = mav_sync(c);
    k.built[0] = 0; k.deriv_slot = -1; k.deriv_levels = 0;
    return rc;
}
static int stage_corner_map(mav_ctx* c, const uint8_t* img, int block_size, const mav_corner_score* scp, float* out, const char* fn)
{
    mav_gftt_params p;
    mav_corner_score sc;
    mav_gftt_defaults(&p);
    p.block_size = block_size;
    CHK(check_gftt_params(p, fn));
    CHK(check_corner_score(scp, &sc, fn));
    CHK(lk_stage_begin(c, img, out, fn));
    LkState& k = c->lk;
    HIPCHK(hipMemsetAsync(k.counters, 0, 2 * sizeof(unsigned), c->stream));
    corner_map_enqueue(c, 0, nullptr, block_size, sc);
    CHK(check_launch("min_eig"));
    CHK(download(c, out, k.eig, c->n0 * sizeof(float)));
    const int rc = mav_sync(c);
    k.built[0] = 0;
    return rc;
}
extern "C" int mav_stage_min_eigen(mav_ctx* c, const uint8_t* img, int block_size, float* out)
{
    return stage_corner_map(c, img, block_size, nullptr, out, "mav_stage_min_eigen");
}
extern "C" int mav_stage_corner_response(mav_ctx* c, const uint8_t* img, int block_size, const mav_corner_score* sc, float* out)
{
    return stage_corner_map(c, img, block_size, sc, out, "mav_stage_corner_response");
}
extern "C" int mav_stage_corner_pick(mav_ctx* c, const uint64_t* keys, int n, const mav_gftt_params* pp, float* corners, int* count)
{
    mav_gftt_params p;
    if (pp) p = *pp; else mav_gftt_defaults(&p);
    CHK(check_gftt_params(p, "mav_stage_corner_pick"));
    if (!c || (n > 0 && !keys) || !corners || !count) return fail(MAV_ERR_ARG, "mav_stage_corner_pick: NULL argument");
    if (n < 0 || n > MAV_GFTT_MAX_CANDIDATES) return fail(MAV_ERR_ARG, "mav_stage_corner_pick: %d keys outside [0, %d]", n, MAV_GFTT_MAX_CANDIDATES);
    for (int i = 0; i < n; i++)
        if ((keys[i] & 0xffffffffu) >= c->n0) return fail(MAV_ERR_ARG, "mav_stage_corner_pick: key %d has index %u outside the frame", i, (unsigned)keys[i]);
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_lk(c));
    LkState& k = c->lk;
    // a key is (value bits << 32) | index; a candidate in memory is the pair (value bits, index)
    std::vector<uint2> cand((size_t)n);
    for (int i = 0; i < n; i++) cand[i] = make_uint2((unsigned)(keys[i] >> 32), (unsigned)keys[i]);
    const unsigned cnt[2] = {0u, (unsigned)n};
    HIPCHK(hipMemcpyAsync(k.counters, cnt, sizeof(cnt), hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(k.cand, cand.data(), (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    CHK(corner_pick_enqueue(c, p, k.out, reinterpret_cast<int*>(k.counters + LK_CNT_PICKED)));
    return corner_pick_fetch(c, p, corners, count, "mav_stage_corner_pick");
}

// ---- ground truth and radial error (include/mavflow_truth.h) ----------------------------------------------------------------------------
// These four keep every kind of resident state: the context's stream, staging blocks behind the last call's (HostCall::beside), the
// caller's outputs and radial_edges -- no last_* record is touched and no buffer one points at is written.
// Everything a ground-truth call can be refused for from its arguments alone, before the context is looked at.
static int gt_flow_checked(mav_ctx* c, const float* depth, const mav_gt_flow_params* params, int batch, int out_depth, const void* flow, bool dev,
                           const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!depth) return fail(MAV_ERR_ARG, "%s: NULL depth", fn);
    if (!params) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (!flow) return fail(MAV_ERR_ARG, "%s: NULL flow", fn);
    if (out_depth != MAV_DEPTH_32F && out_depth != MAV_DEPTH_64F) return fail(MAV_ERR_ARG, "%s: out_depth %d is neither MAV_DEPTH_32F nor MAV_DEPTH_64F", fn, out_depth);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    if (dev) {
        const size_t pair = 2 * depth_bytes(out_depth);
        if ((uintptr_t)depth % sizeof(float)) return fail(MAV_ERR_ARG, "%s: depth is not aligned to its 4-byte elements", fn);
        if ((uintptr_t)params % sizeof(double)) return fail(MAV_ERR_ARG, "%s: params is not aligned to 8 bytes", fn);
        if ((uintptr_t)flow % pair) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its %zu-byte pairs", fn, pair);
    } else {
        for (int b = 0; b < batch; b++)
            if (params[b].flags != 0) return fail(MAV_ERR_ARG, "%s: params[%d].flags 0x%x: no flag is defined", fn, b, params[b].flags);
    }
    return MAV_OK;
}
extern "C" int mav_gt_flow_dev(mav_ctx* c, const float* depth, const uint8_t* seg, const mav_gt_flow_params* params, int batch, int out_depth, void* flow)
{
    CHK(gt_flow_checked(c, depth, params, batch, out_depth, flow, true, "mav_gt_flow_dev"));
    CHK(check_dev_call(c, batch, "mav_gt_flow_dev"));
    {
        ProfScope ps(c, K_MISC);
        launch_gt_flow(c->stream, depth, seg, params, batch, c->W, c->H, out_depth == MAV_DEPTH_64F, flow);
    }
    return check_launch("ground-truth flow");
}
extern "C" int mav_gt_flow(mav_ctx* c, const float* depth, const uint8_t* seg, const mav_gt_flow_params* params, int batch, int out_depth, void* flow)
{
    CHK(gt_flow_checked(c, depth, params, batch, out_depth, flow, false, "mav_gt_flow"));
    HostCall h(c, "mav_gt_flow");
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch;
    const float* dd = h.in(depth, n * sizeof(float));
    const uint8_t* ds = h.in(seg, n);
    const mav_gt_flow_params* dp = h.in(params, sizeof(mav_gt_flow_params) * batch);
    char* df = h.out((char*)flow, n * 2 * depth_bytes(out_depth));
    CHK(h.staged());
    CHK(mav_gt_flow_dev(c, dd, ds, dp, batch, out_depth, df));
    return h.finish();
}

static int radial_edges_checked(const double* e, int n, const char* what, RadialEdges* out, const char* fn)
{
    if (!e) return fail(MAV_ERR_ARG, "%s: NULL %s_edges", fn, what);
    if (n < 2 || n > MAV_RADIAL_MAX_EDGES) return fail(MAV_ERR_ARG, "%s: %d %s_edges outside [2, %d]", fn, n, what, MAV_RADIAL_MAX_EDGES);
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(e[i])) return fail(MAV_ERR_ARG, "%s: %s_edges[%d] is not finite", fn, what, i);
        if (i && !(e[i - 1] < e[i])) return fail(MAV_ERR_ARG, "%s: %s_edges are not strictly increasing at [%d]", fn, what, i);
    }
    out->n = n;
    out->pad = 0;
    memcpy(out->e, e, sizeof(double) * n);
    memset(out->e + n, 0, sizeof(double) * (MAV_RADIAL_MAX_EDGES - n));
    return MAV_OK;
}
static int radial_hist_checked(mav_ctx* c, const float* flow, const float* gt_flow, int batch, const double* mag_edges, int n_mag_edges,
                               const double* err_edges, int n_err_edges, const int64_t* table, bool dev, RadialEdges* em, RadialEdges* ee, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!flow) return fail(MAV_ERR_ARG, "%s: NULL flow", fn);
    if (!gt_flow) return fail(MAV_ERR_ARG, "%s: NULL gt_flow", fn);
    if (!table) return fail(MAV_ERR_ARG, "%s: NULL table", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    CHK(radial_edges_checked(mag_edges, n_mag_edges, "mag", em, fn));
    CHK(radial_edges_checked(err_edges, n_err_edges, "err", ee, fn));
    if ((n_mag_edges - 1) * (n_err_edges - 1) > MAV_RADIAL_MAX_CELLS)
        return fail(MAV_ERR_ARG, "%s: %d x %d bins are more than %d cells", fn, n_mag_edges - 1, n_err_edges - 1, MAV_RADIAL_MAX_CELLS);
    if (dev) {
        if ((uintptr_t)flow % 8) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its 8-byte pairs", fn);
        if ((uintptr_t)gt_flow % 8) return fail(MAV_ERR_ARG, "%s: gt_flow is not aligned to its 8-byte pairs", fn);
        if ((uintptr_t)table % 8) return fail(MAV_ERR_ARG, "%s: table is not aligned to its 8-byte words", fn);
    }
    return MAV_OK;
}
static int radial_hist_enqueue(mav_ctx* c, const float* flow, const float* gt_flow, const uint8_t* sky, int batch, const RadialEdges& em,
                               const RadialEdges& ee, int64_t* table)
{
    if (!c->radial_edges) CHK(c->mem.alloc(&c->radial_edges, sizeof(double) * 2 * MAV_RADIAL_MAX_EDGES, MEM_OTHER, "radial-error edge lists"));
    const bool resident = c->radial_mag.n == em.n && c->radial_err.n == ee.n && !memcmp(c->radial_mag.e, em.e, sizeof(double) * em.n) &&
                          !memcmp(c->radial_err.e, ee.e, sizeof(double) * ee.n);
    c->radial_mag.n = c->radial_err.n = 0;                              // whatever goes wrong below, the lists are sent again
    ProfScope ps(c, K_MISC);
    const hipError_t e = launch_radial_hist(c->stream, flow, gt_flow, sky, batch, c->W, c->H, em, ee, c->radial_edges, resident, (unsigned long long*)table);
    if (e != hipSuccess) return fail(MAV_ERR_HIP, "radial-error histogram: granting the counters' LDS failed: %s", hipGetErrorString(e));
    CHK(check_launch("radial-error histogram"));
    c->radial_mag = em; c->radial_err = ee;
    return MAV_OK;
}
extern "C" int mav_radial_error_hist_dev(mav_ctx* c, const float* flow, const float* gt_flow, const uint8_t* sky, int batch, const double* mag_edges,
                                         int n_mag_edges, const double* err_edges, int n_err_edges, int64_t* table)
{
    RadialEdges em, ee;
    CHK(radial_hist_checked(c, flow, gt_flow, batch, mag_edges, n_mag_edges, err_edges, n_err_edges, table, true, &em, &ee, "mav_radial_error_hist_dev"));
    CHK(check_dev_call(c, batch, "mav_radial_error_hist_dev"));
    return radial_hist_enqueue(c, flow, gt_flow, sky, batch, em, ee, table);
}
extern "C" int mav_radial_error_hist(mav_ctx* c, const float* flow, const float* gt_flow, const uint8_t* sky, int batch, const double* mag_edges,
                                     int n_mag_edges, const double* err_edges, int n_err_edges, int64_t* table)
{
    RadialEdges em, ee;
    CHK(radial_hist_checked(c, flow, gt_flow, batch, mag_edges, n_mag_edges, err_edges, n_err_edges, table, false, &em, &ee, "mav_radial_error_hist"));
    HostCall h(c, "mav_radial_error_hist");
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch, words = MAV_RADIAL_TABLE_WORDS((size_t)(n_mag_edges - 1), (size_t)(n_err_edges - 1));
    const float* df = h.in(flow, n * 2 * sizeof(float));
    const float* dg = h.in(gt_flow, n * 2 * sizeof(float));
    const uint8_t* ds = h.in(sky, n);
    int64_t* dt = h.in(table, words * sizeof(int64_t));             // the caller's counts so far: the kernel adds to them
    h.fetch(table, dt, words * sizeof(int64_t));
    CHK(h.staged());
    CHK(radial_hist_enqueue(c, df, dg, ds, batch, em, ee, dt));
    return h.finish();
}

// ---- validation tail (include/mavflow_validation.h) --------------------------------------------------------------------------------------
// Like the ground-truth calls these keep every kind of resident state: the context's stream, staging blocks behind the last call's
// (HostCall::beside), the caller's outputs and gts_scratch -- no last_* record is touched and no buffer one points at is written.
extern "C" void mav_gt_stats_defaults(mav_gt_stats_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->dt = 1.0;
    p->box_fraction = 0.1;
    p->depth_fraction = 0.8f;
    p->seg_threshold = 127;
}
// Everything a call can be refused for from its arguments alone, before the context is looked at.
static int gt_stats_checked(mav_ctx* c, const uint8_t* seg, const float* gt_flow, const float* depth, const mav_gt_stats_params* params, int batch,
                            int max_pixels, const mav_gt_stats_record* records, const int32_t* indices, bool dev, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!seg) return fail(MAV_ERR_ARG, "%s: NULL seg", fn);
    if (!params) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    if (max_pixels < 1 || max_pixels > MAV_GT_STATS_MAX_PIXELS)
        return fail(MAV_ERR_ARG, "%s: max_pixels %d outside [1, %d]", fn, max_pixels, MAV_GT_STATS_MAX_PIXELS);
    if (dev) {
        if ((uintptr_t)depth % 4) return fail(MAV_ERR_ARG, "%s: depth is not aligned to its 4-byte elements", fn);
        if ((uintptr_t)gt_flow % 8) return fail(MAV_ERR_ARG, "%s: gt_flow is not aligned to its 8-byte pairs", fn);
        if ((uintptr_t)params % 8) return fail(MAV_ERR_ARG, "%s: params is not aligned to 8 bytes", fn);
        if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
        if ((uintptr_t)indices % 4) return fail(MAV_ERR_ARG, "%s: indices is not aligned to its 4-byte elements", fn);
    } else {
        for (int b = 0; b < batch; b++) {
            const mav_gt_stats_params& p = params[b];
            if (p.flags & ~(MAV_GT_STATS_FRAME0 | MAV_GT_STATS_THR_F64)) return fail(MAV_ERR_ARG, "%s: params[%d].flags 0x%x has unknown bits", fn, b, p.flags);
            for (int k = 0; k < 3; k++)
                if (!std::isfinite(p.omega[k])) return fail(MAV_ERR_ARG, "%s: params[%d].omega[%d] is not finite", fn, b, k);
            if (!std::isfinite(p.dt)) return fail(MAV_ERR_ARG, "%s: params[%d].dt is not finite", fn, b);
            if (p.dt == 0.0 && !(p.flags & MAV_GT_STATS_FRAME0)) return fail(MAV_ERR_ARG, "%s: params[%d].dt is 0 without MAV_GT_STATS_FRAME0", fn, b);
        }
    }
    return MAV_OK;
}
extern "C" int mav_gt_stats_dev(mav_ctx* c, const uint8_t* seg, const float* gt_flow, const uint8_t* sky, const float* depth,
                                const mav_gt_stats_params* params, int batch, int max_pixels, mav_gt_stats_record* records, int32_t* indices)
{
    const char* fn = "mav_gt_stats_dev";
    CHK(gt_stats_checked(c, seg, gt_flow, depth, params, batch, max_pixels, records, indices, true, fn));
    CHK(check_dev_call(c, batch, fn));
    CHK(grow_buffer(c, &c->gts_scratch, &c->gts_cap, gt_stats_scratch_bytes(batch, c->H, max_pixels, gt_flow && !indices), MEM_OTHER, READ_ON_COMPUTE,
                    ALLOC_FIRST, "validation scratch"));
    const GtStatsCall k{seg, sky, gt_flow, depth, params, batch, c->W, c->H, max_pixels, c->gts_scratch, records, indices};
    static const int kid[GTS_PHASES] = {K_GTS_MAX, K_GTS_COUNT, K_GTS_LIST, K_GTS_SUM};
    for (int ph = 0; ph < GTS_PHASES; ph++) {
        ProfScope ps(c, kid[ph]);
        launch_gt_stats_phase(c->stream, ph, k);
    }
    return check_launch("validation statistics");
}
extern "C" int mav_gt_stats(mav_ctx* c, const uint8_t* seg, const float* gt_flow, const uint8_t* sky, const float* depth, const mav_gt_stats_params* params,
                            int batch, int max_pixels, mav_gt_stats_record* records, int32_t* indices)
{
    CHK(gt_stats_checked(c, seg, gt_flow, depth, params, batch, max_pixels, records, indices, false, "mav_gt_stats"));
    HostCall h(c, "mav_gt_stats");
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch;
    const uint8_t* ds = h.in(seg, n);
    const float* dg = h.in(gt_flow, n * 2 * sizeof(float));
    const uint8_t* dk = h.in(sky, n);
    const float* dd = h.in(depth, n * sizeof(float));
    const mav_gt_stats_params* dp = h.in(params, sizeof(mav_gt_stats_params) * batch);
    mav_gt_stats_record* dr = h.out(records, sizeof(mav_gt_stats_record) * batch);
    int32_t* di = h.out(indices, sizeof(int32_t) * (size_t)batch * max_pixels);
    CHK(h.staged());
    CHK(mav_gt_stats_dev(c, ds, dg, dk, dd, dp, batch, max_pixels, dr, di));
    return h.finish();
}

// ---- k-means clustering (include/mavflow_cluster.h) ---------------------------------------------------------------------------------------
// Like the validation tail these keep every kind of resident state, and they hold no device memory of the context's at all: the _dev form
// works in the caller's workspace, the host form in staging blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_cluster.h"

extern "C" void mav_kmeans_defaults(mav_kmeans_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->K = 8;
    p->attempts = 10;
    p->max_iter = 10;
    p->dims = 3;
    p->depth = MAV_KMEANS_F32;
    p->eps = 1.0;
}
static int kmeans_shape_checked(int n, int K, int dims, const char* fn)
{
    if (K < 1 || K > MAV_KMEANS_MAX_K) return fail(MAV_ERR_ARG, "%s: K %d outside [1, %d]", fn, K, MAV_KMEANS_MAX_K);
    if (dims < 1 || dims > MAV_KMEANS_MAX_DIMS) return fail(MAV_ERR_ARG, "%s: dims %d outside [1, %d]", fn, dims, MAV_KMEANS_MAX_DIMS);
    if (n < K || n > MAV_KMEANS_MAX_N) return fail(MAV_ERR_ARG, "%s: n %d outside [K = %d, %d]", fn, n, K, MAV_KMEANS_MAX_N);
    return MAV_OK;
}
static int kmeans_params_checked(int n, const mav_kmeans_params* p, const char* fn)
{
    if (!p) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (p->attempts < 1 || p->attempts > MAV_KMEANS_MAX_ATTEMPTS) return fail(MAV_ERR_ARG, "%s: attempts %d outside [1, %d]", fn, p->attempts, MAV_KMEANS_MAX_ATTEMPTS);
    if (p->depth != MAV_KMEANS_F32 && p->depth != MAV_KMEANS_U8) return fail(MAV_ERR_ARG, "%s: depth %d is neither MAV_KMEANS_F32 nor MAV_KMEANS_U8", fn, p->depth);
    if (p->max_iter < 1) return fail(MAV_ERR_ARG, "%s: max_iter %d is less than 1", fn, p->max_iter);
    if (p->flags != 0) return fail(MAV_ERR_ARG, "%s: flags 0x%x: no flag is defined", fn, p->flags);
    if (!std::isfinite(p->eps)) return fail(MAV_ERR_ARG, "%s: eps is not finite", fn);
    return kmeans_shape_checked(n, p->K, p->dims, fn);
}
extern "C" size_t mav_kmeans_workspace_bytes(int n, int batch, const mav_kmeans_params* p)
{
    if (batch < 1 || kmeans_params_checked(n, p, "mav_kmeans_workspace_bytes") != MAV_OK) return 0;
    return km_image_bytes(n, p->attempts, p->K, p->dims) * (size_t)batch;
}
// Everything a call can be refused for from its arguments alone, before the context is looked at.
static int kmeans_checked(mav_ctx* c, const void* samples, int n, int batch, const mav_kmeans_params* p, const float* init, const int32_t* labels,
                          const float* centers, const mav_kmeans_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!samples) return fail(MAV_ERR_ARG, "%s: NULL samples", fn);
    if (!init) return fail(MAV_ERR_ARG, "%s: NULL init", fn);
    if (!labels) return fail(MAV_ERR_ARG, "%s: NULL labels", fn);
    if (!centers) return fail(MAV_ERR_ARG, "%s: NULL centers", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return kmeans_params_checked(n, p, fn);
}
static int kmeans_staging_checked(mav_ctx* c, int n, int batch, int dims, const char* fn)
{
    const size_t cap = (size_t)c->max_batch * c->n0 * 4;
    if ((size_t)batch * n * dims > cap) return fail(MAV_ERR_ARG, "%s: batch * n * dims = %zu is more than max_batch * W * H * 4 = %zu", fn, (size_t)batch * n * dims, cap);
    return MAV_OK;
}
extern "C" int mav_kmeans_dev(mav_ctx* c, const void* samples, int n, int batch, const mav_kmeans_params* p, const float* init, int32_t* labels, float* centers,
                              mav_kmeans_record* records, void* workspace, size_t workspace_bytes)
{
    const char* fn = "mav_kmeans_dev";
    CHK(kmeans_checked(c, samples, n, batch, p, init, labels, centers, records, fn));
    if (!workspace) return fail(MAV_ERR_ARG, "%s: NULL workspace", fn);
    if (p->depth == MAV_KMEANS_F32 && (uintptr_t)samples % 4) return fail(MAV_ERR_ARG, "%s: samples is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)init % 4) return fail(MAV_ERR_ARG, "%s: init is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)labels % 4) return fail(MAV_ERR_ARG, "%s: labels is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)centers % 4) return fail(MAV_ERR_ARG, "%s: centers is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    if ((uintptr_t)workspace % 16) return fail(MAV_ERR_ARG, "%s: workspace is not aligned to 16 bytes", fn);
    const size_t need = km_image_bytes(n, p->attempts, p->K, p->dims) * (size_t)batch;
    if (workspace_bytes < need) return fail(MAV_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    CHK(check_dev_call(c, batch, fn));
    KmCall k;
    k.samples = samples; k.init = init; k.labels = labels; k.centers = centers; k.records = records; k.ws = (char*)workspace;
    k.n = n; k.B = batch; k.A = p->attempts; k.K = p->K; k.D = p->dims; k.u8 = p->depth == MAV_KMEANS_U8;
    k.max_iter = p->max_iter < 2 ? 2 : p->max_iter > 100 ? 100 : p->max_iter;
    k.eps2 = p->eps > 0.0 ? p->eps * p->eps : 0.0;
    {
        ProfScope ps(c, K_MISC);
        launch_kmeans(c->stream, k);
    }
    return check_launch("k-means");
}
extern "C" int mav_kmeans(mav_ctx* c, const void* samples, int n, int batch, const mav_kmeans_params* p, const float* init, int32_t* labels, float* centers,
                          mav_kmeans_record* records)
{
    const char* fn = "mav_kmeans";
    CHK(kmeans_checked(c, samples, n, batch, p, init, labels, centers, records, fn));
    if (batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    CHK(kmeans_staging_checked(c, n, batch, p->dims, fn));
    const size_t items = (size_t)batch * n * p->dims, seeds = (size_t)batch * p->attempts * p->K * p->dims;
    if (p->depth == MAV_KMEANS_F32) {
        const float* x = (const float*)samples;
        for (size_t i = 0; i < items; i++)
            if (!std::isfinite(x[i])) return fail(MAV_ERR_ARG, "%s: samples[%zu] is not finite", fn, i);
    }
    for (size_t i = 0; i < seeds; i++)
        if (!std::isfinite(init[i])) return fail(MAV_ERR_ARG, "%s: init[%zu] is not finite", fn, i);
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t wsb = km_image_bytes(n, p->attempts, p->K, p->dims) * (size_t)batch;
    const char* dx = h.in((const char*)samples, items * (p->depth == MAV_KMEANS_U8 ? 1 : sizeof(float)));
    const float* di = h.in(init, seeds * sizeof(float));
    char* dw = h.scratch<char>(wsb);
    int32_t* dl = h.out(labels, sizeof(int32_t) * (size_t)batch * n);
    float* dc = h.out(centers, sizeof(float) * (size_t)batch * p->K * p->dims);
    mav_kmeans_record* dr = h.out(records, sizeof(mav_kmeans_record) * batch);
    CHK(h.staged());
    CHK(mav_kmeans_dev(c, dx, n, batch, p, di, dl, dc, dr, dw, wsb));
    return h.finish();
}
static int kmeans_paint_checked(mav_ctx* c, const int32_t* labels, const float* centers, int n, int batch, int K, int dims, const uint8_t* res, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!labels) return fail(MAV_ERR_ARG, "%s: NULL labels", fn);
    if (!centers) return fail(MAV_ERR_ARG, "%s: NULL centers", fn);
    if (!res) return fail(MAV_ERR_ARG, "%s: NULL res", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return kmeans_shape_checked(n, K, dims, fn);
}
extern "C" int mav_kmeans_paint_dev(mav_ctx* c, const int32_t* labels, const float* centers, int n, int batch, int K, int dims, uint8_t* res, uint8_t* mask)
{
    const char* fn = "mav_kmeans_paint_dev";
    CHK(kmeans_paint_checked(c, labels, centers, n, batch, K, dims, res, fn));
    if ((uintptr_t)labels % 4) return fail(MAV_ERR_ARG, "%s: labels is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)centers % 4) return fail(MAV_ERR_ARG, "%s: centers is not aligned to its 4-byte elements", fn);
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_kmeans_paint(c->stream, labels, centers, n, batch, K, dims, res, mask);
    }
    return check_launch("k-means paint");
}
extern "C" int mav_kmeans_paint(mav_ctx* c, const int32_t* labels, const float* centers, int n, int batch, int K, int dims, uint8_t* res, uint8_t* mask)
{
    const char* fn = "mav_kmeans_paint";
    CHK(kmeans_paint_checked(c, labels, centers, n, batch, K, dims, res, fn));
    if (batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    CHK(kmeans_staging_checked(c, n, batch, dims, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const int32_t* dl = h.in(labels, sizeof(int32_t) * (size_t)batch * n);
    const float* dc = h.in(centers, sizeof(float) * (size_t)batch * K * dims);
    uint8_t* dr = h.out(res, (size_t)batch * n * dims);
    uint8_t* dm = h.out(mask, (size_t)batch * n);
    CHK(h.staged());
    CHK(mav_kmeans_paint_dev(c, dl, dc, n, batch, K, dims, dr, dm));
    return h.finish();
}

// ---- image warps (include/mavflow_warp.h) ---------------------------------------------------------------------------------------------------
// Like the clustering calls these keep every kind of resident state and hold no device memory of the context's: the _dev forms work on the
// caller's blocks alone, the host forms in staging blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_warp.h"

static size_t warp_px_bytes(int format)     // bytes of one pixel; 0: no such format
{
    switch (format) {
    case MAV_WARP_U8C1: return 1;
    case MAV_WARP_U8C3: return 3;
    case MAV_WARP_F32C1: return 4;
    case MAV_WARP_F32C2: return 8;
    }
    return 0;
}
// Everything a warp can be refused for from its arguments alone, before the context is looked at.  ops: the policy's operands, by name.
static int warp_checked(mav_ctx* c, const void* src, int format, const void* a, const char* a_name, const void* b, const char* b_name, int flags, int batch,
                        const void* dst, bool dev, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!src) return fail(MAV_ERR_ARG, "%s: NULL src", fn);
    if (!a) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, a_name);
    if (b_name && !b) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, b_name);
    if (!dst) return fail(MAV_ERR_ARG, "%s: NULL dst", fn);
    if (!warp_px_bytes(format)) return fail(MAV_ERR_ARG, "%s: format %d is none of MAV_WARP_U8C1, _U8C3, _F32C1, _F32C2", fn, format);
    if (flags != 0 && flags != MAV_WARP_INVERSE_MAP) return fail(MAV_ERR_ARG, "%s: flags 0x%x: 0 or MAV_WARP_INVERSE_MAP", fn, flags);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    if (dev) {
        const bool f32 = format == MAV_WARP_F32C1 || format == MAV_WARP_F32C2;
        const bool matrix = a_name[0] == 'M';
        if (f32 && (uintptr_t)src % 4) return fail(MAV_ERR_ARG, "%s: src is not aligned to its 4-byte elements", fn);
        if (f32 && (uintptr_t)dst % 4) return fail(MAV_ERR_ARG, "%s: dst is not aligned to its 4-byte elements", fn);
        if ((uintptr_t)a % (matrix ? 8 : 4)) return fail(MAV_ERR_ARG, "%s: %s is not aligned to its %d-byte elements", fn, a_name, matrix ? 8 : 4);
        if (b_name && (uintptr_t)b % 4) return fail(MAV_ERR_ARG, "%s: %s is not aligned to its 4-byte elements", fn, b_name);
    }
    return MAV_OK;
}
// The host forms' look at the matrices: finite, and invertible where the call inverts (the determinant as the device takes it).
static int warp_matrices_checked(const double* M, int n, int batch, bool inverts, const char* fn)
{
    for (int b = 0; b < batch; b++) {
        const double* m = M + (size_t)b * n;
        for (int i = 0; i < n; i++)
            if (!std::isfinite(m[i])) return fail(MAV_ERR_ARG, "%s: M[%d][%d] is not finite", fn, b, i);
        if (!inverts) continue;
        const double d = n == 6 ? m[0] * m[4] - m[1] * m[3]
                                : (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
        if (d == 0 || !std::isfinite(d)) return fail(MAV_ERR_ARG, "%s: M[%d] is singular (determinant %g)", fn, b, d);
    }
    return MAV_OK;
}
static int warp_enqueue(mav_ctx* c, int policy, const void* src, int format, const void* a, const void* b, int flags, int batch, void* dst, const char* fn)
{
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_warp(c->stream, policy, format, src, a, b, flags, c->W, c->H, batch, dst);
    }
    return check_launch("warp");
}
// One host-form warp: a and b are host blocks of a_bytes / b_bytes per call.
static int warp_host(mav_ctx* c, int policy, const void* src, int format, const void* a, size_t a_bytes, const void* b, size_t b_bytes, int flags, int batch,
                     void* dst, const char* fn)
{
    if (batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t img = (size_t)batch * c->n0 * warp_px_bytes(format);
    const char* ds = h.in((const char*)src, img);
    const char* da = h.in((const char*)a, a_bytes);
    const char* db = h.in((const char*)b, b_bytes);
    char* dd = h.out((char*)dst, img);
    CHK(h.staged());
    CHK(warp_enqueue(c, policy, ds, format, da, db, flags, batch, dd, fn));
    return h.finish();
}
extern "C" int mav_remap_dev(mav_ctx* c, const void* src, int format, const float* map_xy, int batch, void* dst)
{
    const char* fn = "mav_remap_dev";
    CHK(warp_checked(c, src, format, map_xy, "map_xy", nullptr, nullptr, 0, batch, dst, true, fn));
    return warp_enqueue(c, WARP_POLICY_MAP, src, format, map_xy, nullptr, 0, batch, dst, fn);
}
extern "C" int mav_remap(mav_ctx* c, const void* src, int format, const float* map_xy, int batch, void* dst)
{
    const char* fn = "mav_remap";
    CHK(warp_checked(c, src, format, map_xy, "map_xy", nullptr, nullptr, 0, batch, dst, false, fn));
    return warp_host(c, WARP_POLICY_MAP, src, format, map_xy, sizeof(float) * 2 * batch * c->n0, nullptr, 0, 0, batch, dst, fn);
}
extern "C" int mav_remap_planes_dev(mav_ctx* c, const void* src, int format, const float* map_x, const float* map_y, int batch, void* dst)
{
    const char* fn = "mav_remap_planes_dev";
    CHK(warp_checked(c, src, format, map_x, "map_x", map_y, "map_y", 0, batch, dst, true, fn));
    return warp_enqueue(c, WARP_POLICY_PLANES, src, format, map_x, map_y, 0, batch, dst, fn);
}
extern "C" int mav_remap_planes(mav_ctx* c, const void* src, int format, const float* map_x, const float* map_y, int batch, void* dst)
{
    const char* fn = "mav_remap_planes";
    CHK(warp_checked(c, src, format, map_x, "map_x", map_y, "map_y", 0, batch, dst, false, fn));
    const size_t plane = sizeof(float) * batch * c->n0;
    return warp_host(c, WARP_POLICY_PLANES, src, format, map_x, plane, map_y, plane, 0, batch, dst, fn);
}
extern "C" int mav_warp_flow_dev(mav_ctx* c, const void* img, int format, const float* flow, int batch, void* dst)
{
    const char* fn = "mav_warp_flow_dev";
    CHK(warp_checked(c, img, format, flow, "flow", nullptr, nullptr, 0, batch, dst, true, fn));
    return warp_enqueue(c, WARP_POLICY_FLOW, img, format, flow, nullptr, 0, batch, dst, fn);
}
extern "C" int mav_warp_flow(mav_ctx* c, const void* img, int format, const float* flow, int batch, void* dst)
{
    const char* fn = "mav_warp_flow";
    CHK(warp_checked(c, img, format, flow, "flow", nullptr, nullptr, 0, batch, dst, false, fn));
    return warp_host(c, WARP_POLICY_FLOW, img, format, flow, sizeof(float) * 2 * batch * c->n0, nullptr, 0, 0, batch, dst, fn);
}
extern "C" int mav_warp_affine_dev(mav_ctx* c, const void* src, int format, const double* M, int flags, int batch, void* dst)
{
    const char* fn = "mav_warp_affine_dev";
    CHK(warp_checked(c, src, format, M, "M", nullptr, nullptr, flags, batch, dst, true, fn));
    return warp_enqueue(c, WARP_POLICY_AFFINE, src, format, M, nullptr, flags, batch, dst, fn);
}
extern "C" int mav_warp_affine(mav_ctx* c, const void* src, int format, const double* M, int flags, int batch, void* dst)
{
    const char* fn = "mav_warp_affine";
    CHK(warp_checked(c, src, format, M, "M", nullptr, nullptr, flags, batch, dst, false, fn));
    CHK(warp_matrices_checked(M, 6, batch, !(flags & MAV_WARP_INVERSE_MAP), fn));
    return warp_host(c, WARP_POLICY_AFFINE, src, format, M, sizeof(double) * 6 * batch, nullptr, 0, flags, batch, dst, fn);
}
extern "C" int mav_warp_perspective_dev(mav_ctx* c, const void* src, int format, const double* M, int flags, int batch, void* dst)
{
    const char* fn = "mav_warp_perspective_dev";
    CHK(warp_checked(c, src, format, M, "M", nullptr, nullptr, flags, batch, dst, true, fn));
    return warp_enqueue(c, WARP_POLICY_PERSPECTIVE, src, format, M, nullptr, flags, batch, dst, fn);
}
extern "C" int mav_warp_perspective(mav_ctx* c, const void* src, int format, const double* M, int flags, int batch, void* dst)
{
    const char* fn = "mav_warp_perspective";
    CHK(warp_checked(c, src, format, M, "M", nullptr, nullptr, flags, batch, dst, false, fn));
    CHK(warp_matrices_checked(M, 9, batch, !(flags & MAV_WARP_INVERSE_MAP), fn));
    return warp_host(c, WARP_POLICY_PERSPECTIVE, src, format, M, sizeof(double) * 9 * batch, nullptr, 0, flags, batch, dst, fn);
}
static int warp_method_checked(mav_ctx* c, const float* flow, const double* M, int kind, int batch, const mav_warp_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!flow) return fail(MAV_ERR_ARG, "%s: NULL flow", fn);
    if (!M) return fail(MAV_ERR_ARG, "%s: NULL M", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (kind != MAV_WARP_AFFINE && kind != MAV_WARP_PERSPECTIVE) return fail(MAV_ERR_ARG, "%s: kind %d is neither MAV_WARP_AFFINE nor MAV_WARP_PERSPECTIVE", fn, kind);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return MAV_OK;
}
extern "C" int mav_warp_method_dev(mav_ctx* c, const float* flow, const double* M, int kind, int batch, float* diff, float* mag, mav_warp_record* records)
{
    const char* fn = "mav_warp_method_dev";
    CHK(warp_method_checked(c, flow, M, kind, batch, records, fn));
    if ((uintptr_t)flow % 4) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)M % 8) return fail(MAV_ERR_ARG, "%s: M is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)diff % 4) return fail(MAV_ERR_ARG, "%s: diff is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)mag % 4) return fail(MAV_ERR_ARG, "%s: mag is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_warp_method(c->stream, kind == MAV_WARP_AFFINE ? WARP_POLICY_AFFINE : WARP_POLICY_PERSPECTIVE, flow, M, c->W, c->H, batch, diff, mag, records);
    }
    return check_launch("warp method");
}
extern "C" int mav_warp_method(mav_ctx* c, const float* flow, const double* M, int kind, int batch, float* diff, float* mag, mav_warp_record* records)
{
    const char* fn = "mav_warp_method";
    CHK(warp_method_checked(c, flow, M, kind, batch, records, fn));
    const int n = kind == MAV_WARP_AFFINE ? 6 : 9;
    CHK(warp_matrices_checked(M, n, batch, true, fn));
    if (batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const float* df = h.in(flow, sizeof(float) * 2 * batch * c->n0);
    const double* dm = h.in(M, sizeof(double) * n * batch);
    float* dd = h.out(diff, sizeof(float) * 2 * batch * c->n0);
    float* dg = h.out(mag, sizeof(float) * batch * c->n0);
    mav_warp_record* dr = h.out(records, sizeof(mav_warp_record) * batch);
    CHK(h.staged());
    CHK(mav_warp_method_dev(c, df, dm, kind, batch, dd, dg, dr));
    return h.finish();
}

// ---- image resize (include/mavflow_resize.h) ------------------------------------------------------------------------------------------------
// Like the warps these keep every kind of resident state and hold no device memory of the context's: the _dev forms work on the caller's
// blocks alone and allocate nothing, the host forms in staging blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_resize.h"

// Everything a resize can be refused for from its arguments alone, before the context is looked at.  px_src / px_dst: bytes per pixel.
static int resize_checked(mav_ctx* c, const void* src, const char* src_name, size_t px_src, int sw, int sh, int dw, int dh, int batch, const void* dst,
                          const char* dst_name, size_t px_dst, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!src) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, src_name);
    if (!dst) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, dst_name);
    const int sides[4] = {sw, sh, dw, dh};
    const char* names[4] = {"sw", "sh", "dw", "dh"};
    for (int i = 0; i < 4; i++)
        if (sides[i] < 1 || sides[i] > MAV_RESIZE_MAX_SIDE) return fail(MAV_ERR_ARG, "%s: %s %d outside [1, %d]", fn, names[i], sides[i], MAV_RESIZE_MAX_SIDE);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)batch * sw * sh * px_src, d0 = (uintptr_t)dst, d1 = d0 + (size_t)batch * dw * dh * px_dst;
    if (s0 < d1 && d0 < s1) return fail(MAV_ERR_ARG, "%s: %s and %s overlap", fn, src_name, dst_name);
    return MAV_OK;
}
static int resize_call_checked(mav_ctx* c, const void* src, int format, int sw, int sh, int dw, int dh, int interpolation, int batch, const void* dst, bool dev,
                               const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!warp_px_bytes(format)) return fail(MAV_ERR_ARG, "%s: format %d is none of MAV_WARP_U8C1, _U8C3, _F32C1, _F32C2", fn, format);
    if (interpolation != MAV_INTER_NEAREST && interpolation != MAV_INTER_LINEAR && interpolation != MAV_INTER_AREA)
        return fail(MAV_ERR_ARG, "%s: interpolation %d is none of MAV_INTER_NEAREST, _LINEAR, _AREA", fn, interpolation);
    CHK(resize_checked(c, src, "src", warp_px_bytes(format), sw, sh, dw, dh, batch, dst, "dst", warp_px_bytes(format), fn));
    if (interpolation == MAV_INTER_AREA && (dw > sw || dh > sh))
        return fail(MAV_ERR_ARG, "%s: MAV_INTER_AREA enlarging (%d x %d -> %d x %d) is not built", fn, sw, sh, dw, dh);
    if (dev && (format == MAV_WARP_F32C1 || format == MAV_WARP_F32C2)) {
        if ((uintptr_t)src % 4) return fail(MAV_ERR_ARG, "%s: src is not aligned to its 4-byte elements", fn);
        if ((uintptr_t)dst % 4) return fail(MAV_ERR_ARG, "%s: dst is not aligned to its 4-byte elements", fn);
    }
    return MAV_OK;
}
static int sky_mask_checked(mav_ctx* c, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int batch, const uint8_t* sky, const char* fn)
{
    CHK(resize_checked(c, pred_bgr, "pred_bgr", 3, sw, sh, dw, dh, batch, sky, "sky", 1, fn));
    if (key0 < 0 || key0 > 255) return fail(MAV_ERR_ARG, "%s: key0 %d outside [0, 255]", fn, key0);
    if (key1 < 0 || key1 > 255) return fail(MAV_ERR_ARG, "%s: key1 %d outside [0, 255]", fn, key1);
    return MAV_OK;
}
extern "C" int mav_resize_dev(mav_ctx* c, const void* src, int format, int sw, int sh, int dw, int dh, int interpolation, int batch, void* dst)
{
    const char* fn = "mav_resize_dev";
    CHK(resize_call_checked(c, src, format, sw, sh, dw, dh, interpolation, batch, dst, true, fn));
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_resize(c->stream, format, src, sw, sh, dw, dh, interpolation, batch, dst);
    }
    return check_launch("resize");
}
extern "C" int mav_resize(mav_ctx* c, const void* src, int format, int sw, int sh, int dw, int dh, int interpolation, int batch, void* dst)
{
    const char* fn = "mav_resize";
    CHK(resize_call_checked(c, src, format, sw, sh, dw, dh, interpolation, batch, dst, false, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t px = warp_px_bytes(format);
    const char* ds = h.in((const char*)src, (size_t)batch * sw * sh * px);
    char* dd = h.out((char*)dst, (size_t)batch * dw * dh * px);
    CHK(h.staged());
    {
        ProfScope ps(c, K_MISC);
        launch_resize(c->stream, format, ds, sw, sh, dw, dh, interpolation, batch, dd);
    }
    CHK(check_launch("resize"));
    return h.finish();
}
extern "C" int mav_sky_mask_dev(mav_ctx* c, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int batch, uint8_t* sky)
{
    const char* fn = "mav_sky_mask_dev";
    CHK(sky_mask_checked(c, pred_bgr, sw, sh, dw, dh, key0, key1, batch, sky, fn));
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_sky_mask(c->stream, pred_bgr, sw, sh, dw, dh, key0, key1, batch, sky);
    }
    return check_launch("sky mask");
}
extern "C" int mav_sky_mask(mav_ctx* c, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int batch, uint8_t* sky)
{
    const char* fn = "mav_sky_mask";
    CHK(sky_mask_checked(c, pred_bgr, sw, sh, dw, dh, key0, key1, batch, sky, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const uint8_t* dp = h.in(pred_bgr, (size_t)batch * sw * sh * 3);
    uint8_t* dk = h.out(sky, (size_t)batch * dw * dh);
    CHK(h.staged());
    {
        ProfScope ps(c, K_MISC);
        launch_sky_mask(c->stream, dp, sw, sh, dw, dh, key0, key1, batch, dk);
    }
    CHK(check_launch("sky mask"));
    return h.finish();
}

// ---- robust affine fit (include/mavflow_affine.h) -------------------------------------------------------------------------------------------
// Like the warps these keep every kind of resident state and hold no device memory of the context's: the _dev forms work in the caller's
// workspace (the flow form's gathered pairs included), the host forms in staging blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_affine.h"
#include <cfloat>

extern "C" void mav_affine_defaults(mav_affine_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 3.0;
    p->confidence = 0.99;
    p->max_iters = 2000;
    p->refine = 1;
}
static int affine_params_checked(int n, const mav_affine_params* p, const char* fn)
{
    if (!p) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (n < 3 || n > MAV_AFFINE_MAX_PAIRS) return fail(MAV_ERR_ARG, "%s: n %d outside [3, %d]", fn, n, MAV_AFFINE_MAX_PAIRS);
    if (p->max_iters < 1 || p->max_iters > MAV_AFFINE_MAX_ITERS) return fail(MAV_ERR_ARG, "%s: max_iters %d outside [1, %d]", fn, p->max_iters, MAV_AFFINE_MAX_ITERS);
    if (!std::isfinite(p->threshold) || p->threshold < 0.0) return fail(MAV_ERR_ARG, "%s: threshold %g is negative or not finite", fn, p->threshold);
    if (!(p->confidence > 0.0 && p->confidence < 1.0)) return fail(MAV_ERR_ARG, "%s: confidence %g outside (0, 1)", fn, p->confidence);
    if (p->flags != 0) return fail(MAV_ERR_ARG, "%s: flags 0x%x: no flag is defined", fn, p->flags);
    return MAV_OK;
}
extern "C" size_t mav_estimate_affine_workspace_bytes(int n, int batch, const mav_affine_params* p)
{
    if (batch < 1) { fail(MAV_ERR_ARG, "mav_estimate_affine_workspace_bytes: batch %d is less than 1", batch); return 0; }
    if (affine_params_checked(n, p, "mav_estimate_affine_workspace_bytes") != MAV_OK) return 0;
    return aff_workspace_bytes(n, batch, p->max_iters);
}
// need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 3, max_iters) as the header writes it out
static void affine_need_table(int n, double confidence, int max_iters, int32_t* need)
{
    const double ln = log(1.0 - confidence);
    for (int g = 0; g <= n; g++) {
        if (g < 3) { need[g] = max_iters; continue; }
        const double w = (double)g / (double)n;
        const double den = 1.0 - (w * w) * w;
        if (den < DBL_MIN) { need[g] = 0; continue; }
        const double ld = log(den);
        need[g] = ld >= 0.0 || -ln >= max_iters * (-ld) ? max_iters : (int32_t)nearbyint(ln / ld);
    }
}
// Everything a call can be refused for from its arguments alone, before the context is looked at.  a, b: src and dst, or flow and coords.
static int affine_checked(mav_ctx* c, const void* a, const char* a_name, const void* b, const char* b_name, int n, int batch, const mav_affine_params* p,
                          const int32_t* triples, const double* M, const uint8_t* inliers, const mav_affine_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!a) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, a_name);
    if (!b) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, b_name);
    if (!triples) return fail(MAV_ERR_ARG, "%s: NULL triples", fn);
    if (!M) return fail(MAV_ERR_ARG, "%s: NULL M", fn);
    if (!inliers) return fail(MAV_ERR_ARG, "%s: NULL inliers", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return affine_params_checked(n, p, fn);
}
// what the _dev forms refuse beyond that: a's alignment is `a_align`, b's is checked where b is a device pointer (b_align != 0)
static int affine_dev_checked(const void* a, const char* a_name, size_t a_align, const void* b, const char* b_name, size_t b_align, int n, int batch,
                              const mav_affine_params* p, const int32_t* triples, const double* M, const mav_affine_record* records, const void* workspace,
                              size_t workspace_bytes, const char* fn)
{
    if (!workspace) return fail(MAV_ERR_ARG, "%s: NULL workspace", fn);
    if ((uintptr_t)a % a_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, a_name, a_align);
    if (b_align && (uintptr_t)b % b_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, b_name, b_align);
    if ((uintptr_t)triples % 4) return fail(MAV_ERR_ARG, "%s: triples is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)M % 8) return fail(MAV_ERR_ARG, "%s: M is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    if ((uintptr_t)workspace % 16) return fail(MAV_ERR_ARG, "%s: workspace is not aligned to 16 bytes", fn);
    const size_t need = aff_workspace_bytes(n, batch, p->max_iters);
    if (workspace_bytes < need) return fail(MAV_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return MAV_OK;
}
// the host forms' triples: every index inside [0, n), no index twice
static int affine_triples_checked(const int32_t* t, int n, int batch, int max_iters, const char* fn)
{
    for (size_t i = 0; i < (size_t)batch * max_iters; i++) {
        const int32_t *q = t + 3 * i;
        for (int j = 0; j < 3; j++)
            if (q[j] < 0 || q[j] >= n) return fail(MAV_ERR_ARG, "%s: triples[%zu][%d] = %d outside [0, %d)", fn, i, j, q[j], n);
        if (q[0] == q[1] || q[0] == q[2] || q[1] == q[2]) return fail(MAV_ERR_ARG, "%s: triples[%zu] = (%d, %d, %d) repeats an index", fn, i, q[0], q[1], q[2]);
    }
    return MAV_OK;
}
static int affine_coords_checked(const mav_ctx* c, const int32_t* coords, int n, const char* fn)
{
    for (int i = 0; i < n; i++)
        if (coords[2 * i] < 0 || coords[2 * i] >= c->W || coords[2 * i + 1] < 0 || coords[2 * i + 1] >= c->H)
            return fail(MAV_ERR_ARG, "%s: sample %d = (%d, %d) lies outside the %dx%d frame", fn, i, coords[2 * i], coords[2 * i + 1], c->W, c->H);
    return MAV_OK;
}
// the table's copy and the three launches
static int affine_enqueue(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_affine_params* p, const int32_t* triples, double* M,
                          uint8_t* inliers, mav_affine_record* records, void* workspace)
{
    std::vector<int32_t> need((size_t)n + 1);             // this call's own block: the copy below has taken its bytes when it returns
    affine_need_table(n, p->confidence, p->max_iters, need.data());
    HIPCHK(hipMemcpyAsync(workspace, need.data(), sizeof(int32_t) * need.size(), hipMemcpyHostToDevice, c->stream));
    AffCall a;
    a.src = src; a.dst = dst; a.triples = triples; a.M = M; a.inliers = inliers; a.records = records; a.ws = (char*)workspace;
    a.n = n; a.B = batch; a.max_iters = p->max_iters; a.refine = p->refine != 0; a.t2 = p->threshold * p->threshold;
    { ProfScope ps(c, K_MISC); launch_affine_score(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_affine_choose(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_affine_finish(c->stream, a); }
    return check_launch("affine fit");
}
extern "C" int mav_estimate_affine_dev(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_affine_params* p, const int32_t* triples,
                                       double* M, uint8_t* inliers, mav_affine_record* records, void* workspace, size_t workspace_bytes)
{
    const char* fn = "mav_estimate_affine_dev";
    CHK(affine_checked(c, src, "src", dst, "dst", n, batch, p, triples, M, inliers, records, fn));
    CHK(affine_dev_checked(src, "src", 8, dst, "dst", 8, n, batch, p, triples, M, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    return affine_enqueue(c, src, dst, n, batch, p, triples, M, inliers, records, workspace);
}
extern "C" int mav_estimate_affine(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_affine_params* p, const int32_t* triples,
                                   double* M, uint8_t* inliers, mav_affine_record* records)
{
    const char* fn = "mav_estimate_affine";
    CHK(affine_checked(c, src, "src", dst, "dst", n, batch, p, triples, M, inliers, records, fn));
    CHK(affine_triples_checked(triples, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t pairs = sizeof(double) * 2 * (size_t)n * batch, wsb = aff_workspace_bytes(n, batch, p->max_iters);
    const double *ds = h.in(src, pairs), *dd = h.in(dst, pairs);
    const int32_t* dt = h.in(triples, sizeof(int32_t) * 3 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dM = h.out(M, sizeof(double) * 6 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_affine_record* dr = h.out(records, sizeof(mav_affine_record) * batch);
    CHK(h.staged());
    CHK(mav_estimate_affine_dev(c, ds, dd, n, batch, p, dt, dM, di, dr, dw, wsb));
    return h.finish();
}
extern "C" int mav_flow_affine_dev(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_affine_params* p, const int32_t* triples,
                                   double* M, uint8_t* inliers, mav_affine_record* records, void* workspace, size_t workspace_bytes)
{
    const char* fn = "mav_flow_affine_dev";
    CHK(affine_checked(c, flow, "flow", coords, "coords", n, batch, p, triples, M, inliers, records, fn));
    CHK(affine_dev_checked(flow, "flow", 8, coords, "coords", 0, n, batch, p, triples, M, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    CHK(affine_coords_checked(c, coords, n, fn));
    char* ws = (char*)workspace;
    int32_t* dcoords = (int32_t*)(ws + aff_coords_offset(n, batch, p->max_iters));
    double *ps = (double*)(ws + aff_src_offset(n, batch, p->max_iters)), *pd = (double*)(ws + aff_dst_offset(n, batch, p->max_iters));
    HIPCHK(hipMemcpyAsync(dcoords, coords, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    { ProfScope ps_(c, K_MISC); launch_pair_gather(c->stream, flow, dcoords, n, batch, c->W, c->H, ps, pd); }
    CHK(check_launch("pair_gather"));
    return affine_enqueue(c, ps, pd, n, batch, p, triples, M, inliers, records, workspace);
}
extern "C" int mav_flow_affine(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_affine_params* p, const int32_t* triples,
                               double* M, uint8_t* inliers, mav_affine_record* records, double* pairs_dst)
{
    const char* fn = "mav_flow_affine";
    CHK(affine_checked(c, flow, "flow", coords, "coords", n, batch, p, triples, M, inliers, records, fn));
    CHK(affine_triples_checked(triples, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    CHK(affine_coords_checked(c, coords, n, fn));
    const size_t wsb = aff_workspace_bytes(n, batch, p->max_iters);
    const float* df = h.in(flow, c->n0 * batch * 2 * sizeof(float));
    const int32_t* dt = h.in(triples, sizeof(int32_t) * 3 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dM = h.out(M, sizeof(double) * 6 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_affine_record* dr = h.out(records, sizeof(mav_affine_record) * batch);
    if (dw) h.fetch(pairs_dst, dw + aff_dst_offset(n, batch, p->max_iters), sizeof(double) * 2 * (size_t)n * batch);
    CHK(h.staged());
    CHK(mav_flow_affine_dev(c, df, coords, n, batch, p, dt, dM, di, dr, dw, wsb));
    return h.finish();
}

// ---- robust fundamental-matrix fit and dense epipolar residual (include/mavflow_fundamental.h) ---------------------------------------------
// As the affine fit: every kind of resident state is kept, no device memory of the context's is held; the _dev forms work in the caller's
// workspace (the flow form's gathered pairs included), the host forms in staging blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_fundamental.h"

extern "C" void mav_fundamental_defaults(mav_fundamental_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 3.0;
    p->confidence = 0.99;
    p->max_iters = 1000;
}
static int fundamental_params_checked(int n, const mav_fundamental_params* p, const char* fn)
{
    if (!p) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (n < 7 || n > MAV_FUNDAMENTAL_MAX_PAIRS) return fail(MAV_ERR_ARG, "%s: n %d outside [7, %d]", fn, n, MAV_FUNDAMENTAL_MAX_PAIRS);
    if (p->max_iters < 1 || p->max_iters > MAV_FUNDAMENTAL_MAX_ITERS)
        return fail(MAV_ERR_ARG, "%s: max_iters %d outside [1, %d]", fn, p->max_iters, MAV_FUNDAMENTAL_MAX_ITERS);
    if (!std::isfinite(p->threshold) || p->threshold < 0.0) return fail(MAV_ERR_ARG, "%s: threshold %g is negative or not finite", fn, p->threshold);
    if (!(p->confidence > 0.0 && p->confidence < 1.0)) return fail(MAV_ERR_ARG, "%s: confidence %g outside (0, 1)", fn, p->confidence);
    if (p->flags != 0) return fail(MAV_ERR_ARG, "%s: flags 0x%x: no flag is defined", fn, p->flags);
    return MAV_OK;
}
extern "C" size_t mav_find_fundamental_workspace_bytes(int n, int batch, const mav_fundamental_params* p)
{
    if (batch < 1) { fail(MAV_ERR_ARG, "mav_find_fundamental_workspace_bytes: batch %d is less than 1", batch); return 0; }
    if (fundamental_params_checked(n, p, "mav_find_fundamental_workspace_bytes") != MAV_OK) return 0;
    return fm_workspace_bytes(n, batch, p->max_iters);
}
// need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 7, max_iters) as the header writes it out
static void fundamental_need_table(int n, double confidence, int max_iters, int32_t* need)
{
    const double ln = log(1.0 - confidence);
    for (int g = 0; g <= n; g++) {
        if (g < 7) { need[g] = max_iters; continue; }
        const double w = (double)g / (double)n;
        const double w2 = w * w;
        const double w4 = w2 * w2;
        const double den = 1.0 - (w4 * w2) * w;
        if (den < DBL_MIN) { need[g] = 0; continue; }
        const double ld = log(den);
        need[g] = ld >= 0.0 || -ln >= max_iters * (-ld) ? max_iters : (int32_t)nearbyint(ln / ld);
    }
}
// Everything a call can be refused for from its arguments alone, before the context is looked at.  a, b: src and dst, or flow and coords.
static int fundamental_checked(mav_ctx* c, const void* a, const char* a_name, const void* b, const char* b_name, int n, int batch,
                               const mav_fundamental_params* p, const int32_t* subsets, const double* F, const uint8_t* inliers,
                               const mav_fundamental_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!a) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, a_name);
    if (!b) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, b_name);
    if (!subsets) return fail(MAV_ERR_ARG, "%s: NULL subsets", fn);
    if (!F) return fail(MAV_ERR_ARG, "%s: NULL F", fn);
    if (!inliers) return fail(MAV_ERR_ARG, "%s: NULL inliers", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return fundamental_params_checked(n, p, fn);
}
// what the _dev forms refuse beyond that: a's alignment is `a_align`, b's is checked where b is a device pointer (b_align != 0)
static int fundamental_dev_checked(const void* a, const char* a_name, size_t a_align, const void* b, const char* b_name, size_t b_align, int n, int batch,
                                   const mav_fundamental_params* p, const int32_t* subsets, const double* F, const mav_fundamental_record* records,
                                   const void* workspace, size_t workspace_bytes, const char* fn)
{
    if (!workspace) return fail(MAV_ERR_ARG, "%s: NULL workspace", fn);
    if ((uintptr_t)a % a_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, a_name, a_align);
    if (b_align && (uintptr_t)b % b_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, b_name, b_align);
    if ((uintptr_t)subsets % 4) return fail(MAV_ERR_ARG, "%s: subsets is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)F % 8) return fail(MAV_ERR_ARG, "%s: F is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    if ((uintptr_t)workspace % 16) return fail(MAV_ERR_ARG, "%s: workspace is not aligned to 16 bytes", fn);
    const size_t need = fm_workspace_bytes(n, batch, p->max_iters);
    if (workspace_bytes < need) return fail(MAV_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return MAV_OK;
}
// the host forms' subsets: every index inside [0, n), no index twice
static int fundamental_subsets_checked(const int32_t* t, int n, int batch, int max_iters, const char* fn)
{
    for (size_t i = 0; i < (size_t)batch * max_iters; i++) {
        const int32_t* q = t + 7 * i;
        for (int j = 0; j < 7; j++) {
            if (q[j] < 0 || q[j] >= n) return fail(MAV_ERR_ARG, "%s: subsets[%zu][%d] = %d outside [0, %d)", fn, i, j, q[j], n);
            for (int k = 0; k < j; k++)
                if (q[k] == q[j]) return fail(MAV_ERR_ARG, "%s: subsets[%zu] repeats the index %d", fn, i, q[j]);
        }
    }
    return MAV_OK;
}
// the table's copy and the four launches
static int fundamental_enqueue(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_fundamental_params* p, const int32_t* subsets,
                               double* F, uint8_t* inliers, mav_fundamental_record* records, void* workspace)
{
    std::vector<int32_t> need((size_t)n + 1);             // this call's own block: the copy below has taken its bytes when it returns
    fundamental_need_table(n, p->confidence, p->max_iters, need.data());
    HIPCHK(hipMemcpyAsync(workspace, need.data(), sizeof(int32_t) * need.size(), hipMemcpyHostToDevice, c->stream));
    FmCall a;
    a.src = src; a.dst = dst; a.subsets = subsets; a.F = F; a.inliers = inliers; a.records = records; a.ws = (char*)workspace;
    a.n = n; a.B = batch; a.max_iters = p->max_iters; a.t2 = p->threshold * p->threshold;
    { ProfScope ps(c, K_MISC); launch_fm_models(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_fm_score(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_fm_choose(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_fm_finish(c->stream, a); }
    return check_launch("fundamental fit");
}
extern "C" int mav_find_fundamental_dev(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_fundamental_params* p,
                                        const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, void* workspace,
                                        size_t workspace_bytes)
{
    const char* fn = "mav_find_fundamental_dev";
    CHK(fundamental_checked(c, src, "src", dst, "dst", n, batch, p, subsets, F, inliers, records, fn));
    CHK(fundamental_dev_checked(src, "src", 8, dst, "dst", 8, n, batch, p, subsets, F, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    return fundamental_enqueue(c, src, dst, n, batch, p, subsets, F, inliers, records, workspace);
}
extern "C" int mav_find_fundamental(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_fundamental_params* p,
                                    const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records)
{
    const char* fn = "mav_find_fundamental";
    CHK(fundamental_checked(c, src, "src", dst, "dst", n, batch, p, subsets, F, inliers, records, fn));
    CHK(fundamental_subsets_checked(subsets, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t pairs = sizeof(double) * 2 * (size_t)n * batch, wsb = fm_workspace_bytes(n, batch, p->max_iters);
    const double *ds = h.in(src, pairs), *dd = h.in(dst, pairs);
    const int32_t* dt = h.in(subsets, sizeof(int32_t) * 7 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dF = h.out(F, sizeof(double) * 9 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_fundamental_record* dr = h.out(records, sizeof(mav_fundamental_record) * batch);
    CHK(h.staged());
    CHK(mav_find_fundamental_dev(c, ds, dd, n, batch, p, dt, dF, di, dr, dw, wsb));
    return h.finish();
}
extern "C" int mav_flow_fundamental_dev(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_fundamental_params* p,
                                        const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, void* workspace,
                                        size_t workspace_bytes)
{
    const char* fn = "mav_flow_fundamental_dev";
    CHK(fundamental_checked(c, flow, "flow", coords, "coords", n, batch, p, subsets, F, inliers, records, fn));
    CHK(fundamental_dev_checked(flow, "flow", 8, coords, "coords", 0, n, batch, p, subsets, F, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    CHK(affine_coords_checked(c, coords, n, fn));         // the affine flow form's range check of the host coords
    char* ws = (char*)workspace;
    int32_t* dcoords = (int32_t*)(ws + fm_coords_offset(n, batch, p->max_iters));
    double *ps = (double*)(ws + fm_src_offset(n, batch, p->max_iters)), *pd = (double*)(ws + fm_dst_offset(n, batch, p->max_iters));
    HIPCHK(hipMemcpyAsync(dcoords, coords, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    { ProfScope ps_(c, K_MISC); launch_pair_gather(c->stream, flow, dcoords, n, batch, c->W, c->H, ps, pd); }
    CHK(check_launch("pair_gather"));
    return fundamental_enqueue(c, ps, pd, n, batch, p, subsets, F, inliers, records, workspace);
}
extern "C" int mav_flow_fundamental(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_fundamental_params* p,
                                    const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, double* pairs_dst)
{
    const char* fn = "mav_flow_fundamental";
    CHK(fundamental_checked(c, flow, "flow", coords, "coords", n, batch, p, subsets, F, inliers, records, fn));
    CHK(fundamental_subsets_checked(subsets, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    CHK(affine_coords_checked(c, coords, n, fn));
    const size_t wsb = fm_workspace_bytes(n, batch, p->max_iters);
    const float* df = h.in(flow, c->n0 * batch * 2 * sizeof(float));
    const int32_t* dt = h.in(subsets, sizeof(int32_t) * 7 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dF = h.out(F, sizeof(double) * 9 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_fundamental_record* dr = h.out(records, sizeof(mav_fundamental_record) * batch);
    if (dw) h.fetch(pairs_dst, dw + fm_dst_offset(n, batch, p->max_iters), sizeof(double) * 2 * (size_t)n * batch);
    CHK(h.staged());
    CHK(mav_flow_fundamental_dev(c, df, coords, n, batch, p, dt, dF, di, dr, dw, wsb));
    return h.finish();
}
static int epipolar_checked(mav_ctx* c, const float* flow, const double* F, double threshold, int batch, const mav_epipolar_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!flow) return fail(MAV_ERR_ARG, "%s: NULL flow", fn);
    if (!F) return fail(MAV_ERR_ARG, "%s: NULL F", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    if (!std::isfinite(threshold) || threshold < 0.0) return fail(MAV_ERR_ARG, "%s: threshold %g is negative or not finite", fn, threshold);
    return MAV_OK;
}
extern "C" int mav_epipolar_residual_dev(mav_ctx* c, const float* flow, const double* F, double threshold, int batch, float* residual, uint8_t* mask,
                                         mav_epipolar_record* records)
{
    const char* fn = "mav_epipolar_residual_dev";
    CHK(epipolar_checked(c, flow, F, threshold, batch, records, fn));
    if ((uintptr_t)flow % 4) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)F % 8) return fail(MAV_ERR_ARG, "%s: F is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)residual % 4) return fail(MAV_ERR_ARG, "%s: residual is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_epipolar_residual(c->stream, flow, F, threshold * threshold, c->W, c->H, batch, residual, mask, records);
    }
    return check_launch("epipolar residual");
}
extern "C" int mav_epipolar_residual(mav_ctx* c, const float* flow, const double* F, double threshold, int batch, float* residual, uint8_t* mask,
                                     mav_epipolar_record* records)
{
    const char* fn = "mav_epipolar_residual";
    CHK(epipolar_checked(c, flow, F, threshold, batch, records, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const float* df = h.in(flow, sizeof(float) * 2 * batch * c->n0);
    const double* dF = h.in(F, sizeof(double) * 9 * batch);
    float* dr = h.out(residual, sizeof(float) * batch * c->n0);
    uint8_t* dm = h.out(mask, (size_t)batch * c->n0);
    mav_epipolar_record* drec = h.out(records, sizeof(mav_epipolar_record) * batch);
    CHK(h.staged());
    CHK(mav_epipolar_residual_dev(c, df, dF, threshold, batch, dr, dm, drec));
    return h.finish();
}

// ---- robust essential-matrix fit (include/mavflow_essential.h) -----------------------------------------------------------------------------
// As the fundamental fit: every kind of resident state is kept, no device memory of the context's is held; the _dev forms work in the
// caller's workspace (the flow form's gathered pairs included), the host forms in staging blocks behind the last call's.
#include "../../include/mavflow_essential.h"

extern "C" void mav_essential_defaults(mav_essential_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 1.0;
    p->confidence = 0.999;
    p->fx = 1.0;
    p->fy = 1.0;
    p->max_iters = 1000;
}
static int essential_params_checked(int n, const mav_essential_params* p, const char* fn)
{
    if (!p) return fail(MAV_ERR_ARG, "%s: NULL params", fn);
    if (n < 5 || n > MAV_ESSENTIAL_MAX_PAIRS) return fail(MAV_ERR_ARG, "%s: n %d outside [5, %d]", fn, n, MAV_ESSENTIAL_MAX_PAIRS);
    if (p->max_iters < 1 || p->max_iters > MAV_ESSENTIAL_MAX_ITERS)
        return fail(MAV_ERR_ARG, "%s: max_iters %d outside [1, %d]", fn, p->max_iters, MAV_ESSENTIAL_MAX_ITERS);
    if (!std::isfinite(p->threshold) || p->threshold < 0.0) return fail(MAV_ERR_ARG, "%s: threshold %g is negative or not finite", fn, p->threshold);
    if (!(p->confidence > 0.0 && p->confidence < 1.0)) return fail(MAV_ERR_ARG, "%s: confidence %g outside (0, 1)", fn, p->confidence);
    if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || !(p->fx > 0.0) || !(p->fy > 0.0))
        return fail(MAV_ERR_ARG, "%s: camera fx %g, fy %g: not finite or not positive", fn, p->fx, p->fy);
    if (!std::isfinite(p->cx) || !std::isfinite(p->cy)) return fail(MAV_ERR_ARG, "%s: camera cx %g, cy %g: not finite", fn, p->cx, p->cy);
    if (p->flags != 0) return fail(MAV_ERR_ARG, "%s: flags 0x%x: no flag is defined", fn, p->flags);
    return MAV_OK;
}
extern "C" size_t mav_find_essential_workspace_bytes(int n, int batch, const mav_essential_params* p)
{
    if (batch < 1) { fail(MAV_ERR_ARG, "mav_find_essential_workspace_bytes: batch %d is less than 1", batch); return 0; }
    if (essential_params_checked(n, p, "mav_find_essential_workspace_bytes") != MAV_OK) return 0;
    return em_workspace_bytes(n, batch, p->max_iters);
}
// need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 5, max_iters) as the header writes it out
static void essential_need_table(int n, double confidence, int max_iters, int32_t* need)
{
    const double ln = log(1.0 - confidence);
    for (int g = 0; g <= n; g++) {
        if (g < 5) { need[g] = max_iters; continue; }
        const double w = (double)g / (double)n;
        const double w2 = w * w;
        const double den = 1.0 - (w2 * w2) * w;
        if (den < DBL_MIN) { need[g] = 0; continue; }
        const double ld = log(den);
        need[g] = ld >= 0.0 || -ln >= max_iters * (-ld) ? max_iters : (int32_t)nearbyint(ln / ld);
    }
}
// Everything a call can be refused for from its arguments alone, before the context is looked at.  a, b: src and dst, or flow and coords.
static int essential_checked(mav_ctx* c, const void* a, const char* a_name, const void* b, const char* b_name, int n, int batch,
                             const mav_essential_params* p, const int32_t* subsets, const double* E, const double* F, const uint8_t* inliers,
                             const mav_essential_record* records, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!a) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, a_name);
    if (!b) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, b_name);
    if (!subsets) return fail(MAV_ERR_ARG, "%s: NULL subsets", fn);
    if (!E) return fail(MAV_ERR_ARG, "%s: NULL E", fn);
    if (!F) return fail(MAV_ERR_ARG, "%s: NULL F", fn);
    if (!inliers) return fail(MAV_ERR_ARG, "%s: NULL inliers", fn);
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (batch < 1) return fail(MAV_ERR_ARG, "%s: batch %d is less than 1", fn, batch);
    return essential_params_checked(n, p, fn);
}
// what the _dev forms refuse beyond that: a's alignment is `a_align`, b's is checked where b is a device pointer (b_align != 0)
static int essential_dev_checked(const void* a, const char* a_name, size_t a_align, const void* b, const char* b_name, size_t b_align, int n, int batch,
                                 const mav_essential_params* p, const int32_t* subsets, const double* E, const double* F,
                                 const mav_essential_record* records, const void* workspace, size_t workspace_bytes, const char* fn)
{
    if (!workspace) return fail(MAV_ERR_ARG, "%s: NULL workspace", fn);
    if ((uintptr_t)a % a_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, a_name, a_align);
    if (b_align && (uintptr_t)b % b_align) return fail(MAV_ERR_ARG, "%s: %s is not aligned to %zu bytes", fn, b_name, b_align);
    if ((uintptr_t)subsets % 4) return fail(MAV_ERR_ARG, "%s: subsets is not aligned to its 4-byte elements", fn);
    if ((uintptr_t)E % 8) return fail(MAV_ERR_ARG, "%s: E is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)F % 8) return fail(MAV_ERR_ARG, "%s: F is not aligned to its 8-byte elements", fn);
    if ((uintptr_t)records % 16) return fail(MAV_ERR_ARG, "%s: records is not aligned to 16 bytes", fn);
    if ((uintptr_t)workspace % 16) return fail(MAV_ERR_ARG, "%s: workspace is not aligned to 16 bytes", fn);
    const size_t need = em_workspace_bytes(n, batch, p->max_iters);
    if (workspace_bytes < need) return fail(MAV_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return MAV_OK;
}
// the host forms' subsets: every index inside [0, n), no index twice
static int essential_subsets_checked(const int32_t* t, int n, int batch, int max_iters, const char* fn)
{
    for (size_t i = 0; i < (size_t)batch * max_iters; i++) {
        const int32_t* q = t + 5 * i;
        for (int j = 0; j < 5; j++) {
            if (q[j] < 0 || q[j] >= n) return fail(MAV_ERR_ARG, "%s: subsets[%zu][%d] = %d outside [0, %d)", fn, i, j, q[j], n);
            for (int k = 0; k < j; k++)
                if (q[k] == q[j]) return fail(MAV_ERR_ARG, "%s: subsets[%zu] repeats the index %d", fn, i, q[j]);
        }
    }
    return MAV_OK;
}
// the table's copy and the four launches
static int essential_enqueue(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_essential_params* p, const int32_t* subsets,
                             double* E, double* F, uint8_t* inliers, mav_essential_record* records, void* workspace)
{
    std::vector<int32_t> need((size_t)n + 1);             // this call's own block: the copy below has taken its bytes when it returns
    essential_need_table(n, p->confidence, p->max_iters, need.data());
    HIPCHK(hipMemcpyAsync(workspace, need.data(), sizeof(int32_t) * need.size(), hipMemcpyHostToDevice, c->stream));
    EmCall a;
    a.src = src; a.dst = dst; a.subsets = subsets; a.E = E; a.F = F; a.inliers = inliers; a.records = records; a.ws = (char*)workspace;
    a.n = n; a.B = batch; a.max_iters = p->max_iters;
    const double t = p->threshold / ((p->fx + p->fy) / 2.0);
    a.t2 = t * t; a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy;
    { ProfScope ps(c, K_MISC); launch_em_models(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_em_score(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_em_choose(c->stream, a); }
    { ProfScope ps(c, K_MISC); launch_em_finish(c->stream, a); }
    return check_launch("essential fit");
}
extern "C" int mav_find_essential_dev(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_essential_params* p,
                                      const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, void* workspace,
                                      size_t workspace_bytes)
{
    const char* fn = "mav_find_essential_dev";
    CHK(essential_checked(c, src, "src", dst, "dst", n, batch, p, subsets, E, F, inliers, records, fn));
    CHK(essential_dev_checked(src, "src", 8, dst, "dst", 8, n, batch, p, subsets, E, F, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    return essential_enqueue(c, src, dst, n, batch, p, subsets, E, F, inliers, records, workspace);
}
extern "C" int mav_find_essential(mav_ctx* c, const double* src, const double* dst, int n, int batch, const mav_essential_params* p,
                                  const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records)
{
    const char* fn = "mav_find_essential";
    CHK(essential_checked(c, src, "src", dst, "dst", n, batch, p, subsets, E, F, inliers, records, fn));
    CHK(essential_subsets_checked(subsets, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t pairs = sizeof(double) * 2 * (size_t)n * batch, wsb = em_workspace_bytes(n, batch, p->max_iters);
    const double *ds = h.in(src, pairs), *dd = h.in(dst, pairs);
    const int32_t* dt = h.in(subsets, sizeof(int32_t) * 5 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dE = h.out(E, sizeof(double) * 9 * batch);
    double* dF = h.out(F, sizeof(double) * 9 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_essential_record* dr = h.out(records, sizeof(mav_essential_record) * batch);
    CHK(h.staged());
    CHK(mav_find_essential_dev(c, ds, dd, n, batch, p, dt, dE, dF, di, dr, dw, wsb));
    return h.finish();
}
extern "C" int mav_flow_essential_dev(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_essential_params* p,
                                      const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, void* workspace,
                                      size_t workspace_bytes)
{
    const char* fn = "mav_flow_essential_dev";
    CHK(essential_checked(c, flow, "flow", coords, "coords", n, batch, p, subsets, E, F, inliers, records, fn));
    CHK(essential_dev_checked(flow, "flow", 8, coords, "coords", 0, n, batch, p, subsets, E, F, records, workspace, workspace_bytes, fn));
    CHK(check_dev_call(c, batch, fn));
    CHK(affine_coords_checked(c, coords, n, fn));         // the affine flow form's range check of the host coords
    char* ws = (char*)workspace;
    int32_t* dcoords = (int32_t*)(ws + em_coords_offset(n, batch, p->max_iters));
    double *ps = (double*)(ws + em_src_offset(n, batch, p->max_iters)), *pd = (double*)(ws + em_dst_offset(n, batch, p->max_iters));
    HIPCHK(hipMemcpyAsync(dcoords, coords, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    { ProfScope ps_(c, K_MISC); launch_pair_gather(c->stream, flow, dcoords, n, batch, c->W, c->H, ps, pd); }
    CHK(check_launch("pair_gather"));
    return essential_enqueue(c, ps, pd, n, batch, p, subsets, E, F, inliers, records, workspace);
}
extern "C" int mav_flow_essential(mav_ctx* c, const float* flow, const int32_t* coords, int n, int batch, const mav_essential_params* p,
                                  const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, double* pairs_dst)
{
    const char* fn = "mav_flow_essential";
    CHK(essential_checked(c, flow, "flow", coords, "coords", n, batch, p, subsets, E, F, inliers, records, fn));
    CHK(essential_subsets_checked(subsets, n, batch, p->max_iters, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    CHK(affine_coords_checked(c, coords, n, fn));
    const size_t wsb = em_workspace_bytes(n, batch, p->max_iters);
    const float* df = h.in(flow, c->n0 * batch * 2 * sizeof(float));
    const int32_t* dt = h.in(subsets, sizeof(int32_t) * 5 * (size_t)batch * p->max_iters);
    char* dw = h.scratch<char>(wsb);
    double* dE = h.out(E, sizeof(double) * 9 * batch);
    double* dF = h.out(F, sizeof(double) * 9 * batch);
    uint8_t* di = h.out(inliers, (size_t)batch * n);
    mav_essential_record* dr = h.out(records, sizeof(mav_essential_record) * batch);
    if (dw) h.fetch(pairs_dst, dw + em_dst_offset(n, batch, p->max_iters), sizeof(double) * 2 * (size_t)n * batch);
    CHK(h.staged());
    CHK(mav_flow_essential_dev(c, df, coords, n, batch, p, dt, dE, dF, di, dr, dw, wsb));
    return h.finish();
}

// ---- flow pictures (include/mavflow_vis.h) -------------------------------------------------------------------------------------------------
// Like the warps and the resizes these keep every kind of resident state and hold no device memory of the context's: the _dev forms work
// on the caller's blocks alone (the record block is the minimum / maximum pass's scratch) and allocate nothing, the host forms in staging
// blocks behind the last call's (HostCall::beside).
#include "../../include/mavflow_vis.h"

extern "C" int mav_vis_form(int W, int H, int batch, const void* flow, const void* bgr, const void* hsv) { return vis_form(W, H, batch, flow, bgr, hsv); }

// What every call of the family is refused for before the context's device is looked at; a, b: the two pointers every call needs.
static int vis_checked(mav_ctx* c, const void* a, const char* a_name, const void* b, const char* b_name, int batch, const char* fn)
{
    if (!c) return fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!a) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, a_name);
    if (!b) return fail(MAV_ERR_ARG, "%s: NULL %s", fn, b_name);
    if (batch < 1 || batch > c->max_batch) return fail(MAV_ERR_ARG, "%s: batch %d outside [1, %d]", fn, batch, c->max_batch);
    if ((uint64_t)c->n0 * (uint64_t)batch > 0x7FFFFFFFull) return fail(MAV_ERR_ARG, "%s: %d images of %d x %d are more than 2^31 - 1 pixels", fn, batch, c->W, c->H);
    return MAV_OK;
}
static int flow_hsv_checked(mav_ctx* c, const float* flow, int batch, int mode, const uint8_t* bgr, const mav_hsv_record* records, bool dev, const char* fn)
{
    CHK(vis_checked(c, flow, "flow", bgr, "bgr", batch, fn));
    if (!records) return fail(MAV_ERR_ARG, "%s: NULL records", fn);
    if (mode != MAV_HSV_PROCESS && mode != MAV_HSV_DRAW) return fail(MAV_ERR_ARG, "%s: mode %d is neither MAV_HSV_PROCESS nor MAV_HSV_DRAW", fn, mode);
    if (dev && (uintptr_t)flow % 4) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its 4-byte elements", fn);
    if (dev && (uintptr_t)records % 4) return fail(MAV_ERR_ARG, "%s: records is not aligned to 4", fn);
    return MAV_OK;
}
extern "C" int mav_flow_hsv_dev(mav_ctx* c, const float* flow, int batch, int mode, uint8_t* bgr, uint8_t* hsv, mav_hsv_record* records)
{
    const char* fn = "mav_flow_hsv_dev";
    CHK(flow_hsv_checked(c, flow, batch, mode, bgr, records, true, fn));
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        const hipError_t e = launch_flow_hsv(c->stream, flow, c->W, c->H, batch, mode, bgr, hsv, records);
        if (e != hipSuccess) return fail(MAV_ERR_HIP, "%s: zeroing the records failed: %s", fn, hipGetErrorString(e));
    }
    return check_launch("flow_hsv");
}
extern "C" int mav_flow_hsv(mav_ctx* c, const float* flow, int batch, int mode, uint8_t* bgr, uint8_t* hsv, mav_hsv_record* records)
{
    const char* fn = "mav_flow_hsv";
    CHK(flow_hsv_checked(c, flow, batch, mode, bgr, records, false, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch;
    const float* df = h.in(flow, n * 2 * sizeof(float));
    uint8_t* db = h.out(bgr, n * 3);
    uint8_t* dh = h.out(hsv, n * 3);
    mav_hsv_record* dr = h.out(records, sizeof(mav_hsv_record) * batch);
    CHK(h.staged());
    {
        ProfScope ps(c, K_MISC);
        const hipError_t e = launch_flow_hsv(c->stream, df, c->W, c->H, batch, mode, db, dh, dr);
        if (e != hipSuccess) return fail(MAV_ERR_HIP, "%s: zeroing the records failed: %s", fn, hipGetErrorString(e));
    }
    CHK(check_launch("flow_hsv"));
    return h.finish();
}
static int cvt_color_checked(mav_ctx* c, const uint8_t* src, int code, int batch, const uint8_t* dst, const char* fn)
{
    CHK(vis_checked(c, src, "src", dst, "dst", batch, fn));
    if (code != MAV_COLOR_HSV2BGR && code != MAV_COLOR_BGR2HSV && code != MAV_COLOR_BGR2RADIAL)
        return fail(MAV_ERR_ARG, "%s: code %d is none of MAV_COLOR_HSV2BGR, MAV_COLOR_BGR2HSV, MAV_COLOR_BGR2RADIAL", fn, code);
    return MAV_OK;
}
extern "C" int mav_cvt_color_dev(mav_ctx* c, const uint8_t* src, int code, int batch, uint8_t* dst)
{
    const char* fn = "mav_cvt_color_dev";
    CHK(cvt_color_checked(c, src, code, batch, dst, fn));
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_cvt_color(c->stream, src, code, c->W, c->H, batch, dst);
    }
    return check_launch("cvt_color");
}
extern "C" int mav_cvt_color(mav_ctx* c, const uint8_t* src, int code, int batch, uint8_t* dst)
{
    const char* fn = "mav_cvt_color";
    CHK(cvt_color_checked(c, src, code, batch, dst, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch * 3;
    const uint8_t* ds = h.in(src, n);
    uint8_t* dd = h.out(dst, n);
    CHK(h.staged());
    {
        ProfScope ps(c, K_MISC);
        launch_cvt_color(c->stream, ds, code, c->W, c->H, batch, dd);
    }
    CHK(check_launch("cvt_color"));
    return h.finish();
}
static int draw_flow_checked(mav_ctx* c, const uint8_t* img, const float* flow, int batch, int step, const uint8_t* colour, bool dev, const char* fn)
{
    CHK(vis_checked(c, img, "img", flow, "flow", batch, fn));
    if (!colour) return fail(MAV_ERR_ARG, "%s: NULL bgr_colour", fn);
    if (step < 1) return fail(MAV_ERR_ARG, "%s: step %d is less than 1", fn, step);
    if (dev && (uintptr_t)flow % 4) return fail(MAV_ERR_ARG, "%s: flow is not aligned to its 4-byte elements", fn);
    return MAV_OK;
}
extern "C" int mav_draw_flow_dev(mav_ctx* c, uint8_t* img, const float* flow, int batch, int step, float threshold, const uint8_t* bgr_colour)
{
    const char* fn = "mav_draw_flow_dev";
    CHK(draw_flow_checked(c, img, flow, batch, step, bgr_colour, true, fn));
    CHK(check_dev_call(c, batch, fn));
    {
        ProfScope ps(c, K_MISC);
        launch_draw_flow(c->stream, img, flow, c->W, c->H, batch, step, threshold, bgr_colour);
    }
    return check_launch("draw_flow");
}
extern "C" int mav_draw_flow(mav_ctx* c, uint8_t* img, const float* flow, int batch, int step, float threshold, const uint8_t* bgr_colour)
{
    const char* fn = "mav_draw_flow";
    CHK(draw_flow_checked(c, img, flow, batch, step, bgr_colour, false, fn));
    HostCall h(c, fn);
    CHK(h.beside(batch));
    const size_t n = c->n0 * batch;
    uint8_t* di = h.in(img, n * 3);                           // drawn into on the device, and brought back
    const float* df = h.in(flow, n * 2 * sizeof(float));
    h.fetch(img, di, n * 3);
    CHK(h.staged());
    {
        ProfScope ps(c, K_MISC);
        launch_draw_flow(c->stream, di, df, c->W, c->H, batch, step, threshold, bgr_colour);
    }
    CHK(check_launch("draw_flow"));
    return h.finish();
}

// ---- what kernels_shapes.hip's host side needs of a context (mavflow_internal.h) ----------------------------------------------------------
int ctx_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int ctx_enter(mav_ctx* c, int batch, const char* fn, CtxView* out)
{
    CHK(check_dev_call(c, batch, fn));
    *out = CtxView{c->stream, c->W, c->H, c->max_batch};
    return MAV_OK;
}
int ctx_check_launch(const char* what) { return check_launch(what); }
StagedCall::StagedCall(mav_ctx* c, const char* fn) : h(new HostCall(c, fn)) {}
StagedCall::~StagedCall() { delete h; }
int StagedCall::begin(int batch, CtxView* out)
{
    CHK(h->beside(batch));
    *out = CtxView{h->c->stream, h->c->W, h->c->H, h->c->max_batch};
    return MAV_OK;
}
void* StagedCall::in(const void* host, size_t bytes) { return h->in((const char*)host, bytes); }
void* StagedCall::out(void* host, size_t bytes) { return h->out((char*)host, bytes); }
void* StagedCall::inout(void* host, size_t bytes)
{
    char* d = h->in((const char*)host, bytes);
    h->fetch(host, d, bytes);
    return d;
}
void* StagedCall::scratch(size_t bytes) { return h->scratch<char>(bytes); }
int StagedCall::staged() const { return h->staged(); }
int StagedCall::finish() { return h->finish(); }
MiscScope::MiscScope(mav_ctx* c) : p(new ProfScope(c, K_MISC)) {}
MiscScope::~MiscScope() { delete p; }

// ---- the debug frame's pictures on the device (include/mavflow_shapes.h): mav_flow_to_color and mav_last_global_motion_render with
// device outputs and the caller's scratch field; nothing resident is replaced, nothing is waited for
#include "../../include/mavflow_shapes.h"
extern "C" int mav_motion_pictures_dev(mav_ctx* c, const float* flow, int batch, float* field, uint8_t* img_flow, uint8_t* img_warped,
                                       uint8_t* img_global)
{
    const char* fn = "mav_motion_pictures_dev";
    CHK(check_dev_call(c, batch, fn));
    if (!field) return fail(MAV_ERR_ARG, "%s: NULL field", fn);
    if (img_flow && !flow) return fail(MAV_ERR_ARG, "%s: img_flow without flow", fn);
    if ((uintptr_t)flow % 4 || (uintptr_t)field % 4) return fail(MAV_ERR_ARG, "%s: flow and field must be aligned to 4", fn);
    if ((img_warped || img_global) && (!c->gm.last.batch || batch != c->gm.last.batch))
        return fail(MAV_ERR_STATE, "%s: no flow of a %d-item global-motion call is resident", fn, batch);
    if (!img_flow && !img_warped && !img_global) return MAV_OK;
    CHK(ensure_render(c));
    // float32 fields are rendered in numpy's float32 arithmetic, the frame-0 form: the renderer's mode block is made on the device from
    // `batch` bytes of 1 at the head of the caller's field, which is written only afterwards (stream order)
    ProfScope ps(c, K_MISC);
    launch_fill_bytes(c->stream, (uint8_t*)field, 1, (size_t)batch);
    launch_make_derot(c->stream, nullptr, nullptr, (const uint8_t*)field, batch, c->W, c->H, c->render_derot);
    const DerotParams* derot = c->render_derot;
    if (img_flow)
        launch_render_f32(c->stream, flow, derot, nullptr, nullptr, batch, c->W, c->H, mav_thr_params{}, c->render_max, nullptr, img_flow, nullptr);
    const mav_ctx::Motion::Last& l = c->gm.last;
    for (int k = 0; k < 2; k++) {
        uint8_t* img = k == 0 ? img_warped : img_global;
        if (!img) continue;
        launch_motion_pass_a(c->stream, l.flow, l.M, l.m_stride, batch, c->W, c->H, k == 0 ? field : nullptr, nullptr, k == 1 ? field : nullptr, nullptr);
        launch_render_f32(c->stream, field, derot, nullptr, nullptr, batch, c->W, c->H, mav_thr_params{}, c->render_max, nullptr, img, nullptr);
    }
    return check_launch("motion pictures");
}
// a profiled launch section of the JPEG decoder (kernels_jpeg.hip): launch 0 .. 3 = classes jpeg_intervals, jpeg_entropy, jpeg_idct, jpeg_finish
JpegScope::JpegScope(mav_ctx* c, int launch) : p(new ProfScope(c, K_JPEG_INTERVALS + launch)) {}
JpegScope::~JpegScope() { delete p; }

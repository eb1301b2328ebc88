// Internal declarations shared by the host side (mavflow.cpp) and the kernel translation units.
// gfx950 only: wave = 64 lanes, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/mavflow.h"

#define MAV_MAX_POLY_N 16
#define MAV_TILE 32  // flow-iteration tile edge (pixels)

// FarnebackPrepareGaussian output, centre tap first (index k = |offset|).
struct PolyCoef {
    int n;
    float g[MAV_MAX_POLY_N + 1], xg[MAV_MAX_POLY_N + 1], xxg[MAV_MAX_POLY_N + 1];
    float ig11, ig03, ig33, ig55;
};

// GaussianBlur(ksize, sigma) + resize(INTER_LINEAR) of one layer: the f32 Gaussian taps (device memory, getGaussianKernel) and
// the two resize ratios; everything else is arithmetic inside the kernels.
struct BlurParams {
    int ksize;
    int fixed3;          // ksize == 3 with the fixed kernel [1/4, 1/2, 1/4] (sigma == 0)
    const float* g;      // [ksize]
    double scale_x;      // W / w
    double scale_y;      // H / h
    // resize(INTER_LINEAR) coordinates of the layer's w columns and h rows as tables (device memory; built once per context by the host
    // in resize_coord's own arithmetic): source index and weight of the right / lower neighbour.  nullptr: evaluated in the kernel.
    const int* xs; const float* xf;      // [w]
    const int* ys; const float* yf;      // [h]
};

// How the detection kernels treat one pair's float32 flow (what numpy does with it in the reference):
//   PROMOTE   frame index >= 1 with zero rates: flow - 0.0 is the float32 field promoted to double, double arithmetic after it
//   DEROTATE  frame index >= 1: Detector.derotate (detector.py:83-117) in double, evaluated on the fly
//   FRAME0    frame index 0: derotate returns the float32 array itself (detector.py:80-81), float32 arithmetic after it
enum { MAV_PAIR_PROMOTE = 0, MAV_PAIR_DEROTATE = 1, MAV_PAIR_FRAME0 = 2 };
struct DerotParams {  // one pair; Detector.derotate
    double o0, o1, o2, sx, sy;  // sx = w*dt/2, sy = h*dt/2
    int mode;                   // MAV_PAIR_*
};

// Derotated flow vector at pixel (col, row) in double, reference operation order (detector.py:92-114).
static __device__ __forceinline__ void derot_apply(float2 f, const DerotParams* __restrict__ dp, int W, int H, int row, int col,
                                                   double* fu, double* fv)
{
    double u = (double)f.x, v = (double)f.y;
    if (dp && dp->mode == MAV_PAIR_DEROTATE) {
        const double x = -((double)col / (double)W - 0.5) * 2.0;
        const double y = -((double)row / (double)H - 0.5) * 2.0;
        const double o0 = dp->o0, o1 = dp->o1, o2 = dp->o2;
        double du = (((o0 * x) * y - o1 * (x * x)) - o1) + o2 * y;
        double dv = ((((-o2) * x + o0) + o0 * (y * y))) - (o1 * x) * y;
        du = du * dp->sx;
        dv = dv * dp->sy;
        u = u - du;
        v = v - dv;
    }
    *fu = u; *fv = v;
}
static __device__ __forceinline__ void derot_apply(double2 f, const DerotParams*, int, int, int, int, double* fu, double* fv)
{
    *fu = f.x; *fv = f.y;
}

// Several layers in one launch (a small group's whole pyramid): job tables passed by value in the kernel arguments.
#define MAV_MAX_JOBS 6
struct PolyJob { const float* I; float* R; size_t I_stride, R_stride; int w, h, tiles_x, per_img, first_block, fast; };
struct PolyJobs { int n, pad; PolyJob j[MAV_MAX_JOBS]; };

// ---- flow kernels (kernels_flow.hip) ----------------------------------------------------------------------
// All take G slots; slot s reads/writes base + s*stride (strides in elements).
// The frames of a layer-image launch: G images of W x H from two runs, the first `split` from img, the rest from img2 (same stride);
// img2 == nullptr: one run.  T = uint8_t, uint16_t or float (the three source depths, instantiated in kernels_flow.hip; esize = sizeof(T)).
template <typename T>
struct FrameRun {
    const T *img, *img2;
    int split;
    size_t img_stride;
    int G, W, H;
    FrameRun runs() const { return img2 ? *this : FrameRun{img, img, G, img_stride, G, W, H}; }   // "one run" spelled as two: what the kernels take
};
// One layer's image of those frames: w x h, slot s at out + s * out_stride.  (The head of a BlurJob: the kernel argument's layout.)
struct LayerTarget { float* out; size_t out_stride; BlurParams bp; int w, h; };
struct BlurJob : LayerTarget { int fused, gx, gy, first_block, rows_cap, pitch_w, th, pad; };
struct BlurJobs { int n, pad; BlurJob j[MAV_MAX_JOBS]; };
// the separable two-pass form's scratch (G x H x w floats, slot stride `stride`); two_pass: take that form even for a layer that would be
// fused (the stage hook compares the two forms).  Layers with a short Gaussian (blur_resize_is_fused) never touch tmp otherwise.
struct BlurScratch { float* tmp; size_t stride; bool two_pass = false; };
template <typename T>
void launch_blur_resize(hipStream_t st, const FrameRun<T>& f, const LayerTarget& t, const BlurScratch& scratch);
bool blur_resize_is_fused(int W, int H, int w, int h, int ksize, int esize = 1);
template <typename T>
bool blur_resize_needs_tmp(const FrameRun<T>& f, const LayerTarget& t);
void launch_polyexp(hipStream_t st, const float* I, size_t I_stride, int G, int w, int h, const PolyCoef& pc, float* R,
                    size_t R_stride);
// jobs.j[i]: I, R, I_stride, R_stride, w, h filled by the caller; G images per job
void launch_polyexp_multi(hipStream_t st, PolyJobs jobs, int G, const PolyCoef& pc);
template <typename T>
bool blur_multi_ok(const FrameRun<T>& f, const LayerTarget& t);
// jobs.j[i]: the LayerTarget filled by the caller, for layers blur_multi_ok accepts.  More than 8 frames (the deep layers of a whole
// call): one launch per tile code (fused_path_of) instead of one for all jobs.
template <typename T>
void launch_blur_multi(hipStream_t st, const FrameRun<T>& f, BlurJobs jobs);

// G pairs of one w x h layer: their expansions R0 / R1, (h, w, 5) each -- the five values of a pixel lie together.
struct PairOperands { const float *R0, *R1; size_t R_stride; int G, w, h; };
// The stage hooks keep their host contract of five planes (include/mavflow.h) and transpose at the edge, on the host copy, so that no
// launch is added.  The staged copy must live until the call's finish() has returned.
inline std::vector<float> expansion_of_planes(const float* planes, size_t n)
{
    std::vector<float> e(planes ? 5 * n : 0);
    for (size_t c = 0; c < 5 && planes; c++)
        for (size_t i = 0; i < n; i++) e[5 * i + c] = planes[c * n + i];
    return e;
}
// rc: what the call's finish() returned; the planes are written only when it succeeded
inline int planes_of_expansion(int rc, const std::vector<float>& e, size_t n, float* planes)
{
    for (size_t c = 0; c < 5 && rc == MAV_OK; c++)
        for (size_t i = 0; i < n; i++) planes[c * n + i] = e[5 * i + c];
    return rc;
}
// Where a layer's initial flow comes from: nowhere (zero flow: the top layer), the coarser layer's field (pw x ph; resize(INTER_LINEAR)
// to the layer's size times mul, evaluated inside the kernel and never written) or a field of the layer's own size (the stage hook; the
// top layer of a call with OPTFLOW_USE_INITIAL_FLOW).  kind = k_update_matrices' MODE.
struct FlowSource {
    enum Kind { ZERO = 0, COARSER = 1, FIELD = 2 };
    Kind kind = ZERO;
    const float* flow = nullptr;
    size_t stride = 0;
    int pw = 0, ph = 0;
    float mul = 0.f;
    static FlowSource coarser(const float* flow, size_t stride, int pw, int ph, float mul)      // flow == nullptr: zero
    {
        return flow ? FlowSource{COARSER, flow, stride, pw, ph, mul} : FlowSource{};
    }
    static FlowSource field(const float* flow, size_t stride) { return FlowSource{FIELD, flow, stride}; }
    FlowSource from_pair(int s0) const { FlowSource u = *this; if (u.flow) u.flow += (size_t)s0 * stride; return u; }
};
// The initial M (FarnebackUpdateMatrices on the source's flow) of pixel rows [y_begin, y_end) of the pairs; y_end < 0 = to the bottom.
struct InitialMArgs : PairOperands {
    float* M;
    size_t M_stride;
    int y_begin = 0, y_end = -1;
};
void launch_initial_m(hipStream_t st, const InitialMArgs& a, const FlowSource& src);
// The Gaussian window of the sweep (OPTFLOW_FARNEBACK_GAUSSIAN): taps k[0..m], m = winsize / 2, as gauss_taps() computes them on the host.
#define MAV_MAX_WIN_HALF 32                     // winsize <= 64 (mav_create)
struct GaussTaps { float k[MAV_MAX_WIN_HALF + 1]; };
void gauss_taps(int winsize, GaussTaps* out);
// One sweep launch (k_blur_iter_*): M_in -> flow and, with do_update, M_out.  launch_blur_iter and blur_iter_bands_ok take the same
// object, so the predicate answers for the operands that are launched.
struct SweepArgs : PairOperands {
    const float* M_in;
    float* M_out;
    size_t M_stride;
    int winsize;
    float* flow;
    size_t f_stride;
    int do_update, store_flow;            // store_flow == 0: the sweep's flow is consumed inside the kernel only (valid when do_update != 0)
    int ty0 = 0, ty1 = -1;                // tile rows [ty0, ty1) of 16 pixel rows; ty1 < 0 = the whole layer
    int strip = 0;                        // width in tiles of the tile order's column strips; 0 = automatic
    bool write_through = false;           // M' through sc1 stores: see k_blur_iter_fast
    const GaussTaps* gauss = nullptr;     // OPTFLOW_FARNEBACK_GAUSSIAN: the window's taps; nullptr = box window
};
void launch_blur_iter(hipStream_t st, const SweepArgs& a);
int blur_iter_tile_rows(int h);                 // 16-pixel tile rows of a layer of height h
// band launches (ty0 / ty1) are honoured only by the fast sweep kernel: true when launch_blur_iter will take it for these operands
bool blur_iter_bands_ok(const SweepArgs& a);
size_t blur_iter_lds_bytes(int winsize);
const char* blur_iter_prepare(int winsize);   // grants the general sweep kernels (both windows) their dynamic LDS on the current device

void launch_probe_r3w1(hipStream_t st, const float* a, const float* b, const float* c, float* d, size_t n_float4);   // calibration

// ---- detection kernels (kernels_detect.hip, compiled with -ffp-contract=off) --------------------------------
struct FoeScratch {
    double* cand;                  // [B][N][2] compacted candidates
    int* count;                    // [B]
    unsigned long long* best_key;  // [B]
    unsigned* done;                // [B][2] tickets: [0] workgroups of the vote that have finished, [1] of the phi kernel (both self-resetting)
};
// FlowT = float (optionally derotated on the fly) or double (already derotated).
void launch_foe_f32(hipStream_t st, const float* flow, const DerotParams* derot /*dev, [B] or null*/, const uint32_t* samples,
                    int B, int W, int H, int N, double mag2_thr, float mag2_thr_f32 /* frame-0 pairs */, double dist2_thr,
                    FoeScratch s, double* foe, int32_t* box_acc /* nullable: the pair's accumulators are initialised here too */,
                    unsigned long long* max_phi_bits /* nullable */);
void launch_foe_f64(hipStream_t st, const double* flow, const uint32_t* samples, int B, int W, int H, int N, double mag2_thr,
                    double dist2_thr, FoeScratch s, double* foe, int32_t* box_acc, unsigned long long* max_phi_bits);
// box_acc: [B][4] int32 accumulators (x0 min, y0 min, x1 max, y1 max), initialised by launch_box_init or by launch_foe_*.
void launch_box_init(hipStream_t st, int32_t* box_acc, unsigned long long* max_phi_bits, unsigned* done /* FoeScratch::done or null */, int B);
// How a phi launch ends and is tuned: results / box_out (either may be null) are written by the pair's last workgroup (needs done).
struct PhiLaunch {
    unsigned* done = nullptr;
    mav_result* results = nullptr;
    int32_t* box_out = nullptr;
    bool screen = true;      // option "phi_screen"
    int yloop = 0;           // option "phi_yloop" (0 = automatic)
};
void launch_phi_mask_f32(hipStream_t st, const float* flow, const DerotParams* derot, const double* foe, const uint8_t* sky,
                         int B, int W, int H, mav_thr_params thr, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                         int32_t* box_acc, unsigned long long* max_phi_bits, const PhiLaunch& pl);
void launch_phi_mask_f64(hipStream_t st, const double* flow, const double* foe, const uint8_t* sky, int B, int W, int H,
                         mav_thr_params thr, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, int32_t* box_acc,
                         unsigned long long* max_phi_bits, const PhiLaunch& pl);
void launch_box_finalize(hipStream_t st, const int32_t* box_acc, int B, int32_t* box);
void launch_derotate(hipStream_t st, const float* flow, const DerotParams* derot, int B, int W, int H, double* out);
void launch_bbox_u8(hipStream_t st, const uint8_t* img, int B, int W, int H, int* maxv /*[B] scratch*/, int32_t* box_acc);
void launch_window_max(hipStream_t st, const uint8_t* img, int B, int W, int H, unsigned long long* key /*[B]*/,
                       int64_t* out);
void launch_tpr_fpr(hipStream_t st, const uint8_t* gt, const uint8_t* mask, unsigned mask_value, int B, int W, int H,
                    unsigned long long* counts /*[B][4]*/);
// one pass over gt for one mask (mask1 = counts1 = nullptr) or two; gt_stride = 0: one ground-truth image for every pair
void launch_tpr_fpr2(hipStream_t st, const uint8_t* gt, size_t gt_stride, const uint8_t* mask0, const uint8_t* mask1, unsigned mask_value, int B,
                     int W, int H, unsigned long long* counts0 /*[B][4]*/, unsigned long long* counts1 /*[B][4]*/);
// Threshold sweep (mav_roc_sweep): the checked lists of one call, passed to the kernel by value.  ang32 / mag32: the thresholds rounded
// to float32 (what a frame-0 pair compares against); mag0_sq_lo <= mag[0]^2 (rounded down on the host): a double pair with
// u*u + v*v below it passes no magnitude gate and needs no square root.
struct RocThr {
    int ka, km;
    double mag0_sq_lo;
    double ang[MAV_ROC_MAX_ANGLES], mag[MAV_ROC_MAX_MAGS];
    float ang32[MAV_ROC_MAX_ANGLES], mag32[MAV_ROC_MAX_MAGS];
};
// table: B x MAV_ROC_TABLE_WORDS(ka, km) int64 (zeroed here); gt_stride = 0: one ground-truth image for every pair
// flow: float32 (derot says how each pair is treated) or, with f64, an already derotated float64 field (derot is not read)
// returns the table fill's error, if any (nothing is launched then)
hipError_t launch_roc_sweep(hipStream_t st, const void* flow, bool f64, const DerotParams* derot /*dev, [B] or null*/, const double* foe,
                      const uint8_t* sky, const uint8_t* gt, size_t gt_stride, int B, int W, int H, const RocThr& thr, unsigned long long* table);
void launch_bgr2gray(hipStream_t st, const uint8_t* bgr, size_t n, uint8_t* gray);
void launch_ransac_only(hipStream_t st, FoeScratch s, int M, int N, double dist2_thr, double* foe);
void launch_make_derot(hipStream_t st, const double* omega /*null: no rotation*/, const double* dt, const uint8_t* frame0, int B,
                       int W, int H, DerotParams* out);
// Result images (BGR u8, (B, H, W, 3) each, any may be null): the fixed-mask image, flow_to_color of the derotated flow and the JET
// colour map of phi.  radmax: [B] scratch.  foe / thr are read only for the result and phi images.
void launch_render_f32(hipStream_t st, const float* flow, const DerotParams* derot, const double* foe, const uint8_t* sky, int B, int W,
                       int H, mav_thr_params thr, unsigned long long* radmax, uint8_t* res, uint8_t* flow_img, uint8_t* phi_img);
// flow_to_color of an already derotated float64 field
void launch_render_f64(hipStream_t st, const double* flow, int B, int W, int H, unsigned long long* radmax, uint8_t* flow_img);
void launch_colormap_jet(hipStream_t st, const uint8_t* gray, size_t n, uint8_t* bgr);
// The processed.mp4 frame: frames (B, H, W, 3) BGR, fixed masks (B, H, W), FoE and ground-truth FoE (B, 2) each -> out (B, H, W, 3)
// and written[B] (zeroed here, then set by the kernel).  radius in [0, MAV_OVERLAY_MAX_RADIUS].
void launch_overlay(hipStream_t st, const uint8_t* frames, const uint8_t* mask, const double* foe, const double* foe_gt, int B, int W, int H,
                    int radius, uint8_t* out, uint8_t* written);

// ---- window search (kernels_window.hip, compiled with -ffp-contract=off) -----------------------------------------
#define MAV_PYR_MAX 32
// Levels of analyze_pyramid for one frame size: dims, first window index of each level in the reference's scan order
// (base[n] = total), and the byte offset of a level's image block (levels >= 1, batch images back to back) in the workspace.
struct PyrPlan {
    int n;
    int w[MAV_PYR_MAX], h[MAV_PYR_MAX];
    unsigned base[MAV_PYR_MAX + 1];
    size_t off[MAV_PYR_MAX];
};
void launch_area_resize(hipStream_t st, const uint8_t* src, size_t src_stride, int sw, int sh, uint8_t* dst, size_t dst_stride,
                        int dw, int dh, int B);
// OPTFLOW_USE_INITIAL_FLOW: B float2 fields sw x sh -> dw x dh (cv2.resize INTER_AREA, fast or general path as OpenCV picks it), times
// `scale` (flow *= scale).  dw <= sw, dh <= sh; strides in floats.
void launch_area_resize_flow(hipStream_t st, const float* src, size_t src_stride, int sw, int sh, float* dst, size_t dst_stride, int dw,
                             int dh, int B, double scale);
void launch_level_scan(hipStream_t st, const uint8_t* img, size_t stride, int B, int W, int H, unsigned idx_base,
                       unsigned long long* key /*[B], zeroed by the caller*/);
void launch_pyramid_finalize(hipStream_t st, const unsigned long long* key, const PyrPlan& plan, const uint8_t* img0,
                             const uint8_t* ws, int B, int64_t* out /*[B][6]*/);
void launch_optimize_window(hipStream_t st, const uint8_t* img, int B, int W, int H, unsigned long long* sat /*[B][(H+1)(W+1)]*/,
                            const int32_t* win_in, int64_t* score, int32_t* win_out);

// ---- PNG encoder (kernels_png.hip) ------------------------------------------------------------------------------------
// An image's scanline stream (per row the filter byte + W * C bytes) is deflated in independent segments of MAV_PNG_SEG bytes, one
// workgroup each; a segment costs at most its length + 5 bytes (the stored form) and is built in a slot of MAV_PNG_SLOT bytes.
#define MAV_PNG_SEG 24576
#define MAV_PNG_SLOT (MAV_PNG_SEG + 16)
size_t png_segments(size_t raw);                 // segments of a scanline stream of `raw` bytes
size_t png_workspace_per_image(size_t raw);      // device bytes launch_png_encode needs per image of a launch chain
// images img0 .. img0 + nimg - 1 of `imgs` ((H, W, C) u8 each; C = 1 gray, 3 BGR, 4 BGRA) -> their zlib streams, packed into `out`
// behind the streams of the images before them; index[i] = (offset, size) of image i.  index[img0 - 1] must be complete (same stream).
void launch_png_encode(hipStream_t st, const uint8_t* imgs, int img0, int nimg, int W, int H, int C, uint8_t* ws, uint8_t* out,
                       unsigned long long* index);

// ---- sparse optical flow (kernels_lk.hip, compiled with -ffp-contract=off) -----------------------------------------------------------
// Levels of the tracker's pyramid for one frame size (level l + 1 = ((w + 1) / 2, (h + 1) / 2)); off[l]: first element of level l
// inside a frame's u8 pyramid block and inside the int16-pair derivative block.
#define MAV_LK_MAX_LEVELS 8
#define MAV_LK_HIST 104           // iteration-count histogram: bins 0 .. 102 iterations, last bin = more
struct LkLevels { int n; int w[MAV_LK_MAX_LEVELS], h[MAV_LK_MAX_LEVELS]; unsigned off[MAV_LK_MAX_LEVELS]; };
struct LkTrackArgs {
    const uint8_t *I, *J;         // pyramid blocks of the previous / next frame
    const short2* D;              // Scharr pairs of the previous frame's levels
    LkLevels lv;                  // n = levels in use
    const float* pts;             // (n, 2)
    int n, win_w, win_h, max_count;
    double eps2;                  // epsilon^2
    float min_eig;
    float* out;                   // (n, 2)
    uint8_t* status;              // (n)
    unsigned* iter_hist;          // [MAV_LK_HIST] or null: iterations per (point, level) that reached the loop
    const int* n_dev;             // null, or the device's own point count: min(*n_dev, n) points run, none if it is negative
};
// the tracker's second form: cv2's `err` output and flags (kernels_lk.hip LkErr).  With USE_INITIAL_FLOW `out` is read before it is written.
struct LkTrackErrArgs : LkTrackArgs {
    float* err;                   // (n) or null
    int flags;                    // MAV_OPTFLOW_USE_INITIAL_FLOW | MAV_OPTFLOW_LK_GET_MIN_EIGENVALS
};
struct LkPickArgs {
    const uint2* cand;            // sorted candidates (value bits, linear index)
    const unsigned* n_ptr;        // their count; > cap: overflow
    unsigned cap;
    int W, max_corners;
    int pick;                     // 0: min_distance < 1, no distance test
    int cell, gw, gh, slots;      // the grid of accepted corners: gw x gh cells of cell x cell pixels, `slots` words each
    double md2;                   // min_distance^2
    unsigned* grid;               // gw * gh * slots words, zeroed by the caller
    float* corners;               // (max_corners, 2); entries from *count on are left alone
    int* count;                   // accepted corners, or -(candidates) on overflow
    unsigned* stats;              // [0] chunks, [1] rounds of this pick
};
// min-eigenvalue map of a W x H u8 image (block_size odd, <= 15) and its maximum as an ordered key (*maxkey zeroed by the caller)
// mask (H, W) u8 or null: only pixels with a non-zero mask byte enter the maximum (and become candidates below)
void launch_min_eig(hipStream_t st, const uint8_t* img, const uint8_t* mask, int W, int H, int block_size, float s2, float* eig, unsigned* maxkey);
// the same map with the Harris response (a c - b b) - (k (a + c)) (a + c) as the score
void launch_harris(hipStream_t st, const uint8_t* img, const uint8_t* mask, int W, int H, int block_size, float s2, float k, float* eig,
                   unsigned* maxkey);
// candidates (value bits, linear index) appended at cand[*count++] while *count < cap (*count zeroed by the caller, counts past cap)
void launch_corner_candidates(hipStream_t st, const float* eig, const uint8_t* mask, int W, int H, const unsigned* maxkey, double quality,
                              uint2* cand, unsigned* count, unsigned cap);
// in-place descending sort of cand[0 .. *n_ptr) by (value bits << 32) | index (cap: a power of two, the buffer's size), then the pick;
// neither needs the host to know *n_ptr
void launch_pick_sort(hipStream_t st, uint2* cand, const unsigned* n_ptr, unsigned cap);
void launch_corner_pick(hipStream_t st, const LkPickArgs& a);
void launch_lk_pyrdown(hipStream_t st, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh);
void launch_lk_scharr(hipStream_t st, const uint8_t* pyr, const LkLevels& lv, int levels, short2* out);
size_t lk_track_lds_bytes(int win_w, int win_h);
void launch_lk_track(hipStream_t st, const LkTrackArgs& a);
void launch_lk_track_err(hipStream_t st, const LkTrackErrArgs& a);

// ---- global-motion subtraction (kernels_motion.hip, compiled with -ffp-contract=off) ----------------------------------------------------
// src[b][i] = coords[i], dst[b][i] = coords[i] + flow[b][y_i][x_i], (B, n, 2) float64 each; coords (n, 2) int32 (x, y) on the device
void launch_pair_gather(hipStream_t st, const float* flow, const int32_t* coords, int n, int B, int W, int H, double* src, double* dst);
// the fit of B items of n pairs: work = homography_work_doubles(n) doubles per item; H (B, 9), ok (B)
size_t homography_work_doubles(int n);
void launch_homography_fit(hipStream_t st, const double* src, const double* dst, int n, int B, double* work, double* H, int* ok);
// M: item b's six entries at M + b * m_stride.  Pass A: key[b] (zeroed by the caller, or null) = (float bits of the largest residual
// magnitude << 32) | ~(its first pixel index); warped / gm (B, H, W, 2) and mag (B, H, W) float32, each nullable.  Pass B: gray (B, H, W).
void launch_motion_pass_a(hipStream_t st, const float* flow, const double* M, int m_stride, int B, int W, int H, float* warped, float* mag,
                          float* gm, unsigned long long* key);
void launch_motion_pass_b(hipStream_t st, const float* flow, const double* M, int m_stride, int B, int W, int H, const unsigned long long* key,
                          uint8_t* gray);
void launch_motion_window(hipStream_t st, const int64_t* pyr, int B, int32_t* win);
void launch_motion_pack(hipStream_t st, const unsigned long long* key, const int64_t* pyr, const int32_t* win, const int64_t* opt_score,
                        const int32_t* opt_win, const int* ok, int B, int W, mav_motion_result* out);

// ---- connected components (kernels_components.hip, integer arithmetic only) -----------------------------------------------------------
// B images of W x H from `mask`; ws: B * cc_workspace_per_image bytes; labels nullable; counts (B), blobs (B, max_blobs: zeroed by the caller).
struct CcArgs {
    const uint8_t* mask;
    int B, W, H, connectivity, min_area, max_blobs;
    void* ws;
    int32_t* labels;
    mav_cc_counts* counts;
    mav_blob* blobs;
};
size_t cc_workspace_per_image(int W, int H);
void launch_components(hipStream_t st, const CcArgs& a);

// ---- flow history (kernels_history.hip, compiled with -ffp-contract=off) ----------------------------------------------------------------
// The slots a push walks, in order (mav_history_schedule): at most MAV_HISTORY_MAX_LENGTH - 1 entries of one byte, four to a word, passed
// to the kernel by value.
struct HistSlots { int n; unsigned w[(MAV_HISTORY_MAX_LENGTH + 3) / 4]; };
// one remap of a W x H field of pairs (float32 or, with f64, float64) at the float32 maps: out (H, W, 2) float64
void launch_remap_linear(hipStream_t st, const void* src, bool f64, const float* map_x, const float* map_y, int W, int H, double* out);
// a caller's field (aligned to its element) -> a ring slot, copied or widened (float64 into a float32 slot does not exist)
void launch_history_put(hipStream_t st, const void* src, bool src_f64, void* slot, bool ring_f64, int W, int H);
// every pixel's trajectory through the listed slots of the ring (slot s at ring + s * W * H pairs): out (H, W, 2) float64 (r - y, c - x),
// or with out_f32 float32 (c - x, r - y); out is aligned to its element
void launch_history_trace(hipStream_t st, const void* ring, bool ring_f64, const HistSlots& slots, int W, int H, bool axes_xy, bool out_f32, void* out);

// ---- ground truth and radial error (kernels_truth.hip, compiled with -ffp-contract=off; include/mavflow_truth.h) -------------------------
#define MAV_GT_FLOW_GRID_CAP 1024u     // workgroups of 256 pixels per pair; larger frames loop
// depth (B, H, W) float32, seg (B, H, W) u8 or null, params: B blocks on the device; out (B, H, W, 2) float32 or, with out_f64, float64,
// aligned to one pair
void launch_gt_flow(hipStream_t st, const float* depth, const uint8_t* seg, const void* params /* mav_gt_flow_params[B] */, int B, int W, int H,
                    bool out_f64, void* out);
// One checked edge list of a histogram call, passed to a kernel by value (the same bound as MAV_RADIAL_MAX_EDGES).
struct RadialEdges { int n, pad; double e[257]; };
#define MAV_RADIAL_LDS_CELLS 32768     // cells a workgroup can count in LDS (128 KiB of the CU's 160 beside the edge lists): more go to the table directly
#define MAV_RADIAL_GRID_CAP 256        // workgroups of 1024 threads in all pairs of a call: one per CU, which is what the LDS form's counters leave room for
bool radial_hist_lds_counts(int nm, int ne);
int radial_hist_grid(size_t npx, int B);
// flow, gt (B, H, W, 2) float32 aligned to 8, sky (B, H, W) u8 or null; edges_dev: 2 * 257 doubles of the context's, written here first
// unless edges_resident (the stream's last call left these very lists there); table: 2 + cells words, ADDED into.  Returns the error
// of granting the LDS, if any (nothing is launched then).
hipError_t launch_radial_hist(hipStream_t st, const float* flow, const float* gt, const uint8_t* sky, int B, int W, int H, const RadialEdges& mag,
                              const RadialEdges& err, double* edges_dev, bool edges_resident, unsigned long long* table);

// ---- validation tail (kernels_validation.hip, compiled with -ffp-contract=off; include/mavflow_validation.h) -----------------------------
#define MAV_GT_STATS_GRID_CAP 2048u    // workgroups of 256 pixels per image in the maxima's launch; larger frames loop
// One image's accumulators between the phases: the head of the call's scratch, B of them; then (B, H) int32 row counts; then, when
// the caller wants the flow sum but no index list, the (B, max_pixels) list of the call's own.
struct GtsAcc { unsigned long long drone, pos, tp, fp; int seg_max; unsigned depth_key, nan; int pad; int box[4]; };
static_assert(sizeof(GtsAcc) == 64, "GtsAcc");
inline size_t gts_rows_offset(int B) { return sizeof(GtsAcc) * (size_t)B; }
inline size_t gts_list_offset(int B, int H) { return gts_rows_offset(B) + ((sizeof(int) * (size_t)B * H + 15) & ~(size_t)15); }
size_t gt_stats_scratch_bytes(int B, int H, int max_pixels, bool own_list);
// What one call reads and writes, all device pointers: seg, sky (B, H, W) u8, depth (B, H, W) float32 aligned to 4, gt_flow (B, H, W, 2)
// float32 aligned to 8 (sky, depth, gt_flow may be null), params: B mav_gt_stats_params, records: B mav_gt_stats_record, indices
// (B, max_pixels) int32 or null, scratch: gt_stats_scratch_bytes(B, H, max_pixels, gt_flow && !indices) bytes aligned to 16.
struct GtStatsCall {
    const uint8_t *seg, *sky; const float *gt_flow, *depth; const void* params; int B, W, H, max_pixels; void* scratch; void* records; int32_t* indices;
};
enum { GTS_PHASE_MAX, GTS_PHASE_COUNT, GTS_PHASE_LIST, GTS_PHASE_SUM, GTS_PHASES };
// one phase's launches (the phases of a call in this order, on one stream)
void launch_gt_stats_phase(hipStream_t st, int phase, const GtStatsCall& k);

// ---- k-means clustering (kernels_cluster.hip, compiled with -ffp-contract=off; include/mavflow_cluster.h) --------------------------------
#define KM_THREADS 256
#define KM_PER_THREAD 16                // KM_THREADS * KM_PER_THREAD = MAV_KMEANS_CHUNK
#define KM_GRID_CAP 1024u               // workgroups per image in the full-frame launches; more chunks are strode over
// One image's control block at the head of its part of the workspace: everything the launches decide lives here.
struct KmState {
    double S[16][16][4];                // [attempt][cluster][component]
    double shift[16], compact[16];
    unsigned long long key[16];         // the repair's argmax: dist bits << 32 | sample index
    float c[16][16][4];
    float mean[16][4];                  // the donor's mean of the repair in hand
    int n[16][16];
    int done[16], iters[16], repairs[16], pending[16], donor[16];   // pending: the empty cluster being repaired, or -1
    int live, any_pending, best, skipped;
};
// What one call works on, all device pointers; the workspace layout follows from (n, B, A, K, D) alone.
struct KmCall {
    const void* samples; const float* init; int32_t* labels; float* centers; void* records; char* ws;
    int n, B, A, K, D, u8, max_iter; double eps2;
};
inline size_t km_chunks(int n) { return ((size_t)n + KM_THREADS * KM_PER_THREAD - 1) / (KM_THREADS * KM_PER_THREAD); }
inline size_t km_state_bytes() { return (sizeof(KmState) + 255) & ~(size_t)255; }
inline size_t km_labels_bytes(int n, int A) { return ((size_t)A * n + 255) & ~(size_t)255; }            // uint8 (A, n)
inline size_t km_slab_bytes(int n, int A, int K, int D) { return sizeof(double) * km_chunks(n) * A * K * (D + 1); }
inline size_t km_image_bytes(int n, int A, int K, int D) { return km_state_bytes() + km_labels_bytes(n, A) + ((km_slab_bytes(n, A, K, D) + 255) & ~(size_t)255); }
// the whole launch sequence of a call
void launch_kmeans(hipStream_t st, const KmCall& k);
void launch_kmeans_paint(hipStream_t st, const int32_t* labels, const float* centers, int n, int B, int K, int D, uint8_t* res, uint8_t* mask);

// ---- image warps (kernels_warp.hip, compiled with -ffp-contract=off; include/mavflow_warp.h) ---------------------------------------------
// the coordinate policies of the one sampling body
enum { WARP_POLICY_MAP, WARP_POLICY_PLANES, WARP_POLICY_FLOW, WARP_POLICY_AFFINE, WARP_POLICY_PERSPECTIVE };
// a, b: the policy's operands (map_xy | map_x, map_y | flow | M); B images of W x H in `format` (MAV_WARP_*), one launch
void launch_warp(hipStream_t st, int policy, int format, const void* src, const void* a, const void* b, int flags, int W, int H, int B, void* dst);
// Detector.warp_method: records' initialisation, the pass and the records' final form, three launches; diff and mag may be NULL
void launch_warp_method(hipStream_t st, int policy, const float* flow, const double* M, int W, int H, int B, float* diff, float* mag, void* records);

// ---- image resize (kernels_resize.hip, compiled with -ffp-contract=off; include/mavflow_resize.h) ------------------------------------------
// the forms of the one body, as cv::resize's dispatch picks them (RS_AREA_2X2: uint8 alone)
enum { RS_COPY, RS_NEAREST, RS_LINEAR, RS_AREA_2X2, RS_AREA_FAST, RS_AREA_GENERAL };
int resize_form(int format, int sw, int sh, int dw, int dh, int interpolation, int* ix, int* iy);
bool resize_vector_stores(int format, int dw, const void* dst, bool sky);
// B images of sw x sh in `format` (MAV_WARP_*) -> dw x dh, one launch
void launch_resize(hipStream_t st, int format, const void* src, int sw, int sh, int dw, int dh, int interpolation, int B, void* dst);
// resize(U8C3, INTER_LINEAR) + key in one launch: sky (B, dh, dw) uint8, 1 where channels 0 and 1 equal the keys
void launch_sky_mask(hipStream_t st, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int B, uint8_t* sky);

// ---- robust affine fit (kernels_affine.hip, compiled with -ffp-contract=off; include/mavflow_affine.h) ------------------------------------
// What one call works on, all device pointers.  The workspace layout follows from (n, B, max_iters) alone: need[] (n + 1 int32, filled by
// the host's copy), the counts (B, max_iters) int32 (-1: an invalid hypothesis), the choice (B, 4) int32, then the flow form's coords
// (n, 2) int32 and its gathered pairs, src and dst (B, n, 2) float64 each.
struct AffCall {
    const double *src, *dst; const int32_t* triples; double* M; uint8_t* inliers; void* records; char* ws;
    int n, B, max_iters, refine; double t2;
};
__host__ __device__ inline size_t aff_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
__host__ __device__ inline size_t aff_counts_offset(int n) { return aff_round(sizeof(int32_t) * ((size_t)n + 1)); }
__host__ __device__ inline size_t aff_choice_offset(int n, int B, int max_iters) { return aff_counts_offset(n) + aff_round(sizeof(int32_t) * (size_t)B * max_iters); }
__host__ __device__ inline size_t aff_coords_offset(int n, int B, int max_iters) { return aff_choice_offset(n, B, max_iters) + aff_round(sizeof(int32_t) * 4 * (size_t)B); }
__host__ __device__ inline size_t aff_src_offset(int n, int B, int max_iters) { return aff_coords_offset(n, B, max_iters) + aff_round(sizeof(int32_t) * 2 * (size_t)n); }
__host__ __device__ inline size_t aff_dst_offset(int n, int B, int max_iters) { return aff_src_offset(n, B, max_iters) + aff_round(sizeof(double) * 2 * (size_t)n * B); }
__host__ __device__ inline size_t aff_workspace_bytes(int n, int B, int max_iters) { return aff_dst_offset(n, B, max_iters) + aff_round(sizeof(double) * 2 * (size_t)n * B); }
// the three launches of a call, in this order on one stream
void launch_affine_score(hipStream_t st, const AffCall& a);
void launch_affine_choose(hipStream_t st, const AffCall& a);
void launch_affine_finish(hipStream_t st, const AffCall& a);

// ---- robust fundamental-matrix fit and dense epipolar residual (kernels_fundamental.hip, -ffp-contract=off; include/mavflow_fundamental.h) --
// What one call works on, all device pointers.  The workspace layout follows from (n, B, max_iters) alone: need[] (n + 1 int32, filled by
// the host's copy), the models (B, max_iters, 28) float64 (three slots of nine, then two int32: slots with a root, mask of the valid
// ones), the counts (B, max_iters, 3) int32 (-1: an invalid slot), the choice (B, 4) int32, then the flow form's coords (n, 2) int32 and
// its gathered pairs, src and dst (B, n, 2) float64 each.
struct FmCall {
    const double *src, *dst; const int32_t* subsets; double* F; uint8_t* inliers; void* records; char* ws;
    int n, B, max_iters; double t2;
};
__host__ __device__ inline size_t fm_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
__host__ __device__ inline size_t fm_models_offset(int n) { return fm_round(sizeof(int32_t) * ((size_t)n + 1)); }
__host__ __device__ inline size_t fm_counts_offset(int n, int B, int max_iters) { return fm_models_offset(n) + fm_round(sizeof(double) * 28 * (size_t)B * max_iters); }
__host__ __device__ inline size_t fm_choice_offset(int n, int B, int max_iters) { return fm_counts_offset(n, B, max_iters) + fm_round(sizeof(int32_t) * 3 * (size_t)B * max_iters); }
__host__ __device__ inline size_t fm_coords_offset(int n, int B, int max_iters) { return fm_choice_offset(n, B, max_iters) + fm_round(sizeof(int32_t) * 4 * (size_t)B); }
__host__ __device__ inline size_t fm_src_offset(int n, int B, int max_iters) { return fm_coords_offset(n, B, max_iters) + fm_round(sizeof(int32_t) * 2 * (size_t)n); }
__host__ __device__ inline size_t fm_dst_offset(int n, int B, int max_iters) { return fm_src_offset(n, B, max_iters) + fm_round(sizeof(double) * 2 * (size_t)n * B); }
__host__ __device__ inline size_t fm_workspace_bytes(int n, int B, int max_iters) { return fm_dst_offset(n, B, max_iters) + fm_round(sizeof(double) * 2 * (size_t)n * B); }
// the four launches of a fit, in this order on one stream
void launch_fm_models(hipStream_t st, const FmCall& a);
void launch_fm_score(hipStream_t st, const FmCall& a);
void launch_fm_choose(hipStream_t st, const FmCall& a);
void launch_fm_finish(hipStream_t st, const FmCall& a);
// the dense pass: records' initialisation, the pass and the records' final form, three launches; residual and mask may be NULL
void launch_epipolar_residual(hipStream_t st, const float* flow, const double* F, double t2, int W, int H, int B, float* residual, uint8_t* mask, void* records);

// ---- robust essential-matrix fit (kernels_essential.hip, -ffp-contract=off; include/mavflow_essential.h) ----------------------------------
// What one call works on, all device pointers.  The workspace layout follows from (n, B, max_iters) alone: need[] (n + 1 int32, filled by
// the host's copy), the models (B, max_iters, EM_STRIDE) float64 (ten slots of nine, then two int32: slots with a root, mask of the valid
// ones), the counts (B, max_iters, 10) int32 (-1: an invalid slot), the choice (B, 4) int32, then the flow form's coords (n, 2) int32 and
// its gathered pairs, src and dst (B, n, 2) float64 each.
#define EM_SLOTS 10
#define EM_STRIDE 92
struct EmCall {
    const double *src, *dst; const int32_t* subsets; double *E, *F; uint8_t* inliers; void* records; char* ws;
    int n, B, max_iters; double t2, fx, fy, cx, cy;
};
__host__ __device__ inline size_t em_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
__host__ __device__ inline size_t em_models_offset(int n) { return em_round(sizeof(int32_t) * ((size_t)n + 1)); }
__host__ __device__ inline size_t em_counts_offset(int n, int B, int max_iters) { return em_models_offset(n) + em_round(sizeof(double) * EM_STRIDE * (size_t)B * max_iters); }
__host__ __device__ inline size_t em_choice_offset(int n, int B, int max_iters) { return em_counts_offset(n, B, max_iters) + em_round(sizeof(int32_t) * EM_SLOTS * (size_t)B * max_iters); }
__host__ __device__ inline size_t em_coords_offset(int n, int B, int max_iters) { return em_choice_offset(n, B, max_iters) + em_round(sizeof(int32_t) * 4 * (size_t)B); }
__host__ __device__ inline size_t em_src_offset(int n, int B, int max_iters) { return em_coords_offset(n, B, max_iters) + em_round(sizeof(int32_t) * 2 * (size_t)n); }
__host__ __device__ inline size_t em_dst_offset(int n, int B, int max_iters) { return em_src_offset(n, B, max_iters) + em_round(sizeof(double) * 2 * (size_t)n * B); }
__host__ __device__ inline size_t em_workspace_bytes(int n, int B, int max_iters) { return em_dst_offset(n, B, max_iters) + em_round(sizeof(double) * 2 * (size_t)n * B); }
// the four launches of a fit, in this order on one stream
void launch_em_models(hipStream_t st, const EmCall& a);
void launch_em_score(hipStream_t st, const EmCall& a);
void launch_em_choose(hipStream_t st, const EmCall& a);
void launch_em_finish(hipStream_t st, const EmCall& a);

// ---- flow pictures (kernels_vis.hip, compiled with -ffp-contract=off; include/mavflow_vis.h) -----------------------------------------------
// MAV_VIS_FORM_* of a call's sizes and pointers (NULL pointers constrain nothing); -1 for a size below 1
int vis_form(int W, int H, int batch, const void* flow, const void* bgr, const void* hsv);
// the grid points of draw_flow along each axis
void vis_draw_grid(int W, int H, int step, int* nx, int* ny);
// flow (B, H, W, 2) -> bgr and (unless NULL) hsv (B, H, W, 3); records: B mav_hsv_record, the call's only scratch.  MAV_HSV_PROCESS: the
// records' initialisation, the minimum / maximum pass and the picture, three launches; MAV_HSV_DRAW: the records zeroed and one launch.
// Returns the error of zeroing the records, if any (nothing is launched then).
hipError_t launch_flow_hsv(hipStream_t st, const float* flow, int W, int H, int B, int mode, uint8_t* bgr, uint8_t* hsv, void* records);
// src, dst (B, H, W, 3) uint8, code MAV_COLOR_*; one launch
void launch_cvt_color(hipStream_t st, const uint8_t* src, int code, int W, int H, int B, uint8_t* dst);
// img (B, H, W, 3) drawn into; colour: three bytes on the host; one launch (none where the grid is empty)
void launch_draw_flow(hipStream_t st, uint8_t* img, const float* flow, int W, int H, int B, int step, float threshold, const uint8_t* colour);

// ---- shapes (kernels_shapes.hip, compiled with -ffp-contract=off; include/mavflow_shapes.h) -----------------------------------------------
// That unit holds its own host side (the entry points of its header).  What it needs of a context, which only mavflow.cpp can see:
struct CtxView { hipStream_t stream; int W, H, max_batch; };
int ctx_fail(int code, const char* fmt, ...);                               // sets mav_last_error(), returns code
int ctx_enter(mav_ctx* c, int batch, const char* fn, CtxView* out);         // the prologue of a _dev entry point (check_dev_call) and the view
int ctx_check_launch(const char* what);
// One host-pointer call beside the resident state (HostCall::beside): staging blocks behind the last call's, given back on destruction.
struct StagedCall {
    StagedCall(mav_ctx* c, const char* fn);
    ~StagedCall();
    StagedCall(const StagedCall&) = delete;
    int begin(int batch, CtxView* out);
    void* in(const void* host, size_t bytes);          // a block, filled from the host now (NULL host: no block, NULL)
    void* out(void* host, size_t bytes);               // a block, brought to the host by finish()
    void* inout(void* host, size_t bytes);             // both
    void* scratch(size_t bytes);
    int staged() const;
    int finish();
private:
    struct HostCall* h;
};
// a profiled launch section of the miscellaneous class (ProfScope)
struct MiscScope { MiscScope(mav_ctx* c); ~MiscScope(); MiscScope(const MiscScope&) = delete; private: struct ProfScope* p; };
// n bytes of `value` at p (the caller's memory), one launch
void launch_fill_bytes(hipStream_t st, uint8_t* p, uint8_t value, size_t n);

// ---- PNG decode (kernels_png_decode.hip, integer arithmetic only; include/mavflow_png_decode.h) ---------------------------------------------
// That unit holds its own host side, like the shapes unit.  The one gray value of a BGR pixel, cv2.cvtColor(COLOR_BGR2GRAY) on uint8
// (SURVEY A.7): k_bgr2gray and the decoder's gray output both go through it, so their bits agree.
__host__ __device__ inline uint8_t bgr2gray_px(unsigned b, unsigned g, unsigned r) { return (uint8_t)((b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14); }

// ---- JPEG decode (kernels_jpeg.hip, integer arithmetic only; include/mavflow_jpeg.h) ---------------------------------------------------------
// That unit holds its own host side too.  A profiled launch section of its launch 0 .. 3 (intervals, entropy, IDCT, finish: the classes
// "jpeg_intervals", "jpeg_entropy", "jpeg_idct", "jpeg_finish" of mav_profile_get)
struct JpegScope { JpegScope(mav_ctx* c, int launch); ~JpegScope(); JpegScope(const JpegScope&) = delete; private: struct ProfScope* p; };

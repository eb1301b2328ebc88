/*
 * mavflow.h -- C-ABI of libmavflow.so: the MI355X (gfx950) replacement for the per-frame-pair vision math of
 * evroon/mav-detection (Farneback flow -> derotation -> FoE fit -> phi -> threshold masks -> box).
 *
 * The reference is pure Python with no FFI of its own; each entry point below replaces the Python call cited
 * next to it (paths relative to the reference root) and is bound through ctypes (INTEGRATION.md shows the stub
 * a maintainer adds on the reference side).
 *
 * Conventions
 *   - plain C, no torch types; every buffer is caller-allocated, C-contiguous, never retained past the call.
 *   - entry points without a suffix take HOST pointers and are synchronous; `_dev` variants take DEVICE
 *     pointers (hipMalloc'd by anyone in this process, e.g. mav_dev_alloc or a torch tensor's data_ptr()),
 *     enqueue on the context's stream and return without synchronising (call mav_sync).
 *   - return value: 0 = OK, <0 = error (MAV_ERR_*); mav_last_error() gives the message. No abort(), no C++
 *     exceptions cross the boundary.
 *   - a mav_ctx is single-threaded (as the reference's loop is); distinct contexts are independent.
 *   - images are (batch, H, W) u8; flow is (batch, H, W, 2) interleaved (u, v); masks are (batch, H, W) u8 0/1.
 *     The Farneback `_ex` entry points also take 16-bit and float32 frames (MAV_DEPTH_*), as cv2.calcOpticalFlowFarneback does.
 */
#ifndef MAVFLOW_H
#define MAVFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_OK 0
#define MAV_ERR_ARG (-1)   /* bad argument (NULL, size mismatch, pyr_scale >= 1 ...): cv2.error / ValueError in the shim */
#define MAV_ERR_HIP (-2)   /* a HIP runtime call failed */
#define MAV_ERR_OOM (-3)   /* device allocation failed */
#define MAV_ERR_STATE (-4) /* context unusable / no GPU */

/* Frame depths of the `_ex` entry points: cv2's depth codes.  cv2 converts every layer's source frame with convertTo(CV_32F) before
 * GaussianBlur / resize; so does the library -- exactly for 8U and 16U, a copy for 32F -- and everything after the layer image is the
 * same float32 arithmetic for every depth: frames of any depth that hold the same values give the same flow, bit for bit.  No
 * rescaling: the solve's 1e-3 regulariser (optflowgf.cpp) makes the flow depend on the intensity scale, as it does in cv2.  Other
 * codes (signed depths, 64F: narrow on the host first) are MAV_ERR_ARG. */
#define MAV_DEPTH_8U 0
#define MAV_DEPTH_16U 2
#define MAV_DEPTH_32F 5
#define MAV_DEPTH_64F 6 /* the flow history's fields and ring only (mav_history_*, mav_stage_remap_linear): never a frame depth */

typedef struct mav_ctx mav_ctx;

/* src/farneback.py:76-80 -- the literal argument list of cv2.calcOpticalFlowFarneback.
 * Defaults (mav_fb_defaults): 0.4, 1, 12, 10, 8, 1.2, 0.  flags: 0 or MAV_OPTFLOW_USE_INITIAL_FLOW.  The bit is accepted so that a
 * cv2 argument list passes as it is; only mav_farneback_init / mav_farneback_init_dev start from an initial flow, every other entry
 * point starts from zero.  OPTFLOW_FARNEBACK_GAUSSIAN = 256 is not a flag of mav_create (MAV_ERR_ARG): the window is a property of
 * the context, chosen with mav_set_window below; mask the bit and call mav_set_window(ctx, MAV_WINDOW_GAUSSIAN). */
#define MAV_OPTFLOW_USE_INITIAL_FLOW 4
#define MAV_OPTFLOW_FARNEBACK_GAUSSIAN 256 /* cv2's value, for callers that translate a cv2 argument list; see mav_set_window */
typedef struct {
    double pyr_scale;
    int levels, winsize, iterations, poly_n;
    double poly_sigma;
    int flags;
} mav_fb_params;

/* src/focus_of_expansion.py:21-23,67 -- N = 1000 line pairs, |flow2| gate 2.5, RANSAC radius 30 px. */
typedef struct {
    int n_pairs;
    double mag_threshold, ransac_threshold;
} mav_foe_params;

/* src/processor.py:333-341 -- fixed: phi*(mag > fixed_min_mag)*~sky > fixed_deg;
 * dynamic: (mag > dyn_min_mag) * ~sky * (phi > dyn_a + (dyn_b + dyn_c/mag) | phi < dyn_a - (dyn_b + dyn_c/mag)).
 * Defaults: 15, 1.0, 0.5, 0.25, 0.5, 8. */
typedef struct {
    double fixed_deg, fixed_min_mag, dyn_min_mag, dyn_a, dyn_b, dyn_c;
} mav_thr_params;

/* One record per frame pair: what the multi-GPU all-gather moves (32 bytes). box = x0, y0, x1, y1 inclusive
 * of the fixed-threshold mask (src/im_helpers.py:55-84 semantics), all -1 when the mask is empty. */
typedef struct {
    int32_t box[4];
    double foe[2];
} mav_result;

void mav_fb_defaults(mav_fb_params*);
void mav_foe_defaults(mav_foe_params*);
void mav_thr_defaults(mav_thr_params*);

/* ---- context ------------------------------------------------------------------------------------------- */
/* One context per (device, W, H, max_batch); owns its streams, pyramid tables and -- from the first call that computes flow on --
 * the Farneback workspace (174 MB per 1080p slot, 16 slots by default): a context used only for mav_bbox / mav_tpr_fpr_counts /
 * mav_phi_mask / mav_detect / the window search holds a few KB plus the staging blocks of its calls.
 * Size bound: max_batch <= 65535 and max_batch * W * H <= 2^30 pixels (1920x1080 x 512 and 3840x2160 x 128, the global batches of
 * BASELINE configs 4 and 5, are 1 % under it): MAV_ERR_ARG above, so that no per-batch element count leaves 32 bits. */
#define MAV_MAX_BATCH_PIXELS ((size_t)1 << 30)
int mav_create(mav_ctx** out, int device, int W, int H, int max_batch, const mav_fb_params* fb /* NULL = defaults */);
int mav_destroy(mav_ctx*);
const char* mav_last_error(void); /* thread-local, never NULL */
int mav_device_count(void);       /* <= 0 when no GPU is visible */
/* Scheduling / tuning options (every switch of the library is here: it reads no environment variable).  MAV_ERR_ARG for unknown
 * names or values out of range.
 *   "group"            pairs per launch for everything but the finest layer's sweeps (default 16 up to 4 Mpx frames, 8 above)
 *   "group_fine"       pairs per launch for the finest layer's sweeps (default 1: one pair's working set stays in the Infinity Cache;
 *                      0 = same as group)
 *   "pairs_in_flight"  1 | 2 (default 2): the finest layer's per-pair work of a group alternates between two streams, every pair swept
 *                      band by band (bands of <= "band_mb" MB of working set, default 96, or "bands" when set) so that both stay in
 *                      the Infinity Cache; the coarse layers alternate sub-groups of "coarse_half" pairs (0 = half the count that fits
 *                      "coarse_cache_mb", default 220) between the two streams
 *   "bands"            J in [1, 8]: a pair's finest-layer sweeps run band by band over J skewed horizontal bands; 0 = automatic (the
 *                      default: 1 up to ~2.6 Mpx, above that as many as keep a band's working set inside the Infinity Cache; the
 *                      two-stream schedule sizes its bands by "band_mb")
 *   "share_m"          one-stream schedule: all pairs of a group ping-pong M through the first slot's buffers (default 1)
 *   "share_frames"     0: treat a frame sequence (see mav_farneback) as independent pairs (default 1)
 *   "small_batch"      default 1: a group whose finest-layer working set is at most 200 MB (one 1080p pair, two 720p pairs: a chain of
 *                      launches that each fill a fraction of the chip) gets the layer images of its whole pyramid from ONE launch and
 *                      all polynomial expansions from ONE launch instead of two launches per layer
 *   "deep_batch"       default 1: when a call has more than one group, the coarse layers of the pyramid (every layer of at most
 *                      1/"deep_frac" of the frame, default 6: all layers above the finest at pyr_scale 0.4) run ONCE for up to 64 pairs of
 *                      the call before the groups start, instead of once per group; "deep_frac" can be set until the first call that
 *                      computes flow (MAV_ERR_STATE afterwards)
 *   "coarse_bands"     default 0: 1 = a coarse layer whose per-pair working set exceeds "band_mb" (layer 1 of the 4K preset, 106 MB) is
 *                      swept like the finest layer, pairs alternating between the two streams band by band (measured slower: off)
 *   "band_skew"        default -1: the band boundaries are moved down by (iterations - 1) / 2 tile rows -- sweep `it` shifts every
 *                      boundary up by `it` rows, so this gives every band the same average size over its sweeps (even launches, even
 *                      cache footprints); n >= 0: by n rows (0 = equal bands)
 *   "band_phase"       default 0; n > 0: in the two-stream schedule the pairs of the second stream use a band partition shifted by half a
 *                      band whenever a pair has at least n bands, so that the two streams do not build their bands' initial M (HBM-bound)
 *                      at the same moments (measured slower: the lockstep of the two streams protects the Infinity Cache)
 *   "sweep_write_through"  -1 (default): the sweeps' M' stores are write-through (sc1) in the two-stream schedules, plain otherwise;
 *                      0 / 1: never / always
 *   "strip"            width in tiles of the column strips of the XCD-aware tile order (0 = automatic)
 *   "phi_screen"       0: every pixel of the phi / threshold stage takes the exact path (default 1: float32 screen in front of it)
 *   "phi_yloop"        16-row blocks per workgroup of the phi kernel (0 = automatic)
 *   "upload_threads"   host threads that stage pageable sources for mav_upload_gather (default 4, the caller included; until its first call)
 *   "inline_uploads"   default 0; 1 = mav_upload_async / _unordered / mav_upload_gather enqueue their copies on the context's COMPUTE stream
 *                      and mav_upload_fence is a no-op: the context then owns one stream (its copy stream and its second compute stream are
 *                      created by the first call that needs them), i.e. one of the runtime's few hardware queues.  For contexts that take a
 *                      stream of small calls in turn with other contexts ("lanes", mavflow/pipeline.py): streams beyond the runtime's queue
 *                      pool share queues, and lanes that share one do not overlap
 *   "stream_priority"  default 0; -1 = the context's compute stream is re-created in the HIGH priority class (the call drains the context).
 *                      The runtime keeps a pool of hardware queues per priority class and hands a new stream the least-used queue of its
 *                      class: which queue a lane gets otherwise depends on every stream the process has ever made (one idle context created
 *                      before three lanes: 0.31 instead of 0.215 ms per 1280x720 frame).  Lanes take a class of their own
 *   "cc_workspace_mb"  default 256: the most scratch mav_components* holds; a batch is labelled in sub-batches of as many images as fit
 *                      (at least one: 0 = one image at a time)
 * None of them changes a result bit (tests/test_gpu_flow.py, tests/test_gpu_screen.py; "phi_yloop" and "phi_screen":
 * tests/test_gpu_detect_forms.py). */
int mav_set_option(mav_ctx*, const char* name, long value);
int mav_get_option(mav_ctx*, const char* name, long* value);
/* The sweep's window: MAV_WINDOW_BOX (default; cv2's default flags) or MAV_WINDOW_GAUSSIAN (cv2's OPTFLOW_FARNEBACK_GAUSSIAN:
 * FarnebackUpdateFlow_GaussianBlur -- two (2m+1)-tap weighted sums, m = winsize / 2, sigma = 0.3 m, in place of the two box sums, all
 * in float32, and that path's own 2x2 solve).  Every entry point that computes flow follows it: mav_farneback*, mav_process_batch*,
 * mav_frame_step* with compute_flow, mav_stage_blur_iter.  Same tiles, launches, bands and streams as the box window; the flow of
 * a Gaussian context is bit-identical across schedules, as the box window's is.  mav_set_window drains the context's worker and
 * streams first; other values are MAV_ERR_ARG.  The definition (taps included) is restated from OpenCV 4.x and not pinned against
 * a cv2 build: see DESIGN.md section 8. */
#define MAV_WINDOW_BOX 0
#define MAV_WINDOW_GAUSSIAN 1
int mav_set_window(mav_ctx*, int window);
int mav_get_window(mav_ctx*, int* window);
/* The schedule a call of `batch` pairs takes with the options in effect, as one line of JSON: every option above, the group split,
 * whether the small-batch schedule applies and, per layer, the blur form and how the sweeps run (pairs per launch, bands).
 * bench.py prints it into its record and hashes it together with the kernel sources.  A context with the Gaussian window appends
 * one field, "window": "gaussian"; a box context's line does not mention the window. */
int mav_schedule_info(mav_ctx*, int batch, char* buf, size_t cap);
/* The same for frames of a MAV_DEPTH_* depth: only the layers' "blur" forms depend on it (staged rows of 16U / 32F frames take 2x / 4x
 * the LDS of 8U ones, and a short Gaussian whose staged tile would not fit goes through the two-pass form).  MAV_DEPTH_8U: the line
 * of mav_schedule_info, byte for byte. */
int mav_schedule_info_ex(mav_ctx*, int batch, int depth, char* buf, size_t cap);
/* Device memory: free / total bytes of the context's GPU (hipMemGetInfo), the bytes this context holds in all -- ctx_bytes is the sum
 * of the context's live device allocations, whatever they serve (memory from mav_dev_alloc is the caller's and not in it) -- and of
 * those the Farneback workspace alone (0 until a call computes flow).  Any pointer may be NULL. */
int mav_mem_info(mav_ctx*, size_t* dev_free, size_t* dev_total, size_t* ctx_bytes, size_t* workspace_bytes);
int mav_num_layers(const mav_ctx*);
int mav_layer_dims(const mav_ctx*, int k, int* w, int* h, int* ksize, double* sigma);

/* ---- host-pointer entry points (synchronous) ----------------------------------------------------------- */
/* cv2.calcOpticalFlowFarneback(prev, next, None, *fb)   [src/farneback.py:76-80] for `batch` pairs.
 * FRAME SEQUENCES: the reference calls this with next = the frame after prev and keeps `prevgray` for the following call, i.e. a
 * video of n + 1 frames is n pairs whose inner frames each appear twice.  When the two batches are views of ONE run of batch + 1
 * frames -- next == prev + W*H, in every entry point that takes prev / next, host or device pointers -- the library uploads the run
 * once and blurs / expands every frame once per group instead of twice.  The flow is bit-identical to the two-batch form. */
int mav_farneback(mav_ctx*, const uint8_t* prev, const uint8_t* next, int batch, float* flow);
/* cv2.calcOpticalFlowFarneback(prev, next, flow_init, *fb, fb.flags | OPTFLOW_USE_INITIAL_FLOW) for `batch` pairs: pair i starts from
 * flow_init[i], (batch, H, W, 2) float32 -- e.g. the previous pair's flow of a video.  As optflowgf.cpp does, the field enters at the
 * coarsest layer computed (k = mav_num_layers() - 1) only: resize(flow_init, layer size, INTER_AREA) * pyr_scale^k builds that layer's
 * initial matrices; every finer layer upsamples the coarser one's flow as always.  All-zero flow_init = mav_farneback, bit for bit.
 * flow_init == flow (in place, cv2's idiom) is allowed.  The first call allocates the top layer's field for the pairs of one group
 * (mav_mem_info's workspace figure grows by it); a context that never calls it holds nothing more. */
int mav_farneback_init(mav_ctx*, const uint8_t* prev, const uint8_t* next, int batch, const float* flow_init, float* flow);
/* mav_farneback (flow_init NULL) or mav_farneback_init (flow_init = the pairs' initial flow; it may equal flow) on frames of a
 * MAV_DEPTH_* depth: (batch, H, W) uint8_t, uint16_t or float, prev and next of the same depth.  MAV_DEPTH_8U gives the flow of
 * mav_farneback / mav_farneback_init bit for bit; frame runs (next == prev + one frame) are recognised at every depth.  An unknown
 * depth is MAV_ERR_ARG and nothing is enqueued. */
int mav_farneback_ex(mav_ctx*, const void* prev, const void* next, int depth, int batch, const float* flow_init, float* flow);
/* Detector.derotate [src/detector.py:70-117]: omega = angular difference / dt, (batch,3); dt (batch). */
int mav_derotate(mav_ctx*, const float* flow, const double* omega, const double* dt, int batch, double* flow_out);
/* FocusOfExpansion.get_FOE_dense + ransac [src/focus_of_expansion.py:32-86]; samples (batch, 2N, 2) = (row, col)
 * drawn by the caller exactly as :70-71 does (the GPU never generates them). foe (batch, 2). */
int mav_foe_dense(mav_ctx*, const double* flow, const uint32_t* samples, int batch, const mav_foe_params*, double* foe);
/* FocusOfExpansion.ransac [src/focus_of_expansion.py:32-54] on caller-supplied estimates (count, 2), count <= 4096:
 * first estimate with the strictly largest number of others within ransac_threshold; (0, 0) when none has a neighbour. */
int mav_ransac(mav_ctx*, const double* estimates, int count, double ransac_threshold, double* foe /* 2 */);
/* cv2.cvtColor(img, COLOR_BGR2GRAY) [src/farneback.py:21,74] for (batch, H, W, 3) u8 frames -> (batch, H, W) u8. */
int mav_bgr2gray(mav_ctx*, const uint8_t* bgr, int batch, uint8_t* gray);
/* FocusOfExpansion.get_phi [src/focus_of_expansion.py:150-184] + threshold block [src/processor.py:333-341].
 * sky: (batch,H,W) u8 or NULL; phi (degrees), mask_fixed, mask_dyn, max_phi (batch) are each optional (NULL). */
int mav_phi_mask(mav_ctx*, const double* flow, const double* foe, const uint8_t* sky, int batch, const mav_thr_params*,
                 double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, double* max_phi);
/* The same two calls handed a FLOAT32 flow array, which is what the reference does for frame index 0 (derotate returns its
 * input, src/detector.py:80-81): numpy then evaluates the |flow2| gate (:78), get_phi (:163-177, zeros_like keeps float32) and
 * the threshold block in float32.  Same arithmetic here, in numpy's operation order; the line intersections stay in double
 * (float32 + uint32 promotes).  phi / max_phi are float32.  arccos: correctly rounded float32 (numpy's own float32 arccos is a
 * SIMD routine up to 2 ulp away from that, host dependent -- see tests/test_frame0.py). */
int mav_foe_dense_f32(mav_ctx*, const float* flow, const uint32_t* samples, int batch, const mav_foe_params*, double* foe);
int mav_phi_mask_f32(mav_ctx*, const float* flow, const double* foe, const uint8_t* sky, int batch, const mav_thr_params*,
                     float* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, float* max_phi);
/* im_helpers.get_simple_bounding_box [src/im_helpers.py:55-84] on u8 images: box (batch,4) = x0,y0,x1,y1, -1 if empty. */
int mav_bbox(mav_ctx*, const uint8_t* img, int batch, int32_t* box);
/* Level 0 of Detector.analyze_pyramid [src/detector.py:280-312] on the 3-channel replica of a u8 image:
 * out (batch,3) = score, x, y of the first 64x64 / stride-16 window with the strictly largest sum. */
int mav_window_max(mav_ctx*, const uint8_t* img, int batch, int64_t* out);
/* Detector.analyze_pyramid [src/detector.py:280-312] over ALL levels of pyramid() [src/im_helpers.py:12-35; each level =
 * imutils.resize(previous, width=int(w/scale)) = cv2.resize(INTER_AREA), until a side drops below 30 px] with
 * sliding_window() [src/im_helpers.py:38-52], on the 3-channel replica of a u8 image (the reference passes scale 1.5).
 * out (batch,6) = score, x, y, level, argmax_row, argmax_col: the first window in scan order (level 0 first) with the
 * strictly largest sum; x, y in that level's own coordinates (the reference does not rescale them); argmax = position of
 * the window's first maximum (np.unravel_index(window.argmax(), ...)); all 0 when no window has a positive sum.
 * MAV_ERR_ARG when scale <= 1 or a level's size ratio is a whole number in both axes (OpenCV's fast-area path). */
int mav_analyze_pyramid(mav_ctx*, const uint8_t* img, int batch, double scale, int64_t* out);
int mav_pyramid_levels(const mav_ctx*, double scale);                          /* number of levels (>= 1), or MAV_ERR_* */
int mav_pyramid_dims(const mav_ctx*, double scale, int level, int* w, int* h); /* size of level `level` */
/* Detector.optimize_window [src/detector.py:314-358] on the 3-channel replica of a u8 image: greedy growth / shrink of a
 * window by moving one corner diagonally by one pixel per step while the enclosed sum rises (Python slice semantics for
 * windows that leave the image).  window_in / window_out (batch,4) = x, y, w, h; score (batch) = 3 * enclosed sum, 0 and the
 * unchanged window when no neighbour has a positive sum. */
int mav_optimize_window(mav_ctx*, const uint8_t* img, int batch, const int32_t* window_in, int64_t* score, int32_t* window_out);
/* im_helpers.calculate_tpr_fpr [src/im_helpers.py:244-252]: positives = #(gt > 127), negatives = #(255 - gt > 127),
 * tp = #(gt * img > 127), fp = #((255 - gt) * img > 127), where img = mask_value at the set pixels of `mask` (any nonzero byte)
 * and 0 elsewhere, products in wide integers as numpy forms them for the reference's own argument 255 * mask (mask_value 255,
 * src/processor.py:350-351) or for a bool mask (mask_value 1).  gt: any u8 image.
 * counts (batch,4) = positives, negatives, true positives, false positives. */
int mav_tpr_fpr_counts(mav_ctx*, const uint8_t* gt, const uint8_t* mask, int mask_value, int batch, int64_t* counts);
/* The same counts for the two masks the most recent mav_detect / mav_process_batch / mav_phi_mask(_f32) call on this context
 * produced, which are still resident on the device: the validation tail of the loop [src/processor.py:350-351] without moving
 * the masks again.  gt (batch, H, W) u8; counts_fixed / counts_dyn (batch, 4) each, either may be NULL.  MAV_ERR_STATE when
 * no such call precedes or its batch differs. */
int mav_last_masks_tpr_fpr(mav_ctx*, const uint8_t* gt, int mask_value, int batch, int64_t* counts_fixed, int64_t* counts_dyn);

/* The fused loop body of Processor.run_detection [src/processor.py:305-341] for `batch` pairs:
 * frames -> flow -> (derotate) -> FoE -> phi -> masks -> box. omega/dt NULL = no rotation (dt = 1);
 * sky NULL = no sky; flow / mask_fixed / mask_dyn / phi outputs are optional (NULL). results (batch).
 * frame0 (batch) u8 flags or NULL: a nonzero flag marks a pair as the reference's frame index 0, for which
 * Detector.derotate returns the float32 flow untouched [src/detector.py:80-81] and every numpy expression after it
 * (|flow2| gate of get_FOE_dense :78, get_phi :163-177, the threshold block) therefore runs in FLOAT32: that pair is not
 * derotated and is evaluated in float32 arithmetic in numpy's operation order (phi, if requested, is the float32 value
 * widened).  Pairs without the flag follow the float64 path of every later frame. */
int mav_process_batch(mav_ctx*, const uint8_t* prev, const uint8_t* next, const uint32_t* samples, const double* omega,
                      const double* dt, const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params*,
                      const mav_thr_params*, float* flow, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                      mav_result* results);
/* The same loop body from the reference's own flow seam [src/datasets/dataset.py:205-212 -> src/processor.py:305-341]:
 * `flow` is the float32 (batch, H, W, 2) field Dataset.get_flow_uv returns (a .flo file, or mav_farneback's output);
 * derotation, FoE, phi, masks and box as in mav_process_batch.  One upload of the flow, no other transfer of it. */
int mav_detect(mav_ctx*, const float* flow, const uint32_t* samples, const double* omega, const double* dt,
               const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params*, const mav_thr_params*, double* phi,
               uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results);

/* The three images Processor.run_detection writes per frame [src/processor.py:364-374], (batch, H, W, 3) u8 BGR each, as the reference
 * hands them to cv2.imwrite:
 *   img_result  im_helpers.to_rgb(255 * estimate_fixed): 255 where the fixed-threshold mask is set, 0 elsewhere
 *   img_flow    im_helpers.get_flow_vis(derotated flow) = flow_vis.flow_to_color(..., convert_to_bgr=True)
 *   img_phi     im_helpers.apply_colormap(to_rgb(phi, max_value=180.0)) = cv2.applyColorMap(..., COLORMAP_JET)
 * flow / omega / dt / frame0 / sky as in mav_detect, foe (batch, 2) the pairs' FoE (read only for img_result / img_phi), thresholds as
 * in mav_detect (NULL = defaults).  Derotation, the fixed mask and phi are recomputed per pixel in the exact arithmetic of the detection
 * path (no single-precision screen); a frame-0 pair is rendered in float32 as numpy does.  Any image may be NULL (not rendered).
 * JET entries 200..255 are restated from OpenCV's Jet definition: no image the reference wrote pins them. */
int mav_render(mav_ctx*, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
               const uint8_t* sky, int batch, const mav_thr_params*, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi);
/* The same images from what the most recent mav_detect / mav_process_batch(_dev) / mav_detect_dev / frame step on this context left
 * resident (flow, derotation constants, FoE, sky, thresholds): the flow is not moved again.  Host outputs, synchronous.  MAV_ERR_STATE
 * when no such call precedes, its batch differs, or a later call may have overwritten its flow (any other host-pointer call, a flow
 * call).  Device buffers of a _dev call must still hold what that call read. */
int mav_last_render(mav_ctx*, int batch, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi);
/* im_helpers.get_flow_vis [src/im_helpers.py:103-112] alone: flow_to_color(flow, convert_to_bgr=True) of (batch, H, W, 2) fields,
 * float64 (f64 != 0) or float32 (f64 == 0: numpy's float32 arithmetic), -> (batch, H, W, 3) u8 BGR. */
int mav_flow_to_color(mav_ctx*, const void* flow, int f64, int batch, uint8_t* img);
/* cv2.applyColorMap(gray, COLORMAP_JET) of n u8 values -> n BGR triples (a 3-channel image: mav_bgr2gray first, as OpenCV does). */
int mav_colormap_jet(mav_ctx*, const uint8_t* gray, size_t n, uint8_t* bgr);

/* The frame Processor.run_detection writes to processed.mp4 [src/processor.py:376-392], (batch, H, W, 3) u8 BGR:
 *   draw_FoE(frame, foe, [0, 255, 0]) then draw_FoE(frame, foe_gt, [255, 255, 255]) [src/focus_of_expansion.py:186-201]: filled discs
 *   of `radius` (cv2.circle, thickness -1, LINE_8: OpenCV's integer midpoint spans, clipped), centre (int(x), int(y)) truncated toward
 *   zero, white over green; a disc with |x| > 1e9 or |y| > 1e9 is not drawn;
 *   mask_rgb = that frame with (150, 0, 150) where mask_fixed is non-zero; overlay = cv2.addWeighted(frame, 0.2, mask_rgb, 0.8, 0.0),
 *   exactly (p + 4 q + 2) / 5 per byte (no ties: the exact value's fraction is a multiple of .2).
 * written[b] = 1 when the reference writes the frame (np.sum(result_img) > 0: the mask is non-empty or a disc has a pixel inside the
 * image), else 0.  frames (batch, H, W, 3), mask_fixed (batch, H, W), foe / foe_gt (batch, 2); radius in [0, MAV_OVERLAY_MAX_RADIUS]
 * (the reference draws 10).  A NaN coordinate is MAV_ERR_ARG (int(nan) raises in the reference).  The spans are restated from
 * OpenCV's published routine: no image the reference wrote pins them.  The input frames are not modified. */
#define MAV_OVERLAY_MAX_RADIUS 4096
int mav_overlay(mav_ctx*, const uint8_t* frames, const uint8_t* mask_fixed, const double* foe, const double* foe_gt, int batch, int radius,
                uint8_t* overlay, uint8_t* written);
/* The same frames from the fixed mask and dense FoE that the most recent mav_detect / mav_process_batch(_dev) / mav_detect_dev / frame
 * step on this context left resident (the mask is not moved again): host frames and foe_gt in, host overlay and written out,
 * synchronous.  MAV_ERR_STATE under mav_last_render's rules, and when that call kept no fixed mask (mask_fixed NULL).  The dense FoE
 * is finite by construction. */
int mav_last_overlay(mav_ctx*, const uint8_t* frames, const double* foe_gt, int batch, int radius, uint8_t* overlay, uint8_t* written);

/* ---- device-pointer entry points (asynchronous on the context's stream) -------------------------------- */
int mav_farneback_dev(mav_ctx*, const uint8_t* prev, const uint8_t* next, int batch, float* flow);
/* mav_farneback_init on device pointers (enqueue only).  flow_init == flow is allowed; ranges that overlap without being the same
 * field are MAV_ERR_ARG.  mav_last_flow_dev reports `flow`. */
int mav_farneback_init_dev(mav_ctx*, const uint8_t* prev, const uint8_t* next, int batch, const float* flow_init, float* flow);
/* mav_farneback_ex on device pointers (enqueue only); flow_init == flow is allowed (a warm-started chain in place). */
int mav_farneback_ex_dev(mav_ctx*, const void* prev, const void* next, int depth, int batch, const float* flow_init, float* flow);
int mav_process_batch_dev(mav_ctx*, const uint8_t* prev, const uint8_t* next, const uint32_t* samples, const double* omega,
                          const double* dt, const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params*,
                          const mav_thr_params*, float* flow, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                          mav_result* results);
int mav_detect_dev(mav_ctx*, const float* flow, const uint32_t* samples, const double* omega, const double* dt,
                   const uint8_t* frame0, const uint8_t* sky, int batch, const mav_foe_params*, const mav_thr_params*,
                   double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, mav_result* results);
/* Device pointer of the flow field the most recent mav_process_batch_dev / mav_farneback_dev / mav_farneback_init_dev call on this context wrote
 * (the caller's buffer, or the context's own workspace when the caller passed flow == NULL); NULL before the first call.
 * Lets a caller that keeps the flow in the workspace (bench.py) still inspect it. */
/* cv2.cvtColor(COLOR_BGR2GRAY) [src/farneback.py:21,74] on device pointers: (batch, H, W, 3) u8 -> (batch, H, W) u8. */
int mav_bgr2gray_dev(mav_ctx*, const uint8_t* bgr, int batch, uint8_t* gray);
const float* mav_last_flow_dev(const mav_ctx*);
/* mav_render on device pointers (enqueue only); the images are written once, nothing else is. */
int mav_render_dev(mav_ctx*, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                   const uint8_t* sky, int batch, const mav_thr_params*, uint8_t* img_result, uint8_t* img_flow, uint8_t* img_phi);
/* mav_overlay on device pointers (enqueue only).  The FoEs are device data and are not inspected on the host: a NaN coordinate draws
 * no disc here. */
int mav_overlay_dev(mav_ctx*, const uint8_t* frames, const uint8_t* mask_fixed, const double* foe, const double* foe_gt, int batch,
                    int radius, uint8_t* overlay, uint8_t* written);
/* im_helpers.calculate_tpr_fpr [src/im_helpers.py:244-252, called at src/processor.py:350-351] for device-resident masks against a
 * device-resident ground truth, counts left on the device (4 x int64 per pair: positives, negatives, true / false positives): the
 * validation tail of a batch as one more launch behind mav_process_batch_dev / mav_detect_dev.  gt_images = batch: one ground-truth
 * image per pair; gt_images = 1: ONE image shared by every pair (a sequence whose segmentation does not change).  Either mask (with
 * its counts buffer) may be NULL; both masks share one pass over the ground truth. */
int mav_tpr_fpr_counts_dev(mav_ctx*, const uint8_t* gt, int gt_images, const uint8_t* mask_fixed, const uint8_t* mask_dyn, int mask_value,
                           int batch, int64_t* counts_fixed, int64_t* counts_dyn);
int mav_sync(mav_ctx*);
void* mav_stream(mav_ctx*); /* the context's hipStream_t */

/* device memory + copies for callers without their own HIP binding */
int mav_dev_alloc(mav_ctx*, size_t bytes, void** out);
int mav_dev_free(mav_ctx*, void* p);
int mav_memcpy_h2d(mav_ctx*, void* dst, const void* src, size_t bytes);
int mav_memcpy_d2h(mav_ctx*, void* dst, const void* src, size_t bytes);

/* Overlapped uploads: pinned host memory and copies on a second stream, ordered against the compute stream in BOTH
 * directions: mav_upload_async first makes the copy stream wait for everything enqueued on the context's stream so far
 * (so a buffer set is never overwritten while an earlier batch still reads it), and mav_upload_fence makes everything
 * enqueued on the context's stream AFTER the fence wait for the copies issued BEFORE it.  Double-buffered batches:
 *   upload_async(set B) ; process_batch_dev(set A) ; upload_fence() ; upload_async(set A) ; process_batch_dev(set B) ; ... */
int mav_host_alloc(mav_ctx*, size_t bytes, void** out);
int mav_host_free(mav_ctx* /* may be NULL: the memory may outlive its context */, void* p);
int mav_upload_async(mav_ctx*, void* dst_dev, const void* src_host, size_t bytes);
/* The same copy WITHOUT the wait for the compute stream: for a destination no enqueued work touches (the other buffer set).  With
 * mav_upload_async the order  process_batch_dev(set A) ; upload_async(set B)  makes the copy wait for batch A -- correct, but the
 * overlap is gone; this form overlaps in either order.  Overwriting a buffer that enqueued work still reads is the caller's bug. */
int mav_upload_async_unordered(mav_ctx*, void* dst_dev, const void* src_host, size_t bytes);
int mav_upload_fence(mav_ctx*);
/* GATHER upload: `count` separate host arrays of bytes_each bytes -> one contiguous device buffer (array i at dst_dev + i * bytes_each),
 * on the copy stream.  This is the shape the reference's loop hands its data over in: one numpy array per frame from
 * Dataset.get_frame / get_flow_uv [src/datasets/dataset.py:205-230], i.e. 128 separate 2 MB arrays for a batch of 64 pairs at 1080p.
 * Pageable sources are copied into a ring of page-locked chunks by a few worker threads (option "upload_threads", default 4: the
 * calling thread plus three; settable until the first call) and every chunk crosses PCIe while the next one is being filled;
 * sources that are page-locked already (mav_host_alloc) are sent from where they are.  On return every source has been READ (the
 * caller may overwrite it) -- for a page-locked source that means the call waits for its transfer (copy stream), or, with option
 * "inline_uploads" (where the transfer would queue behind the compute stream's kernels), stages it like a pageable one; the
 * transfers of staged sources complete on the copy stream -- mav_upload_fence orders the compute stream behind them.
 * flags: MAV_GATHER_ORDERED: as mav_upload_async, the copies wait for everything enqueued on the compute stream so far (without it:
 * as mav_upload_async_unordered).  MAV_GATHER_SOURCES_HELD: the caller keeps every source alive and unchanged until work enqueued
 * behind the copies has completed (a marker recorded after mav_upload_fence has fired): page-locked sources are then read by the DMA
 * engine whenever the stream gets there and the call waits for nothing.  The same pointer may appear more than once (replication). */
#define MAV_GATHER_ORDERED 1
#define MAV_GATHER_SOURCES_HELD 2
int mav_upload_gather(mav_ctx*, void* dst_dev, const void* const* src_host, int count, size_t bytes_each, int flags);
/* Device -> host copy enqueued on the context's stream (dst_host should be page-locked: mav_host_alloc); complete after mav_sync or
 * after a marker recorded behind it. */
int mav_download_async(mav_ctx*, void* dst_host, const void* src_dev, size_t bytes);
/* Markers: "everything enqueued on the context's stream so far" as an object the host can wait for WITHOUT draining the stream
 * (mav_sync also waits for whatever was enqueued after the marker).  A loop that keeps two batches in flight records one per batch
 * behind the batch's result download and waits for it when it needs those results.  A marker may outlive the context it was
 * recorded on, but once that context is destroyed (mav_destroy drains its streams: everything the marker stood behind has finished)
 * it is only to be destroyed, not waited for or queried: the runtime's event still refers to the context's stream. */
int mav_marker_create(mav_ctx*, void** marker_out);
int mav_marker_record(mav_ctx*, void* marker);
int mav_marker_wait(mav_ctx* /* may be NULL */, void* marker);
/* *done = 1 when everything the marker was recorded behind has completed (or it was never recorded), else 0; never blocks. */
int mav_marker_query(mav_ctx* /* may be NULL */, void* marker, int* done);
int mav_marker_destroy(mav_ctx* /* may be NULL */, void* marker);

/* ---- blob detections: connected components of u8 masks, on the device ----------------------------------------------------------------
 * The step from a mask to objects that the reference left commented out [src/detector.py:189, src/validator.py:116:
 * frame_result.add_box('MAV', 1.0, window)]: where mav_result.box is the hull of EVERY set pixel, this is one record per connected
 * component.  mask: (batch, H, W) u8, any non-zero byte is set.  connectivity 4 or 8.
 *   labels  optional (NULL), (batch, H, W) int32: 0 on background, components numbered 1 .. n in raster order of their FIRST pixel
 *           (top-most row, then left-most column).  That is scipy.ndimage.label's numbering.  It is NOT promised to be cv2's:
 *           cv2.connectedComponents' block-based default algorithms create labels in 2x2-block order (unpinned against cv2, like the
 *           Farneback caveats above).
 *   counts  (batch): n_components = the exact number of components; n_blobs = the exact number with area >= min_area -- it may exceed
 *           max_blobs, which is how a caller sees that the table is truncated.
 *   blobs   (batch, max_blobs) records of 40 bytes: the first min(n_blobs, max_blobs) components with area >= min_area in label order;
 *           x, y, w, h as cv2's CC_STAT_LEFT / TOP / WIDTH / HEIGHT; sum_x, sum_y the integer coordinate sums (sum / area in float64 on
 *           the host is the exact centroid).  Unused records are all-zero bytes: whole tables compare equal.
 * Parameters (mav_cc_defaults: 8, 1, 256; NULL = defaults): connectivity 4 | 8, min_area >= 1, max_blobs 1 .. MAV_CC_MAX_BLOBS; anything
 * else is MAV_ERR_ARG and nothing is enqueued.  All results are integers and functions of the partition into components alone: the same
 * call gives the same bytes every time (tests/test_gpu_components.py compares them with tests/components_ref.py bit for bit).
 * Scratch: two int32 planes + a few counters, 8.03 bytes per pixel, from the context's memory ledger (mav_mem_info counts it); a batch
 * is walked in sub-batches of as many images as fit option "cc_workspace_mb" (default 256; at least one image), so the workspace is
 * bounded whatever max_batch is.  The tile of the first pass is MAV_CC_TILE_W x MAV_CC_TILE_H pixels. */
#define MAV_CC_TILE_W 64
#define MAV_CC_TILE_H 16
#define MAV_CC_MAX_BLOBS 65535
typedef struct {
    int connectivity, min_area, max_blobs;
} mav_cc_params;
typedef struct {
    int32_t n_components, n_blobs;
} mav_cc_counts;
typedef struct {
    int32_t label, x, y, w, h, area;
    int64_t sum_x, sum_y;
} mav_blob;
void mav_cc_defaults(mav_cc_params*);
int mav_components(mav_ctx*, const uint8_t* mask, int batch, const mav_cc_params*, int32_t* labels, mav_cc_counts* counts,
                   mav_blob* blobs);                                                      /* host pointers, synchronous */
int mav_components_dev(mav_ctx*, const uint8_t* mask, int batch, const mav_cc_params*, int32_t* labels, mav_cc_counts* counts,
                       mav_blob* blobs);                                                  /* device pointers, enqueue only */
/* The same for the fixed (which = 0) or dynamic (which = 1) mask that the most recent mav_detect / mav_process_batch /
 * mav_phi_mask(_f32) call on this context left resident: host outputs, the mask is not moved again.  MAV_ERR_STATE exactly as
 * mav_last_masks_tpr_fpr (no such call precedes, its batch differs, or it kept no such mask). */
int mav_last_masks_components(mav_ctx*, int which, int batch, const mav_cc_params*, int32_t* labels, mav_cc_counts* counts,
                              mav_blob* blobs);

/* ---- one iteration of the reference's loop as ONE call ---------------------------------------------------------------------------
 * Processor.run_detection's body [src/processor.py:283-362] is, per frame: read a frame, get the flow (Farneback here), derotate,
 * FoE, phi, masks, TPR / FPR counts against the segmentation, store a record.  Through the entry points above that is a dozen calls
 * per frame (gather upload, fence, Farneback, markers, parameter upload, detect, counts, download, marker) -- at 1280x720, where the
 * GPU needs 0.18 ms per frame, the calling thread needs longer than that to issue them.  mav_frame_step describes the whole
 * iteration; mav_frame_step_dev enqueues it in one call, and mav_frame_step_post hands it to the context's WORKER thread (created by
 * the first post) and returns at once, so that a single-threaded host loop feeding two or three contexts in turn ("lanes") pays a
 * few microseconds per frame and the contexts enqueue side by side.  Every part is optional; what is present runs in this order:
 *   1. the host waits for `wait_before` markers (the last readers of buffers the uploads overwrite),
 *   2. uploads: the packed parameter block (par_host -> par_dev; par_host should be page-locked) and the `gather` lists (host arrays ->
 *      device: frames, a host flow field, per-pair sky masks / ground truth), as mav_upload_gather does, then the upload fence,
 *   3. BGR -> gray of `n_bgr` frames (mav_bgr2gray_dev),
 *   4. compute_flow: flow_dev = Farneback(prev_dev, next_dev) for n pairs (mav_farneback_dev; the frame-sequence layout is
 *      recognised), then the `record_after_flow` markers ("the frame buffers have been read"),
 *   5. detection on flow_dev (mav_detect_dev): samples / omega / dt / frame0 at their offsets inside par_dev, sky_dev, masks,
 *      n records to out_dev; with gt_dev the TPR / FPR counts of both masks (mav_tpr_fpr_counts_dev) to out_dev + off_counts_*,
 *      with cc.max_blobs != 0 the connected components of mask_fixed_dev (mav_components_dev) to out_dev + off_cc_*,
 *   6. out_dev[0 : out_bytes] -> out_host (page-locked), then `record_done`.
 * The library copies the struct and the pointer arrays it refers to (gather[i].src_host, wait_before, record_after_flow) when the
 * step is posted; the HOST BUFFERS themselves (frames, par_host, out_host) must stay valid and unchanged until the step's
 * `record_done` marker has fired (mav_frame_step_wait).  A step that fails after part of it has been enqueued (a parameter refused
 * inside the detection, after the gathers and Farneback) still records `record_after_flow` and `record_done`, behind the upload fence
 * and what it did enqueue: waiting for its marker before giving the host buffers back stays enough. */
typedef struct {
    const void* const* src_host; /* count host arrays of bytes_each bytes ... */
    int count;
    size_t bytes_each;
    void* dst_dev;               /* ... to dst_dev + i * bytes_each */
} mav_gather;
#define MAV_STEP_MAX_GATHER 4
typedef struct mav_frame_step {
    int n; /* pairs (1 <= n <= max_batch) */
    /* 1. */
    void* const* wait_before;
    int n_wait_before;
    /* 2. */
    const void* par_host;
    void* par_dev;
    size_t par_bytes;
    mav_gather gather[MAV_STEP_MAX_GATHER];
    int n_gather;
    /* 3. */
    const uint8_t* bgr_dev; /* n_bgr frames (H, W, 3) u8, gathered there by a `gather` entry */
    int n_bgr;
    uint8_t* gray_dev;      /* n_bgr frames (H, W) u8 out */
    /* 4. */
    int compute_flow;
    const uint8_t* prev_dev; /* n gray frames each */
    const uint8_t* next_dev;
    float* flow_dev;         /* (n, H, W, 2) float32: written by step 4 (NULL: into the context's own flow buffer), or gathered in step 2, or resident */
    void* const* record_after_flow;
    int n_record_after_flow;
    /* 5. */
    int detect;              /* 0: stop after step 4 (a flow-only step) */
    size_t off_samples, off_omega, off_dt, off_frame0; /* byte offsets inside par_dev */
    int has_omega, has_frame0;
    const uint8_t* sky_dev;  /* n sky masks or NULL */
    const uint8_t* gt_dev;   /* ground truth for the counts, or NULL: no counts */
    int gt_images;           /* n, or 1 = one image shared by every pair */
    mav_foe_params foe;
    mav_thr_params thr;
    uint8_t* mask_fixed_dev; /* (n, H, W) u8 each */
    uint8_t* mask_dyn_dev;
    void* out_dev;           /* n mav_result records at offset 0 */
    size_t off_counts_fixed, off_counts_dyn; /* n x 4 int64 each, inside out_dev */
    /* 6. */
    void* out_host;
    size_t out_bytes;
    void* record_done;
    /* 5, behind the counts: connected components of mask_fixed_dev (mav_components_dev), n mav_cc_counts at out_dev + off_cc_counts and
     * n x cc.max_blobs mav_blob records at out_dev + off_cc_blobs (a multiple of 8), so that part 6's one copy carries them.
     * cc.max_blobs == 0 (a zeroed struct): off, not one launch more. */
    mav_cc_params cc;
    size_t off_cc_counts, off_cc_blobs;
} mav_frame_step;
int mav_frame_step_dev(mav_ctx*, const mav_frame_step*);
/* Post the step to the context's worker thread.  From the first post on until mav_worker_drain (or mav_destroy) the worker is the
 * thread that owns the context: the caller may post further steps and wait for tickets, and must call mav_worker_drain before any
 * other entry point of this context (the Python binding does so by itself).  *ticket identifies the step.  mav_destroy lets the
 * worker finish the step it is enqueueing and DROPS the ones still queued. */
int mav_frame_step_post(mav_ctx*, const mav_frame_step*, uint64_t* ticket);
/* Block until step `ticket` has been enqueued by the worker and, when `marker` is not NULL (the step's record_done), until that
 * marker has fired -- for a failed step too.  Returns the step's own return code (and sets mav_last_error to its message).  The
 * first wait for a failed ticket reports the failure, even when a drain has reported it already; after that wait no
 * mav_worker_drain reports it again. */
int mav_frame_step_wait(mav_ctx*, uint64_t ticket, void* marker);
/* Block until the worker has enqueued every posted step (device work may still be running); returns the code of the earliest failed
 * step that neither an earlier drain nor mav_frame_step_wait has reported, MAV_OK if none.  No-op for a context that never posted. */
int mav_worker_drain(mav_ctx*);
/* Block until the worker has enqueued step `ticket` (and every step before it).  Unlike mav_frame_step_wait it delivers nothing: a
 * failure of the step stays for its wait and for the next drain.  MAV_OK at once for ticket 0 or a context that never posted. */
int mav_worker_wait_enqueued(mav_ctx*, uint64_t ticket);

/* ---- threshold sweep: the TPR / FPR counts of every (angle, magnitude) pair in one pass ---------------------------------------------
 * The detector's one decision is the fixed mask [src/processor.py:340-341], phi * (mag > fixed_min_mag) * ~sky > fixed_deg, and
 * mav_result / mav_tpr_fpr_counts report it at one operating point.  The sweep evaluates it at every pair of two lists in ONE pass over
 * flow, sky and ground truth.
 *   angles[0 .. n_angles), mags[0 .. n_mags): HOST arrays (copied by the call), each strictly increasing, finite and >= 0;
 *   1 <= n_angles <= MAV_ROC_MAX_ANGLES, 1 <= n_mags <= MAV_ROC_MAX_MAGS.  Anything else is MAV_ERR_ARG: nothing is enqueued, nothing
 *   is written.
 * Per pair of the batch one table of MAV_ROC_TABLE_WORDS(n_angles, n_mags) int64 words:
 *   pos, neg, then for i in angles, for j in mags: tp[i][j], fp[i][j]
 * pos / neg are mav_tpr_fpr_counts' first two counts; tp[i][j] / fp[i][j] are its last two for the fixed mask that the detection stage
 * produces with thr.fixed_deg = angles[i], thr.fixed_min_mag = mags[j] and everything else the same (sky, derotation, frame-0 pairs),
 * at mask_value 255 -- where a set pixel is a true positive iff gt >= 1 and a false positive iff gt <= 254.
 * Why >= 0: phi is never NaN (angle_diff[isnan] = 0) and never negative, so for a threshold t >= 0 the reference's product form
 * phi * gate > t equals gate && phi > t (a closed gate gives 0 > t, false); the mask is then monotone in both thresholds, a pixel
 * with ia = #{angles < phi} and im = #{mags < mag} (strict comparisons, as the mask's) is set in exactly the cells (i < ia, j < im),
 * and one histogram of the exact bins gives every cell by a suffix sum.  A negative threshold would set every gated-off and sky pixel.
 * A NaN magnitude passes no gate.  A frame-0 pair compares as the detection stage does: float32 phi and magnitude against the thresholds
 * ROUNDED TO FLOAT32 -- two thresholds that collapse to one float32 value give equal cells for such a pair.
 * Of `thr` only the dynamic mask's fields (dyn_min_mag, dyn_a, dyn_b, dyn_c) are ignored, and fixed_deg / fixed_min_mag are replaced by
 * the lists: nothing of it is read today, the parameter is there so that the argument list is mav_render's (NULL is fine).  phi and the magnitude are the exact path's bits (no single-precision screen), the counts are integers:
 * the same call gives the same bytes every time.  No scratch beyond the table. */
#define MAV_ROC_MAX_ANGLES 64
#define MAV_ROC_MAX_MAGS 16
#define MAV_ROC_TABLE_WORDS(ka, km) (2 + 2 * (size_t)(ka) * (km))
typedef struct {
    int n_angles, n_mags;
    const double* angles; /* HOST arrays, copied by the call */
    const double* mags;
} mav_roc_params;
/* flow / foe / omega / dt / frame0 / sky as in mav_render; gt (gt_images, H, W) u8 with gt_images = batch, or 1 = one image shared by
 * every pair (as mav_tpr_fpr_counts_dev); table (batch, MAV_ROC_TABLE_WORDS).  Host pointers, synchronous. */
int mav_roc_sweep(mav_ctx*, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                  const uint8_t* sky, const uint8_t* gt, int gt_images, int batch, const mav_thr_params*, const mav_roc_params*,
                  int64_t* table);
/* The same on device pointers (all but the parameters' arrays); enqueue only. */
int mav_roc_sweep_dev(mav_ctx*, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* frame0,
                      const uint8_t* sky, const uint8_t* gt, int gt_images, int batch, const mav_thr_params*, const mav_roc_params*,
                      int64_t* table);
/* The same on what the most recent mav_detect / mav_process_batch(_dev) / mav_detect_dev / frame step left resident (flow, derotation
 * constants, FoE, sky): gt is a host array, the table a host output, synchronous.  MAV_ERR_STATE exactly as mav_last_render.  A
 * mav_phi_mask / mav_phi_mask_f32 call leaves its field (float64, already derotated; or float32, a frame-0 pair), FoE and sky resident
 * for this call too -- the staged loop's route -- though not for mav_last_render. */
int mav_last_roc_sweep(mav_ctx*, const uint8_t* gt, int gt_images, int batch, const mav_roc_params*, int64_t* table);
/* The loop hook.  mav_frame_step is a frozen layout, so the sweep is armed on the context instead: while armed, every frame step whose
 * part 5 runs with gt_dev also enqueues the sweep behind the counts and the components -- on the step's own flow_dev, FoE, derotation
 * block, sky_dev, gt_dev / gt_images and thr -- and writes n tables at out_dev + off_table, so that part 6's one copy carries them.
 * off_table must be a multiple of 8 (MAV_ERR_ARG here otherwise).  A step with out_host whose out_bytes is smaller than
 * off_table + n tables is refused with MAV_ERR_ARG before anything of it is enqueued (its markers are still recorded).
 * params == NULL disarms; disarmed is the default, and then not one launch or byte of a step differs.  The call drains the worker
 * itself (as mav_frame_step_dev does: it returns a failed step's code that nothing has reported yet, and then changes nothing); it
 * must still not run concurrently with a thread that posts steps.  The armed state belongs to the CONTEXT: whoever runs steps of
 * different shapes on one context arms before each (the Python pipelines do). */
int mav_roc_arm(mav_ctx*, const mav_roc_params* /* NULL: disarm */, size_t off_table);

/* ---- flow history: every pixel's trajectory through the last fields [src/detector.py:365-388, Detector.get_history] ------------------
 * The reference's one temporal operator.  A ring keeps the last `length` flow fields; a push stores a field and returns, for every
 * pixel, the displacement accumulated along the trajectory that starts there and is followed through the ring's fields by chained
 * cv2.remap(field, map_x, map_y, INTER_LINEAR) calls.  On the device that is one kernel per push: a pixel walks its own chain of
 * dependent bilinear gathers, nothing intermediate is written.
 *
 * ONE REMAP (restated from OpenCV 4.x and NOT pinned against a cv2 build: DESIGN.md section 4g lists what to re-check first).
 * src (H, W, 2) float32 or float64, float32 maps, BORDER_CONSTANT with value 0; per output element:
 *   1. qx = round_half_even(map_x * 32.0f) as int32, the product in float32; qy likewise.  A coordinate that is NaN, infinite or whose
 *      product does not fit int32 samples as wholly outside: +0.0 in both channels.
 *   2. sx = clamp(qx >> 5, -32768, 32767) (arithmetic shift), ax = qx & 31; sy, ay likewise.
 *   3. fx = ax / 32, fy = ay / 32 in float32; w00 = (1-fy)(1-fx), w01 = (1-fy) fx, w10 = fy (1-fx), w11 = fy fx: exact multiples of 1/1024.
 *   4. sx >= W or sx + 1 < 0 or sy >= H or sy + 1 < 0: wholly outside, +0.0.
 *   5. otherwise, with T(r, c) the source value widened to double, or 0.0 when (r, c) is out of range, per channel
 *      ((T(sy,sx) w00 + T(sy,sx+1) w01) + T(sy+1,sx) w10) + T(sy+1,sx+1) w11 in double, every product and sum rounded on its own (no
 *      FMA).  All four products are always formed: an in-range NaN tap under a zero weight gives NaN.
 * A float32 ring that holds the same values as a float64 ring therefore gives identical bits.  A NaN result is stored as the quiet NaN
 * 0x7FF8000000000000 (float32: 0x7FC00000): whether a result is a NaN is arithmetic, its sign and payload are the machine's.
 *
 * ONE PUSH, ring of length L at index h (slots zero at creation):  ring[h] = flow;  slots = mav_history_schedule(L, h);  every pixel
 * (y, x) starts from r = y, c = x in double and does, for each s of slots in turn, (u, v) = remap(ring[s], (float)c, (float)r) (the casts
 * round to nearest even), r += u, c += v -- the reference's channel order, lookup_map[..., 0] is the row and the flow's x component is
 * added to it, kept as it is; MAV_HISTORY_AXES_XY: r += v, c += u, the geometrically consistent order --; the result is (r - y, c - x);
 * then h = (h + 1) % L.  The schedule is the reference's loop taken literally: k = (h + 1) % (L - 1); while k != h % (L - 1): emit k,
 * k = (k + 1) % L.  For L = 20: h <= 17 walks h+1 .. 19, 0 .. h-1 (19 steps, the field just stored is not read), h = 18 walks 0 .. 17
 * (18 steps), h = 19 walks 1 .. 19 (the field just stored is read).
 *
 * length 3 .. MAV_HISTORY_MAX_LENGTH; depth MAV_DEPTH_32F or MAV_DEPTH_64F, the ring's element; flags 0 or MAV_HISTORY_AXES_XY.  The
 * ring is length * W * H * 2 * sizeof(element) bytes of the context's device memory (mav_mem_info counts it; 332 MB for 20 float32
 * fields at 1080p), freed by mav_history_destroy or mav_destroy; a failed allocation is MAV_ERR_OOM and leaves nothing behind.  A context
 * may own several histories; a history is used with the context that created it only (MAV_ERR_ARG otherwise). */
#define MAV_HISTORY_MAX_LENGTH 64
#define MAV_HISTORY_AXES_XY 1           /* mav_history_params.flags */
#define MAV_HISTORY_OUT_REFERENCE 0     /* out_form: float64 (H, W, 2) = (r - y, c - x), the reference's return value */
#define MAV_HISTORY_OUT_FLOW_F32 1      /* out_form: float32 (H, W, 2) = (c - x, r - y), each rounded once from the double: the (u, v)
                                           layout mav_detect / mav_render / mav_roc_sweep take */
typedef struct mav_history mav_history; /* opaque; owned by its context */
typedef struct {
    int length, depth, flags;
} mav_history_params;                   /* mav_history_defaults: 20, MAV_DEPTH_32F, 0 */
void mav_history_defaults(mav_history_params*);
/* Pure host, no context: the slots a push at `index` of a ring of `length` walks, in order, into slots[0 .. *n); slots holds
 * length - 1 entries.  MAV_ERR_ARG for a length outside 3 .. MAV_HISTORY_MAX_LENGTH, an index outside 0 .. length - 1 or a NULL pointer. */
int mav_history_schedule(int length, int index, int* slots, int* n);
int mav_history_create(mav_ctx*, const mav_history_params* /* NULL = defaults */, mav_history** out);   /* ring zeroed, index 0 */
int mav_history_destroy(mav_ctx*, mav_history*);   /* waits for the context's stream, then frees the ring */
int mav_history_reset(mav_ctx*, mav_history*);     /* ring zeroed, index 0, pushes 0; enqueue only */
int mav_history_info(mav_ctx*, const mav_history*, int* index, long* pushes, size_t* ring_bytes);   /* any output may be NULL */
/* `count` >= 1 consecutive fields, flow (count, H, W, 2) of flow_depth (MAV_DEPTH_32F, or MAV_DEPTH_64F into a float64 ring: a float32
 * field into a float64 ring is widened, a float64 field into a float32 ring would round and is MAV_ERR_ARG), pushed and traced in order:
 * out (count, H, W, 2) in out_form.  count * W * H <= MAV_MAX_BATCH_PIXELS.  flow and out are aligned to their elements and do not
 * overlap.  Bad arguments are refused before anything is enqueued, the ring, the index and out as they were; mav_last_error names
 * the argument.  mav_history_push: host pointers, synchronous.  mav_history_push_dev: device pointers, enqueue only -- stream order keeps
 * field t's reads ahead of field t + 1's write of the oldest slot. */
int mav_history_push(mav_ctx*, mav_history*, const void* flow, int flow_depth, int count, int out_form, void* out);
int mav_history_push_dev(mav_ctx*, mav_history*, const void* flow, int flow_depth, int count, int out_form, void* out);
/* One remap, as defined above, of a W x H field: src (H, W, 2) of `depth`, map_x / map_y (H, W) float32, out (H, W, 2) float64.  Host
 * pointers, synchronous: the stage-level pin of the trajectory kernel's one body (tests/test_gpu_history.py). */
int mav_stage_remap_linear(mav_ctx*, const void* src, int depth, const float* map_x, const float* map_y, double* out);

/* Frame decode in front of the path [src/datasets/dataset.py:57,223-230: cv2.VideoCapture over image_%05d.png; src/farneback.py:17-21]:
 * the un-filtering pass of a PNG image, host memory, no context.  raw = the inflated IDAT stream of a non-interlaced image (per row a
 * filter-type byte + stride bytes), bpp = bytes per complete pixel (1 for bit depths below 8), out = rows x stride bytes.  Filters 0 - 4 of
 * the PNG specification.  MAV_ERR_ARG for any other filter type.  (zlib inflate and chunk parsing: mavflow/frame_source.py, Python stdlib.) */
int mav_png_unfilter(const uint8_t* raw, int rows, size_t stride, int bpp, uint8_t* out);

/* ---- PNG files of 8-bit images, encoded on the device -------------------------------------------------------------------------------
 * What cv2.imwrite(name + ".png", img) stores for the loop's images [src/processor.py:364-374], minus the few hundred bytes of chunk
 * framing (signature, IHDR, IDAT length + CRC, IEND: mavflow/frame_source.py png_wrap, host code): per image ONE complete RFC 1950 zlib
 * stream whose inflated bytes are the PNG scanline stream -- per row the filter-type byte 1 (Sub) and W * channels filtered bytes, gray /
 * RGB / RGBA (the B <-> R swap of a BGR(A) image happens on load).  Images are (count, H, W, channels) u8 of the context's W x H,
 * channels = 1 (gray), 3 (BGR) or 4 (BGRA); count is not bound by max_batch.  The streams of a call are packed back to back into `out`
 * from offset 0 in image order; index[i] = (offset, size) of image i.  Any inflater reads them; they are NOT the bytes zlib would
 * produce (independent 24 KB segments, byte-run matches only) and the same image gives the same bytes on every call.
 * mav_png_bound: the most bytes one image's stream can take, raw + 5 * ceil(raw / 24576) + 6 with raw = H * (1 + W * channels) -- no
 * context, no GPU; 0 for a bad argument.
 * MAV_ERR_ARG: channels not 1 / 3 / 4, count < 1, W * channels >= 2^31 - 1.  out_bytes: the _dev form needs count * mav_png_bound(...)
 * (it cannot know the sizes); the host forms accept any size and fail with MAV_ERR_ARG, naming the bytes needed, when the streams do
 * not fit -- count * mav_png_bound(...) always does.  The encoder's workspace (at most 256 MB, or one image's) is allocated by the first
 * encode call and reported by mav_mem_info. */
size_t mav_png_bound(int W, int H, int channels);
int mav_png_encode_dev(mav_ctx*, const uint8_t* imgs_dev, int count, int channels, uint8_t* out_dev, size_t out_bytes,
                       uint64_t* index_dev /* count x (offset, size) */);          /* enqueue only, on the context's stream */
int mav_png_encode(mav_ctx*, const uint8_t* imgs_host, int count, int channels, uint8_t* out_host, size_t out_bytes,
                   uint64_t* index /* count x (offset, size) */);                   /* host in / out, synchronous */
/* mav_last_render with the images encoded where they were rendered: only the index and the streams cross PCIe.  index: (images wanted)
 * x batch entries, result / flow / phi order.  MAV_ERR_STATE exactly as mav_last_render. */
int mav_last_render_png(mav_ctx*, int batch, int want_result, int want_flow, int want_phi, uint8_t* out_host, size_t out_bytes,
                        uint64_t* index);
/* mav_last_overlay likewise: frames and foe_gt up, `batch` streams and the written flags back.  MAV_ERR_* exactly as mav_last_overlay. */
int mav_last_overlay_png(mav_ctx*, const uint8_t* frames, const double* foe_gt, int batch, int radius, uint8_t* out_host,
                         size_t out_bytes, uint64_t* index, uint8_t* written);

/* ---- sparse optical flow: Shi-Tomasi corners and the pyramidal Lucas-Kanade tracker ------------------------------------------------
 * cv2.goodFeaturesToTrack [src/lucas_kanade.py:53] and cv2.calcOpticalFlowPyrLK [src/lucas_kanade.py:60] on ONE 8-bit gray frame (pair)
 * of the context's W x H per call: the sparse path is sequential, the features of call i are the tracked points of call i - 1.
 * Restated from OpenCV's published routines with every window sum kept as an exact integer sum; cv2 itself is not pinned.
 * Defaults: the reference's parameters, corners 2000 / 0.2 / 7 / 7 (Sobel aperture 3, min-eigenvalue score, no mask), tracker
 * winSize (21, 21), maxLevel 3, criteria (EPS | COUNT, 30, 0.01), flags 0, minEigThreshold 1e-4.
 * THE RESIDENT FRAME: the context keeps the frame it saw last (the `next` of mav_lk_track, or the frame given to mav_good_features) and
 * its pyramid on the device.  Passing NULL for `prev` / `gray` means that frame: a video uploads every frame once and builds its
 * pyramid once.  MAV_ERR_STATE when there is none.  The workspace (two pyramids, one derivative pyramid, the eigenvalue map, candidates,
 * points: 12 bytes per pixel + 3.2 MB; 6 898 868 bytes at 640 x 480) is allocated by the first of these calls and reported by
 * mav_mem_info.  The device sort and pick add 12 bytes to it: the sort is in place, the pick's grid of accepted corners lives in the
 * eigenvalue map (dead once the candidates are out), a host mask is staged in the frame slot that no call reads again. */
typedef struct {
    int max_corners;          /* 1 .. MAV_LK_MAX_POINTS */
    double quality_level;     /* > 0 */
    double min_distance;      /* < 1: no distance test */
    int block_size;           /* odd, 1 .. 15 */
} mav_gftt_params;
typedef struct {
    int win_w, win_h;         /* odd, 3 .. MAV_LK_MAX_WIN */
    int max_level;            /* 0 .. MAV_LK_MAX_LEVEL; lowered so that every level above 0 is wider than win_w and higher than win_h */
    int max_count;            /* clamped to [0, 100] as cv2 does */
    double epsilon;           /* clamped to [0, 10] as cv2 does */
    double min_eig_threshold;
} mav_lk_params;
#define MAV_LK_MAX_POINTS 65536     /* points per mav_lk_track call, corners per mav_good_features call */
#define MAV_LK_MAX_WIN 33           /* the tracker keeps a point's window (3 int16 planes) in LDS, four points per workgroup */
#define MAV_LK_MAX_LEVEL 7
#define MAV_GFTT_MAX_CANDIDATES 262144 /* local maxima above the quality threshold one frame may have; more is MAV_ERR_ARG, never a silent cut */
void mav_gftt_defaults(mav_gftt_params*);
void mav_lk_defaults(mav_lk_params*);
/* corners (max_corners, 2) float32 (x, y) in acceptance order (strongest first; ties by linear index, larger first), *count of them.
 * gray NULL: the resident frame; otherwise `gray` is uploaded and becomes the resident frame.  Everything runs on the device:
 * eigenvalue map, threshold, non-maximum test, candidate compaction, the sort and the greedy minimum-distance pick; the
 * call brings back the count and the corners and synchronises once. */
int mav_good_features(mav_ctx*, const uint8_t* gray, const mav_gftt_params* /* NULL = defaults */, float* corners, int* count);
/* The same with cv2's `mask` argument: (H, W) u8 or NULL (= mav_good_features bit for bit).  As cv2 does it (restated from OpenCV's
 * published routine, unpinned like the rest): quality_level multiplies the maximum of the eigenvalue map over the pixels whose mask byte
 * is non-zero; the threshold and the 3 x 3 non-maximum test see the whole map (a masked-out neighbour still suppresses); only pixels
 * with a non-zero mask byte become corners.  An all-zero mask: no corner, no error. */
int mav_good_features_ex(mav_ctx*, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params*, float* corners, int* count);
/* next_pts (n, 2) float32 and status (n) u8 for pts (n, 2) float32, 0 <= n <= MAV_LK_MAX_POINTS.  NaN / inf / far-away points are not
 * errors: they end with status 0 as in cv2.  `next` becomes the resident frame.  cv2's error output is not computed (mav_lk_track_err computes it), so this is the
 * status of a C++ call with err == NULL: the final bounds test that comes with err is not run. */
int mav_lk_track(mav_ctx*, const uint8_t* prev /* NULL: the resident frame */, const uint8_t* next, const float* pts, int n,
                 const mav_lk_params* /* NULL = defaults */, float* next_pts, uint8_t* status);
/* Device-pointer forms.  mav_lk_track_dev only enqueues (frames are copied into the workspace on the device).  mav_good_features_dev
 * takes a device frame and returns host corners: its outputs are host memory, so the call synchronises (once). */
int mav_good_features_dev(mav_ctx*, const uint8_t* gray_dev, const mav_gftt_params*, float* corners_host, int* count);
int mav_lk_track_dev(mav_ctx*, const uint8_t* prev_dev, const uint8_t* next_dev, const float* pts_dev, int n, const mav_lk_params*,
                     float* next_pts_dev, uint8_t* status_dev);
/* Corners with device pointers in AND out: only enqueues on the context's stream.  gray_dev NULL: the resident frame; mask_dev (H, W) u8
 * or NULL.  corners_dev holds max_corners x 2 floats, entries from *count_dev on are left as they were.  The host cannot see a candidate
 * overflow here: *count_dev = -(number of candidates) and no corner is written (never a silent cut). */
int mav_good_features_ex_dev(mav_ctx*, const uint8_t* gray_dev, const uint8_t* mask_dev, const mav_gftt_params*, float* corners_dev,
                             int32_t* count_dev);
/* mav_lk_track_dev sized for n_max points whose count lives on the device: waves with index >= *n_dev leave at once without touching
 * memory (all of them if *n_dev is negative); *n_dev == n_max gives the bytes of mav_lk_track_dev(n_max).  mav_lk_last_iterations counts
 * the points that ran.  With mav_good_features_ex_dev: corners -> track as one chain, no host call in between. */
int mav_lk_track_ex_dev(mav_ctx*, const uint8_t* prev_dev, const uint8_t* next_dev, const float* pts_dev, int n_max, const int32_t* n_dev,
                        const mav_lk_params*, float* next_pts_dev, uint8_t* status_dev);
/* The tracker with cv2's `err` output and cv2's two flags.  Like the rest of the sparse path this is OpenCV 4.x lkpyramid.cpp RESTATED
 * and unpinned against a cv2 build.  flags: 0 or any OR of
 *   MAV_OPTFLOW_USE_INITIAL_FLOW      next_pts is read first: a point's start at the top level is next_pts[p] * (1 / 2^level) instead of
 *                                     the scaled previous point (then next_pts must not be NULL for n > 0)
 *   MAV_OPTFLOW_LK_GET_MIN_EIGENVALS  err[p] = the float32 minimum eigenvalue the min_eig_threshold test looks at, of level 0 (written
 *                                     before that test, so a point the test rejects carries it too); 0 when level 0 fails the first
 *                                     bounds test.  Without an err buffer the flag changes nothing.
 * any other bit is MAV_ERR_ARG and nothing is enqueued.  err (n) float32 or NULL.  Without GET_MIN_EIGENVALS, err is cv2's L1 error: for
 * a point whose status is still 1 after level 0, q = next_pts[p] - halfWin; floor(q) must pass the bounds test every level uses
 * (-win <= floor < size, finite) or the STATUS BECOMES 0 and err stays 0 -- the test cv2 runs only when err is asked for, which its
 * Python call always does; otherwise err = (sum over the window of |J(q + k) - I(p + k)|) / (32 win_w win_h), the sum an exact integer
 * (< 2^24, so no summation order is involved), the division in float32.  err = 0 for every point that ends with status 0.
 * mav_lk_last_iterations does not count the error pass.  flags == 0 && err == NULL: mav_lk_track, byte for byte (no final bounds test).
 * prev NULL: the resident frame; resident-frame rules, pyramid reuse and parameter checks are mav_lk_track's. */
#define MAV_OPTFLOW_LK_GET_MIN_EIGENVALS 8      /* cv2's value; MAV_OPTFLOW_USE_INITIAL_FLOW (4) is defined above */
int mav_lk_track_err(mav_ctx*, const uint8_t* prev, const uint8_t* next, const float* pts, int n, const mav_lk_params*, int flags,
                     float* next_pts, uint8_t* status, float* err);
/* enqueue only; n_dev may be NULL (n_max points run).  Entries from min(*n_dev, n_max) on are left as they were in next_pts, status AND
 * err.  pts_dev == next_pts_dev is allowed (each wave reads its point before it writes). */
int mav_lk_track_err_dev(mav_ctx*, const uint8_t* prev_dev, const uint8_t* next_dev, const float* pts_dev, int n_max, const int32_t* n_dev,
                         const mav_lk_params*, int flags, float* next_pts_dev, uint8_t* status_dev, float* err_dev);
/* Corners with cv2's useHarrisDetector / k.  use_harris == 0: the corresponding entry point above, bit for bit.  Otherwise the map is
 * OpenCV's cornerHarris as goodFeaturesToTrack calls it (restated, unpinned): the same integer Sobel and box sums and the same scale s2
 * as the min-eigenvalue map, then a = xx s2, b = xy s2, c = yy s2, t = a + c, response = (a c - b b) - (k t) t in float32 in this order,
 * k rounded to float32 once.  Responses may be negative; a corner is always above max * quality_level > 0.  A non-finite k is
 * MAV_ERR_ARG.  Threshold, non-maximum test, mask, sort and pick are those of mav_good_features_ex. */
typedef struct { int use_harris; double k; } mav_corner_score;   /* mav_corner_score_defaults: 0, 0.04 */
void mav_corner_score_defaults(mav_corner_score*);
int mav_good_features_score(mav_ctx*, const uint8_t* gray, const uint8_t* mask, const mav_gftt_params*, const mav_corner_score* /* NULL = defaults */,
                            float* corners, int* count);
int mav_good_features_score_dev(mav_ctx*, const uint8_t* gray_dev, const uint8_t* mask_dev, const mav_gftt_params*, const mav_corner_score*,
                                float* corners_dev, int32_t* count_dev);  /* enqueue only, as mav_good_features_ex_dev */
/* What the most recent corner pick did: stats[0] = chunks of 1024 ranks it walked, stats[1] = rounds over all chunks.
 * Synchronises. */
int mav_gftt_last_pick(mav_ctx*, uint32_t* stats);
/* Iterations the tracker's loop ran per (point, level) in the most recent track call: hist[i] = how many ran i iterations
 * (i = 0: left the level at the first bounds test), MAV_LK_HIST_BINS bins, the last one = more.  Levels skipped before the loop do not count. */
#define MAV_LK_HIST_BINS 104
int mav_lk_last_iterations(mav_ctx*, uint32_t* hist);
/* size of level `level` (0 .. MAV_LK_MAX_LEVEL) of the tracker's pyramid: level l + 1 = ((w + 1) / 2, (h + 1) / 2) */
int mav_lk_level_dims(const mav_ctx*, int level, int* w, int* h);

/* HIP-event timing on the context's stream (bench.py): start/stop bracket enqueued work; stop synchronises. */
int mav_timer_start(mav_ctx*);
int mav_timer_stop(mav_ctx*, float* ms);
/* Per-kernel-class profiling with HIP events (separate pass, never inside a timed region).  on = 1: events around every launch
 * (durations and launch counts per class); on = 2: events around every RUN of consecutive launches of one class on a stream -- a tenth
 * of the events, for mav_profile_busy, which then sees the two streams overlap almost undisturbed (total_ms / launches then count runs).
 * mav_profile_get: name[i] / total_ms[i] / launches[i] for i < *n (caller passes capacity in *n). */
int mav_profile_enable(mav_ctx*, int on);
int mav_profile_get(mav_ctx*, int* n, const char** names, double* total_ms, long* launches);
/* Milliseconds during which at least one launch of the named kernel classes (comma-separated, names as mav_profile_get reports
 * them) was running in the profiled calls: the union of the launches' intervals.  With two pairs in flight (option
 * "pairs_in_flight") launches of one class overlap and their summed durations exceed the wall time. */
int mav_profile_busy(mav_ctx*, const char* names, double* busy_ms);
/* The profiled launches (mode 1) or runs of launches (mode 2) themselves, as intervals: class index in mav_profile_get's order, stream
 * (0 = the context's stream, 1 = its second compute stream), start / end in ms since mav_profile_enable.  *n = capacity in, count out;
 * with NULL arrays *n returns the number of intervals.  tools/untraced_anatomy.py builds the step's timeline from it without a tracer. */
int mav_profile_intervals(mav_ctx*, int* n, int* kernel_class, int* stream, float* t0_ms, float* t1_ms);

/* Calibration for the roofline record: GB/s this GPU delivers, now, to a plain streaming kernel with the sweep kernel's mix of
 * 3 reads : 1 write (four temporary buffers of bytes_per_buffer each, float4 per thread, `reps` timed launches on the context's
 * stream).  4 x 32 MB stays inside the 256 MB Infinity Cache, 4 x 1 GB does not. */
int mav_membw_probe(mav_ctx*, size_t bytes_per_buffer, int reps, double* gbs);

/* multi-GPU: gather `bytes_per_rank` bytes from every rank (RCCL ncclAllGather over xGMI) on the context's stream.
 * comm is an ncclComm_t created by the caller (mav_comm_* helpers below wrap RCCL's own bootstrap). */
/* One line of JSON: the HIP version libmavflow was built with, the HIP runtime / driver versions the process actually runs (in the
 * multi-GPU bench torch loads its own runtime first and libmavflow binds to it) and RCCL's version once it is loaded (0 before).
 * mav_comm_init returns MAV_ERR_STATE when the running runtime's major version differs from the build's. */
int mav_runtime_info(char* buf, size_t cap);
int mav_comm_unique_id(void* id128 /* 128 bytes out */);
int mav_comm_init(mav_ctx*, const void* id128, int rank, int nranks, void** comm_out);
int mav_comm_count(void* comm, int* nranks); /* ncclCommCount: the ranks the communicator really spans */
int mav_comm_destroy(void* comm);
int mav_allgather_results(mav_ctx*, void* comm, const void* local_dev, size_t bytes_per_rank, void* all_dev);

/* ---- stage hooks (diagnostics / parity tests; host pointers, one image or pair, SoA planes) ------------- */
/* layer image I_k of one frame: convertTo(f32) -> GaussianBlur -> resize   (h_k, w_k) */
int mav_stage_blur_resize(mav_ctx*, const uint8_t* img, int k, float* out);
/* the same through the separable two-pass kernels (H x w scratch in memory) that layers with a long Gaussian use: layers with a
 * short one go through ONE fused kernel in the product path, and the two forms must agree bit for bit */
int mav_stage_blur_resize_two_pass(mav_ctx*, const uint8_t* img, int k, float* out);
/* either of the two for a frame of a MAV_DEPTH_* depth (two_pass != 0: the two-pass form) */
int mav_stage_blur_resize_ex(mav_ctx*, const void* img, int depth, int k, int two_pass, float* out);
/* FarnebackPolyExp of a (h, w) f32 image at layer k -> R as 5 planes (5, h, w) */
int mav_stage_polyexp(mav_ctx*, const float* I, int k, float* R);
/* FarnebackUpdateMatrices at layer k: R0, R1 (5,h,w), flow (h,w,2) -> M (5,h,w) */
int mav_stage_update_matrices(mav_ctx*, const float* R0, const float* R1, const float* flow, int k, float* M);
/* the initial M of layer k as a call builds it: from the coarser layer's flow flow_coarse (h_(k+1), w_(k+1), 2), upsampled to
 * layer k and times 1 / pyr_scale inside the kernel, or from a zero flow when flow_coarse is NULL (MAV_ERR_ARG at the top layer) */
int mav_stage_update_matrices_from(mav_ctx*, const float* R0, const float* R1, const float* flow_coarse, int k, float* M);
/* the initial flow of layer k from a frame-size field flow0 (H, W, 2): resize(INTER_AREA) to (h_k, w_k), times pyr_scale^k */
int mav_stage_initial_flow(mav_ctx*, const float* flow0, int k, float* out);
/* one FarnebackUpdateFlow_Blur sweep (FarnebackUpdateFlow_GaussianBlur on a context with MAV_WINDOW_GAUSSIAN) at layer k:
 * M (5,h,w) -> flow (h,w,2) and, if update != 0, M_out (5,h,w) */
int mav_stage_blur_iter(mav_ctx*, const float* R0, const float* R1, const float* M, int k, int update, float* flow,
                        float* M_out);

/* The phi / mask / box stage exactly as the fused path runs it (float32 flow from the flow stage, derotation on the fly,
 * double arithmetic, single-precision screen when phi == NULL) but with a caller-supplied FoE (batch, 2) instead of the RANSAC
 * fit: lets a test plant pixels around every threshold for a known FoE.  omega / dt / sky / phi / masks / box may be NULL;
 * box (batch, 4) = x0, y0, x1, y1 of the fixed mask. */
int mav_stage_phi_mask(mav_ctx*, const float* flow, const double* foe, const double* omega, const double* dt, const uint8_t* sky,
                       int batch, const mav_thr_params*, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, int32_t* box);

/* The constants the flow kernels run on, as the library derived them (parity tests compare them with an independent
 * derivation): FarnebackPrepareGaussian(poly_n, poly_sigma) -> g, xg, xxg (poly_n + 1 floats each, centre tap first) and
 * ig = {ig11, ig03, ig33, ig55}; and, when k >= 0, layer k's GaussianBlur taps (its ksize floats).  Any pointer may be NULL. */
int mav_stage_coefficients(mav_ctx*, int k, float* g, float* xg, float* xxg, float* ig, float* blur_taps);

/* pyramid level `level` (>= 0) of one u8 image: (h_l, w_l) u8, sizes from mav_pyramid_dims */
int mav_stage_pyramid_level(mav_ctx*, const uint8_t* img, double scale, int level, uint8_t* out);

/* sparse optical flow, one u8 image each (the resident frame is dropped): level `level` of the tracker's pyramid (h_l, w_l) u8; that
 * level's Scharr pairs (h_l, w_l, 2) int16 = (Ix, Iy); the min-eigenvalue map (H, W) float32 of mav_good_features for a block size */
int mav_stage_lk_pyramid(mav_ctx*, const uint8_t* img, int level, uint8_t* out);
int mav_stage_lk_scharr(mav_ctx*, const uint8_t* img, int level, int16_t* out);
int mav_stage_min_eigen(mav_ctx*, const uint8_t* img, int block_size, float* out);
/* the same map with a score: the Harris response for use_harris != 0, mav_stage_min_eigen's bytes otherwise (NULL = defaults) */
int mav_stage_corner_response(mav_ctx*, const uint8_t* img, int block_size, const mav_corner_score*, float* out);
/* the device sort and pick of mav_good_features on n host candidate keys, (value bits << 32) | linear index: distinct, index < W * H,
 * any order, n <= MAV_GFTT_MAX_CANDIDATES.  quality_level and block_size are not used.  The resident frame stays. */
int mav_stage_corner_pick(mav_ctx*, const uint64_t* keys, int n, const mav_gftt_params*, float* corners, int* count);

/* ---- global-motion subtraction: the homography branch of Processor.run_detection [src/processor.py:286-303] ------------------------
 * Detector.get_transformation_matrix [src/detector.py:119-151, HOMOGRAPHY] and Detector.flow_vec_subtract [:153-202].
 *
 * The fit follows cv2.findHomography(src, dst) with method 0 in structure -- a normalised DLT over all pairs (the eigenvector of the
 * smallest eigenvalue of the 9x9 LtL by cyclic Jacobi), then at most MAV_HOMOGRAPHY_LM_ITERATIONS Levenberg-Marquardt evaluations on the
 * reprojection error, H scaled to H[2][2] == 1 -- in float64 with every sum over the pairs taken in index order, so that
 * tests/global_motion_ref.py reproduces its bytes.  It is NOT pinned against cv2.  ok[b] == 0 and H[b] all zero when
 * the pairs of item b do not determine a homography (a coordinate without spread, collinear or repeated points) or an entry is not
 * finite.  n >= 4 pairs per item, the same n for every item; src / dst (batch, n, 2) float64 (x, y); H (batch, 9) float64 row-major. */
#define MAV_HOMOGRAPHY_LM_ITERATIONS 10
#define MAV_HOMOGRAPHY_MAX_PAIRS 65536
int mav_find_homography(mav_ctx*, const double* src, const double* dst, int n, int batch, double* H, int32_t* ok);
int mav_find_homography_dev(mav_ctx*, const double* src, const double* dst, int n, int batch, double* H, int32_t* ok);   /* enqueue only */
/* The pairs of [:126-128] from a flow field, then the fit: src = coords, dst = coords + flow[y, x].  flow (batch, H, W, 2) float32;
 * coords (n, 2) int32 (x, y) inside the frame (host memory in both forms: they are range-checked), shared by the items.
 * pairs_dst: NULL, or (batch, n, 2) float64 receiving dst (the reference's coords_new). */
int mav_flow_homography(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, double* H, int32_t* ok, double* pairs_dst);
int mav_flow_homography_dev(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, double* H, int32_t* ok);  /* flow, H, ok: device */
/* One item of mav_global_motion: the largest residual magnitude and its first position [:180-181], analyze_pyramid's record of the
 * normalised image (as mav_analyze_pyramid's out) and the window after optimize_window (optimize == 0: analyze_pyramid's own window
 * x, y, 64, 64 -- all zero when no window scored -- and opt_score 0). */
typedef struct {
    float max_mag;
    int32_t max_row, max_col;
    int32_t reserved;
    int64_t window[6];        /* score, x, y, level, argmax_row, argmax_col */
    int64_t opt_score;
    int32_t opt_window[4];    /* x, y, w, h */
} mav_motion_result;
/* flow_vec_subtract without its renderings.  M (batch, 6) float64 = rows 0 and 1 of the homography, or the 2x3 affine matrix.  Per pixel
 * global_motion = float32(((m00 x + m01 y) + m02) - x) (float64 inside), warped = global_motion - flow, mag = sqrt(w0 w0 + w1 w1) in
 * float32; gray = one channel of im_helpers.to_rgb(mag): around((|mag| * 255) / max(mag)) in float32, half to even, all zero when the
 * maximum is 0; then analyze_pyramid(scale) and, with optimize != 0, optimize_window from its window, on the device image.
 * warped (batch, H, W, 2) float32, mag (batch, H, W) float32, gray (batch, H, W) u8: optional (NULL).  results (batch).
 * MAV_ERR_ARG as mav_analyze_pyramid for scale <= 1 or an integer-ratio pyramid level. */
int mav_global_motion(mav_ctx*, const float* flow, const double* M, int batch, double scale, int optimize, float* warped, float* mag,
                      uint8_t* gray, mav_motion_result* results);
int mav_global_motion_dev(mav_ctx*, const float* flow, const double* M, int batch, double scale, int optimize, float* warped, float* mag,
                          uint8_t* gray, mav_motion_result* results);                                           /* enqueue only */
/* One iteration of the branch for device-resident flow, enqueue only: gather, fit, subtract, window search; the matrix never visits
 * the host.  coords: host (n, 2) int32.  H (batch, 9), ok (batch), gray (batch, H, W): optional device outputs; results (batch): device.
 * An item whose fit failed (ok == 0) gets an all-zero record. */
int mav_global_motion_step_dev(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, double scale, int optimize, double* H,
                               int32_t* ok, uint8_t* gray, mav_motion_result* results);
/* processor.py:286-303 for `batch` frame pairs as one call: Farneback(prev, next) -> pairs at coords -> homography fit ->
 * subtraction -> normalised image -> analyze_pyramid (-> optimize_window).  prev / next as in mav_farneback (the frame-sequence
 * layout next == prev + W*H is recognised; the context's window is followed); coords (n, 2) int32 host, range-checked, shared
 * by the items; scale / optimize / results / gray / H / ok as in mav_global_motion_step_dev.  flow: optional (batch, H, W, 2)
 * float32 output (NULL: the context's own flow buffer, mav_last_flow_dev reports it).  Every argument is checked before anything
 * is enqueued.  mav_last_global_motion_render works after it as after the step. */
int mav_global_motion_batch(mav_ctx*, const uint8_t* prev, const uint8_t* next, const int32_t* coords, int n, int batch, double scale,
                            int optimize, float* flow, double* H, int32_t* ok, uint8_t* gray, mav_motion_result* results);      /* host pointers, synchronous */
int mav_global_motion_batch_dev(mav_ctx*, const uint8_t* prev, const uint8_t* next, const int32_t* coords, int n, int batch, double scale,
                                int optimize, float* flow, double* H, int32_t* ok, uint8_t* gray, mav_motion_result* results);  /* device pointers except coords; enqueue only */
/* get_flow_vis of flow_uv_warped and of global_motion [:179,202] for the most recent mav_global_motion(_dev) / mav_global_motion_step_dev /
 * mav_global_motion_batch(_dev) on this context, from its resident flow and matrix: (batch, H, W, 3) u8 BGR each, either may be NULL.  Host outputs, synchronous.
 * MAV_ERR_STATE under mav_last_render's rules: no such call precedes, its batch differs, or a later call may have overwritten its flow. */
int mav_last_global_motion_render(mav_ctx*, int batch, uint8_t* img_warped, uint8_t* img_global);

#ifdef __cplusplus
}
#endif
#endif /* MAVFLOW_H */

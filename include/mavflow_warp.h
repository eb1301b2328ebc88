/* libmavflow -- image warps on the device: cv2.remap, cv2.warpAffine and cv2.warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0,
 * Farneback.warp_flow (src/farneback.py:63-69) fused, and Detector.warp_method (src/detector.py:204-240) in one pass.
 *
 * A header of its own beside mavflow.h, like mavflow_truth.h, mavflow_validation.h and mavflow_cluster.h: the entry points here KEEP
 * everything a context holds resident -- every mav_last_* reader returns after them what it returned before.  They run on the context's
 * stream and hold no device memory of the context's: the `_dev` forms take device pointers and only enqueue, the host forms take staging
 * blocks behind the last call's, run, synchronise and give the blocks back.  Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*,
 * mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * Source and destination are both the context's W x H (a destination of another size is not built); `batch` images, 1 .. max_batch.
 * Interpolation is INTER_LINEAR and the border BORDER_CONSTANT with value 0: the calls take no argument for either.
 *
 * The definitions below are OpenCV 4.x modules/imgproc/src/imgwarp.cpp AS REMEMBERED and are NOT pinned against a cv2 build (none is
 * available to this project), like mavflow.h's "ONE REMAP".  What to re-check first against one: (1) the perspective coordinate, taken
 * here per pixel where OpenCV evaluates X0 + M0 * x1 relative to the start of a 32-pixel block -- the two differ in the last bit of a
 * double before a rounding to 1/32 px; (2) the order of the float32 sum under OpenCV's SIMD paths; (3) the int16 weight table (below).
 * tests/warp_ref.py is this text in numpy; the device equals it byte for byte.
 *
 * SAMPLING, given a position (qx, qy) in 1/32 pixel as int32, or "wholly outside":
 *   1. steps 2 - 4 of mavflow.h's ONE REMAP: sx = clamp(qx >> 5, -32768, 32767) (arithmetic shift), ax = qx & 31; sy, ay likewise;
 *      fx = ax / 32, fy = ay / 32 in float32, w00 = (1-fy)(1-fx), w01 = (1-fy) fx, w10 = fy (1-fx), w11 = fy fx (exact multiples of 1/1024);
 *      sx >= W or sx + 1 < 0 or sy >= H or sy + 1 < 0 is wholly outside.  A wholly-outside element is 0 (+0.0) in every channel.
 *      T(r, c) is the source value, or 0 where (r, c) is out of range.
 *   2. float32 formats, per channel: ((T(sy,sx) w00 + T(sy,sx+1) w01) + T(sy+1,sx) w10) + T(sy+1,sx+1) w11 IN FLOAT32, every product and
 *      sum rounded on its own (no FMA): cv2's remapBilinear<Cast<float, float>>.  (The history's remap sums in double and stays what it is.)
 *   3. All four products are always formed: an in-range NaN tap under a zero weight gives NaN.  A NaN result is stored as the quiet NaN
 *      0x7FC00000.
 *   4. uint8 formats, per channel: integer weights W_k = 32768 w_k = 32 (32 - ay | ay)(32 - ax | ax), exact, summing to 32768, held in
 *      int32; out = (T00 W00 + T01 W01 + T10 W10 + T11 W11 + 16384) >> 15.
 *   5. OpenCV keeps these weights in int16, where 32768 saturates to 32767; that happens only with the other three weights at 0, where
 *      (T * 32767 + 16384) >> 15 = T = (T * 32768 + 16384) >> 15 for every byte T: the same byte.
 *
 * COORDINATES -> (qx, qy).  x, y: the destination column and row.
 *   map forms (mav_remap: map_xy[y][x] = (mx, my); mav_remap_planes: map_x[y][x], map_y[y][x]):
 *      step 1 of ONE REMAP: qx = round_half_even(mx * 32.0f) as int32, the product in float32; qy likewise.  A product that is NaN,
 *      infinite or does not fit int32 (either one) makes the element wholly outside.
 *   mav_warp_flow: mx = (float)x + (-u), my = (float)y + (-v) with (u, v) = flow[y][x], each ONE float32 addition (what numpy's in-place
 *      float32 += int64 of Farneback.warp_flow yields); then as the map forms.  No map is read or written.
 *   affine (M = M0 .. M5, row-major 2 x 3, double):
 *      without MAV_WARP_INVERSE_MAP, M is first inverted in double, in this order (every operation rounded on its own):
 *        D = M0*M4 - M1*M3;  D = D != 0 ? 1/D : 0;  A11 = M4*D;  A22 = M0*D;  M0 = A11;  M1 = M1*(-D);  M3 = M3*(-D);  M4 = A22;
 *        b1 = (-M0)*M2 - M1*M5;  b2 = (-M3)*M2 - M4*M5;  M2 = b1;  M5 = b2
 *      X0 = rint((M1*y + M2) * 1024) + 16;   qx = (X0 + rint((M0*x) * 1024)) >> 5      (AB_BITS = 10, round_delta = 16)
 *      Y0 = rint((M4*y + M5) * 1024) + 16;   qy = (Y0 + rint((M3*x) * 1024)) >> 5
 *      rint rounds half to even and saturates to int32 (a NaN gives INT_MIN); the additions are int32 with wrap-around; the shift is
 *      arithmetic.  No element is wholly outside by its coordinates' range.
 *   perspective (M = M0 .. M8, row-major 3 x 3, double):
 *      without MAV_WARP_INVERSE_MAP, M is first inverted by the cofactor formula, det3 along the first row:
 *        d = (M0*(M4*M8 - M5*M7) - M1*(M3*M8 - M5*M6)) + M2*(M3*M7 - M4*M6);  d = d != 0 ? 1/d : 0
 *        N0 = (M4*M8 - M5*M7)*d;  N1 = (M2*M7 - M1*M8)*d;  N2 = (M1*M5 - M2*M4)*d
 *        N3 = (M5*M6 - M3*M8)*d;  N4 = (M0*M8 - M2*M6)*d;  N5 = (M2*M3 - M0*M5)*d
 *        N6 = (M3*M7 - M4*M6)*d;  N7 = (M1*M6 - M0*M7)*d;  N8 = (M0*M4 - M1*M3)*d;   M = N
 *      per pixel in double: Wd = (M6*x + M7*y) + M8;  Wd = Wd != 0 ? 32/Wd : 0
 *        fX = ((M0*x + M1*y) + M2) * Wd;  fY = ((M3*x + M4*y) + M5) * Wd
 *      a NaN fX or fY makes the element wholly outside; otherwise each is clamped to [INT_MIN, INT_MAX] and qx = (int)rint(fX),
 *      qy = (int)rint(fY) (half to even).
 *   A zero determinant gives the zero matrix (the `_dev` forms follow the formulas; the host forms refuse it, below).
 *
 * WARP METHOD (Detector.warp_method :213-224), one pass over a float32 (u, v) field:
 *   stable = warp(flow, M) as mav_warp_affine / mav_warp_perspective on MAV_WARP_F32C2 with flags 0 (M is inverted, as cv2 does)
 *   per element c = 0, 1:  diff_c = (stable_c == 0) ? flow_reset_c - stable_c : flow_c - stable_c,  flow_reset_c = stable_c  -- the
 *     reference's flow_uv[mask] = flow_uv_stable[mask] taken literally, element-wise; float32
 *   mag = sqrtf(d0*d0 + d1*d1) in float32 without FMA (bit for bit the magnitude mav_global_motion produces from the same d0, d1); NaN
 *     results of diff and mag are stored as 0x7FC00000
 *   per image a mav_warp_record: the largest mag (a NaN counts as larger than every number, as numpy's argmax has it) and the row and
 *     column of its FIRST raster position.  Taken with integer atomics on (float bits << 32 | ~pixel index): no floating-point atomic,
 *     the same bytes on every run and at every batch position.  The call itself initialises the records; every byte is written.
 *   The `blocks` arithmetic of :229-237 is dead code in the reference (its result is discarded) and is not built. */
#ifndef MAVFLOW_WARP_H
#define MAVFLOW_WARP_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_WARP_U8C1  0            /* format: uint8, 1 channel */
#define MAV_WARP_U8C3  1            /* uint8, 3 channels (interleaved) */
#define MAV_WARP_F32C1 2            /* float32, 1 channel */
#define MAV_WARP_F32C2 3            /* float32, 2 channels (interleaved): a flow field */
#define MAV_WARP_INVERSE_MAP 16     /* flags: M maps destination to source already (cv2.WARP_INVERSE_MAP) */
#define MAV_WARP_AFFINE 0           /* mav_warp_method's kind: M is (batch, 2, 3) */
#define MAV_WARP_PERSPECTIVE 1      /* M is (batch, 3, 3) */

typedef struct {
    float   max_mag;    /* the largest magnitude of the image */
    int32_t row, col;   /* its first raster position */
    int32_t pad;        /* 0 */
} mav_warp_record;      /* 16 bytes; every byte is written */

/* src, dst: (batch, H, W, channels) of `format`; they do not overlap.  map_xy (batch, H, W, 2) float32; map_x, map_y (batch, H, W)
 * float32; flow (batch, H, W, 2) float32; M (batch, 2, 3) or (batch, 3, 3) double.
 * MAV_ERR_ARG: a NULL pointer; a format that is none of the four; flags other than 0 or MAV_WARP_INVERSE_MAP; batch outside
 *   [1, max_batch]; a kind that is neither MAV_WARP_AFFINE nor MAV_WARP_PERSPECTIVE;
 *   host forms: a non-finite matrix element; without MAV_WARP_INVERSE_MAP (and in mav_warp_method) a matrix whose determinant D / d,
 *   taken as above, is 0 or not finite;
 *   _dev forms: src / dst not aligned to their element (float32 formats: 4), maps and flow not aligned to 4, M to 8, records to 16. */
int mav_remap(mav_ctx*, const void* src, int format, const float* map_xy, int batch, void* dst);
int mav_remap_dev(mav_ctx*, const void* src, int format, const float* map_xy, int batch, void* dst);
int mav_remap_planes(mav_ctx*, const void* src, int format, const float* map_x, const float* map_y, int batch, void* dst);
int mav_remap_planes_dev(mav_ctx*, const void* src, int format, const float* map_x, const float* map_y, int batch, void* dst);
int mav_warp_flow(mav_ctx*, const void* img, int format, const float* flow, int batch, void* dst);
int mav_warp_flow_dev(mav_ctx*, const void* img, int format, const float* flow, int batch, void* dst);
int mav_warp_affine(mav_ctx*, const void* src, int format, const double* M, int flags, int batch, void* dst);
int mav_warp_affine_dev(mav_ctx*, const void* src, int format, const double* M, int flags, int batch, void* dst);
int mav_warp_perspective(mav_ctx*, const void* src, int format, const double* M, int flags, int batch, void* dst);
int mav_warp_perspective_dev(mav_ctx*, const void* src, int format, const double* M, int flags, int batch, void* dst);
/* diff (batch, H, W, 2) float32 and mag (batch, H, W) float32 may each be NULL; records: `batch` blocks, not NULL. */
int mav_warp_method(mav_ctx*, const float* flow, const double* M, int kind, int batch, float* diff, float* mag, mav_warp_record* records);
int mav_warp_method_dev(mav_ctx*, const float* flow, const double* M, int kind, int batch, float* diff, float* mag, mav_warp_record* records);

#ifdef __cplusplus
}
#endif
#endif

/* libmavflow -- image resize on the device: cv2.resize with INTER_NEAREST, INTER_LINEAR and INTER_AREA (shrinking), and the sky mask of
 * Dataset.get_sky_segmentation (src/datasets/dataset.py:152-158) -- the half-resolution prediction resized and keyed -- fused in one pass.
 *
 * A header of its own beside mavflow.h, like mavflow_warp.h, whose four pixel formats it reuses: the entry points here KEEP everything a
 * context holds resident -- every mav_last_* reader returns after them what it returned before.  They run on the context's stream and
 * hold no device memory of the context's: the `_dev` forms take device pointers, allocate nothing and only enqueue (one launch), the host
 * forms take staging blocks behind the last call's, run, synchronise and give the blocks back.  Conventions are mavflow.h's: 0 = OK,
 * < 0 = MAV_ERR_*, mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * Source (sw x sh) and destination (dw x dh) are independent of the context's W x H; every side is in [1, 32767]; `batch` images.
 *
 * The definitions below are as remembered from OpenCV 4.x `modules/imgproc/src/resize.cpp`, NOT pinned against a cv2 build (none is
 * available to this project).  The text of this header IS the definition: tests/resize_ref.py is this text in numpy and the device equals
 * it byte for byte.  What to re-check first against a cv2 build:
 *   (1) the scale: taken here as (double)sw / dw, where hal::resize computes 1. / ((double)dw / sw) -- the two can differ in the last bit
 *       (the pyramid's and the initial flow's private resize in kernels_window.hip keep the second form and stay what they are);
 *   (2) cv2's SIMD helper for one-channel float32 and its summation order (fast area form, 2 x 2 blocks of cn 1 / 4), taken here as
 *       the scalar loop for one and two channels alike;
 *   (3) the u8 linear path: the 11-bit coefficients, the three truncating shifts of the vertical pass, and whether a build's own
 *       HAL / IPP / bit-exact path (INTER_LINEAR of 8-bit images takes one in some builds) replaces it;
 *   (4) the float32 linear path's one-tap region (dx >= xmax: a single product) and its always-two-product vertical pass;
 *   (5) INTER_NEAREST's index: floor(dx * scale_x), against the builds that compute it from a rounded fixed-point step;
 *   (6) the 1e-3 thresholds and the cell width of the general area table (area_span).
 *
 * SCALE.  scale_x = (double)sw / dw, scale_y = (double)sh / dh.  Every float32 product and sum below is rounded on its own: no FMA.
 *
 * DISPATCH, as cv::resize does it, in this order:
 *   1. dw == sw && dh == sh is a copy of the bytes, for every interpolation.
 *   2. MAV_INTER_LINEAR becomes MAV_INTER_AREA when both ratios are the whole number 2: |scale_x - 2| < DBL_EPSILON and
 *      |scale_y - 2| < DBL_EPSILON.
 *   3. Otherwise the named method runs.
 *
 * NEAREST.  sx = min((int)floor(dx * scale_x), sw - 1), sy = min((int)floor(dy * scale_y), sh - 1) with the product in double; all
 *   channels of the source pixel are copied (bytes, a NaN's payload included).
 *
 * LINEAR, the table of one axis (d: destination index, ssize: the source's side):
 *   f = (float)((d + 0.5) * scale - 0.5), the expression evaluated in double and rounded to float32 once;  s = floor(f);
 *   a = f - (float)s in float32;  then s < 0 gives s = 0, a = 0;  then s >= ssize - 1 gives s = ssize - 1, a = 0 -- horizontally this
 *   marks the ONE-TAP REGION.  (sx, a) is the horizontal pair, (sy, b) the vertical one.
 * LINEAR, float32 formats, per channel:
 *   horizontal: h = S[s] * (1.f - a) + S[s + 1] * a, both products always formed; in the one-tap region h = S[s] * 1.f;
 *   vertical, both products always formed: out = h(row sy) * (1.f - b) + h(row min(sy + 1, sh - 1)) * b.
 *   So an infinite tap under a zero weight gives NaN, as in cv2's generic path (left of the first source column S[1] is such a tap).
 *   A NaN result is stored as 0x7FC00000.
 * LINEAR, uint8 formats, per channel:
 *   coefficients a0 = round_half_even((1.f - a) * 2048.f), a1 = round_half_even(a * 2048.f), saturated to int16; b0, b1 likewise from b;
 *   horizontal: h = S[s] * a0 + S[s + 1] * a1 in int32; in the one-tap region h = S[s] * 2048;
 *   vertical: out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2 with h0 of row sy and h1 of row min(sy + 1, sh - 1);
 *   all shifts are arithmetic; the result is clamped to [0, 255].
 *
 * AREA is built for dw <= sw and dh <= sh only (where it enlarges OpenCV falls to another coefficient scheme: refused).
 *   ix = (int)round_half_even(scale_x), iy likewise; the FAST form runs when |scale_x - ix| < DBL_EPSILON and |scale_y - iy| <
 *   DBL_EPSILON, the GENERAL form otherwise.
 * AREA, fast form (the block of destination (dx, dy) is source rows dy*iy .. dy*iy + iy - 1, columns dx*ix .. dx*ix + ix - 1):
 *   uint8 with ix == iy == 2: (S00 + S01 + S10 + S11 + 2) >> 2.  NOTE this rounds a half UP, where the other uint8 area forms (next
 *     line, and the general form) round a half to EVEN;
 *   other uint8: the int32 sum over the block, rows then columns, then rintf((float)sum * (1.f / (ix * iy))) -- the reciprocal taken in
 *     float32, rintf rounding half to even -- clamped to [0, 255];
 *   float32, one and two channels alike: the float sum over the block in row-then-column order, grouped four at a time as the unrolled
 *     scalar loop adds them (sum += ((t0 + t1) + t2) + t3, then the rest one by one), times 1.f / (ix * iy).
 * AREA, general form (any ratio that is not whole on both axes), per axis and destination index d (area_span):
 *   f1 = d * scale, f2 = f1 + scale, cell = min(scale, ssize - f1) in double;  s1 = ceil(f1), s2 = min(floor(f2), ssize - 1),
 *   s1 = min(s1, s2);  taps in this order: (s1 - 1, (float)((s1 - f1) / cell)) if s1 - f1 > 1e-3;  (s, (float)(1 / cell)) for
 *   s = s1 .. s2 - 1;  (s2, (float)(min(min(f2 - s2, 1), cell) / cell)) if f2 - s2 > 1e-3.
 *   per channel: buf(row) = sum over the x taps in order of (float)S[row][s] * alpha, from 0.f; out = sum over the y taps in order of
 *   beta * buf(row), from 0.f; every product and sum float32 (area_row / area_general).
 *   uint8 output is rintf (half to even) with a clamp to [0, 255]; float32 output is the float sum.
 * Every COMPUTED float32 result (linear and both area forms) that is NaN is stored as 0x7FC00000; the copy and NEAREST move bits.
 *
 * SKY MASK.  mav_sky_mask is mav_resize(MAV_WARP_U8C3, MAV_INTER_LINEAR) of the prediction -- the dispatch above included: dw == sw &&
 *   dh == sh is the key of the picture itself, an exact halving takes the area form -- followed by
 *   sky = (c0 == key0 && c1 == key1) ? 1 : 0 per pixel, as (batch, dh, dw) uint8: the layout every `sky` argument of mavflow.h and
 *   mav_frame_step.sky_dev take.  One pass: the three-channel picture is never written.  Its bytes equal those of the two-step route. */
#ifndef MAVFLOW_RESIZE_H
#define MAVFLOW_RESIZE_H

#include "mavflow_warp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_INTER_NEAREST 0         /* interpolation: cv2.INTER_NEAREST */
#define MAV_INTER_LINEAR  1         /* cv2.INTER_LINEAR */
#define MAV_INTER_AREA    3         /* cv2.INTER_AREA */
#define MAV_RESIZE_MAX_SIDE 32767   /* every side of a source or a destination is in [1, MAV_RESIZE_MAX_SIDE] */

/* src (batch, sh, sw, channels) and dst (batch, dh, dw, channels) of `format` (MAV_WARP_U8C1, _U8C3, _F32C1, _F32C2);
 * pred_bgr (batch, sh, sw, 3) uint8, sky (batch, dh, dw) uint8.
 * MAV_ERR_ARG, with the function's name in mav_last_error(): a NULL pointer; a format that is none of the four; an interpolation that is
 *   none of the three; a side outside [1, 32767]; a key outside [0, 255]; batch < 1, or batch above the context's max_batch;
 *   MAV_INTER_AREA with dw > sw or dh > sh; source and destination that overlap;
 *   _dev forms: float32 src / dst not aligned to 4. */
int mav_resize(mav_ctx*, const void* src, int format, int sw, int sh, int dw, int dh, int interpolation, int batch, void* dst);
int mav_resize_dev(mav_ctx*, const void* src, int format, int sw, int sh, int dw, int dh, int interpolation, int batch, void* dst);
int mav_sky_mask(mav_ctx*, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int batch, uint8_t* sky);
int mav_sky_mask_dev(mav_ctx*, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int batch, uint8_t* sky);

#ifdef __cplusplus
}
#endif
#endif

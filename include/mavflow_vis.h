/* libmavflow -- flow pictures on the device: the HSV picture of a flow field as Farneback.process() (src/farneback.py:83-95) and
 * Farneback.draw_hsv (:50-60) compose it, cv2.cvtColor's COLOR_HSV2BGR and COLOR_BGR2HSV on uint8 x 3, and Farneback.draw_flow's
 * (:28-48) field of lines.
 *
 * A header of its own beside mavflow.h: the entry points here KEEP everything a context holds resident -- every mav_last_* reader, the
 * resident pyramids, the history rings and the accumulators return after them what they returned before.  They run on the context's
 * stream, write only what the caller passes in and hold no device memory of the context's: the `_dev` forms take device pointers,
 * allocate nothing and only enqueue, the host forms take staging blocks behind the last call's, run, synchronise and give the blocks
 * back.  Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message.  A refused call has enqueued and
 * written nothing.  All images are the context's W x H; `batch` of them.
 *
 * Every float32 product, sum, quotient and square root below is rounded on its own (no FMA, correctly rounded '/' and sqrt).
 *
 * HSV -> BGR, one uint8 triple (h, s, v) -- mavflow.farneback.hsv_to_bgr, which is the definition, for EVERY triple (h >= 180 and
 *   s = 0 included):  hf = (float)h * (float)(6.0 / 180.0);  sf = (float)s / 255.f;  vf = (float)v / 255.f;  sector = floor(hf);
 *   f = hf - sector;  sector %= 6;  t0 = vf, t1 = vf * (1 - sf), t2 = vf * (1 - sf * f), t3 = vf * (1 - sf * (1 - f));  (b, g, r) =
 *   (t1, t3, t0), (t1, t0, t2), (t3, t0, t1), (t0, t2, t1), (t0, t1, t3), (t2, t1, t0) for sector 0 .. 5;  each channel
 *   clip(rint(x * 255.f), 0, 255), rint rounding a half to even.
 *
 * MAV_HSV_PROCESS -- mavflow.farneback.flow_to_hsv then hsv_to_bgr, which are the definition, bit for bit up to atan2f:
 *   mag = sqrt(fx * fx + fy * fy);  lo, hi: the image's minimum and maximum of mag;
 *   scale = (float)(255.0 / ((double)hi - (double)lo)), the double quotient rounded once; scale = 0 when hi - lo <= DBL_EPSILON;
 *   norm = (mag - lo) * scale;  value = trunc(norm * 2.f) & 255 (the upper half of the range wraps: intended);
 *   ang = atan2f(fy, fx), + (float)(2 pi) where negative;  hue = trunc(((ang * 180.f) / (float)pi) / 2.f) & 255;  saturation 255;
 *   a pixel whose value is 0 becomes (127, 255, 255);  then HSV -> BGR.
 *   The record: mag_min = lo, mag_max = hi, nonzero = the pixels whose value was not 0 BEFORE that repaint, invalid = (nonzero == 0),
 *   the reference's "invalid frame" (:89).  atan2f is the device's: a hue within a few ulp of a whole number can differ by one step
 *   from another libm's.
 * MAV_HSV_DRAW -- Farneback.draw_hsv:  ang = atan2f(fy, fx) + (float)pi;  hue = trunc(ang * (float)(180 / pi / 2));
 *   value = trunc(min(mag * 4.f, 255.f));  saturation 255;  then HSV -> BGR.  No reduction; the records are zeroed.
 *
 * BGR -> HSV is OpenCV's integer path (hsv_shift = 12, hue range 180) AS REMEMBERED, pinned to no cv2 build:
 *   sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) in double, sdiv[0] = hdiv[0] = 0;  v = max(b, g, r),
 *   d = v - min(b, g, r);  s = (d * sdiv[v] + 2048) >> 12;  h = g - b if v == r, else b - r + 2 d if v == g, else r - g + 4 d;
 *   h = (h * hdiv[d] + 2048) >> 12 with an arithmetic shift, + 180 if negative.
 * MAV_COLOR_BGR2RADIAL is im_helpers.get_flow_radial (src/im_helpers.py:87-100) in one pass: BGR -> HSV, S = V = 255, HSV -> BGR.
 *
 * DRAW FLOW.  Grid points x = step / 2, step / 2 + step, ... < W and y likewise.  A point is drawn when
 *   sqrt(fx * fx + fy * fy) > threshold in float32 (a NaN threshold draws nothing).  Its end point is
 *   (trunc((double)x + (double)fx + 0.5), trunc((double)y + (double)fy + 0.5)), each sum clamped to [-2^30, 2^30] before the
 *   conversion (beyond that the picture is unspecified).  The line is cv2.polylines of the two points, thickness 1, LINE_8, shift 0,
 *   AS REMEMBERED from OpenCV 4.x drawing.cpp, pinned to no cv2 build:
 *   clipLine: outcodes c = (x < 0) + 2 (x > W - 1) + 4 (y < 0) + 8 (y > H - 1) of both ends; nothing is drawn if they intersect; an end
 *     with c & 12 moves to the row a = 0 or H - 1: x += (int64)((double)(a - y) * (x2 - x1) / (y2 - y1)) (toward zero), first end, then
 *     second (which sees the first's new place); the codes' x bits are taken again; nothing is drawn if they intersect; then the same
 *     on the columns a = 0 or W - 1 with x and y exchanged.
 *   LineIterator, 8-connected, left to right: the ends are exchanged if x2 < x1; major = max(|dx|, |dy|), minor the other;
 *     err = major - 2 minor; major + 1 pixels; after each pixel the major axis advances one, the minor axis advances one too if
 *     err < 0 was true, and err += 2 major in that case, err -= 2 minor in every case.
 *   Then cv2.circle((x, y), 1, colour, -1): (x - 1 .. x + 1, y), (x, y - 1), (x, y + 1), clipped to the image.
 *   Everything of a call is drawn in ONE colour, so pixels that several lines reach get equal bytes whichever writes last.
 *   What to re-check first against a cv2 build: clipped lines (the truncation toward zero of the two clip steps and their order),
 *   then the iterator's first step on a line whose minor distance is exactly half the major one, then the BGR -> HSV tables.
 *
 * NON-FINITE flows: the picture is unspecified, nothing faults, the next call is unaffected.
 *
 * FORMS.  mav_vis_form says which form of the pixel passes a call takes: MAV_VIS_FORM_FAST when every non-NULL pointer is aligned to 16
 *   bytes and the call has at least 16 pixels (groups of 16 pixels move as 16-byte words; the W * H * batch % 16 last pixels move as
 *   bytes), MAV_VIS_FORM_BYTES otherwise.  The bytes written do not depend on the form. */
#ifndef MAVFLOW_VIS_H
#define MAVFLOW_VIS_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_HSV_PROCESS 0            /* Farneback.process()'s picture */
#define MAV_HSV_DRAW    1            /* Farneback.draw_hsv's picture */
#define MAV_COLOR_BGR2HSV 40         /* cv2.COLOR_BGR2HSV */
#define MAV_COLOR_HSV2BGR 54         /* cv2.COLOR_HSV2BGR */
#define MAV_COLOR_BGR2RADIAL 1040    /* im_helpers.get_flow_radial */
#define MAV_VIS_FORM_BYTES 0
#define MAV_VIS_FORM_FAST  1

typedef struct {
    float mag_min, mag_max;          /* the image's extremes of |flow| */
    int32_t nonzero;                 /* pixels whose value was not 0 before the repaint */
    int32_t invalid;                 /* 1: nonzero == 0, the reference keeps its previous picture */
} mav_hsv_record;                    /* 16 bytes; every byte is written */

/* flow (batch, H, W, 2) float32; bgr, hsv (batch, H, W, 3) uint8, hsv may be NULL; records: `batch` of them; img (batch, H, W, 3) uint8,
 * drawn into; bgr_colour: three bytes, read by the call.
 * MAV_ERR_ARG, with the function's name in mav_last_error(): a NULL pointer (but hsv); a mode or code that is none of the above;
 *   batch < 1, or batch above the context's max_batch; W * H * batch above 2^31 - 1; step < 1;
 *   _dev forms: flow or records not aligned to 4. */
int mav_flow_hsv(mav_ctx*, const float* flow, int batch, int mode, uint8_t* bgr, uint8_t* hsv, mav_hsv_record* records);
int mav_flow_hsv_dev(mav_ctx*, const float* flow, int batch, int mode, uint8_t* bgr, uint8_t* hsv, mav_hsv_record* records);
int mav_cvt_color(mav_ctx*, const uint8_t* src, int code, int batch, uint8_t* dst);
int mav_cvt_color_dev(mav_ctx*, const uint8_t* src, int code, int batch, uint8_t* dst);
int mav_draw_flow(mav_ctx*, uint8_t* img, const float* flow, int batch, int step, float threshold, const uint8_t* bgr_colour);
int mav_draw_flow_dev(mav_ctx*, uint8_t* img, const float* flow, int batch, int step, float threshold, const uint8_t* bgr_colour);
/* The form a call of these sizes and pointers takes (a pure function of its arguments; NULL pointers constrain nothing); -1 for a size
 * below 1. */
int mav_vis_form(int W, int H, int batch, const void* flow, const void* bgr, const void* hsv);

#ifdef __cplusplus
}
#endif
#endif

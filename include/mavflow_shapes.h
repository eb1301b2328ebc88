/* libmavflow -- shapes on the device: cv2.line, cv2.rectangle and the filled cv2.circle as a TABLE of shapes drawn in table order
 * (Detector.draw, Detector.predict, FocusOfExpansion.draw, blob boxes), cv2.add of two uint8 images, and the np.vstack / np.hstack
 * mosaic of the reference's debug frame (src/processor.py:295-301).
 *
 * The rules of mavflow_vis.h hold: the entry points KEEP everything a context holds resident, run on the context's stream, write only
 * what the caller passes in and hold no device memory of the context's.  The `_dev` forms take device pointers, allocate nothing and only
 * enqueue; the host forms take staging blocks behind the last call's, run, synchronise and give the blocks back.  0 = OK, < 0 = MAV_ERR_*,
 * mav_last_error() has the message.  A refused call has enqueued and written nothing.  All images are the context's W x H.
 *
 * THE TABLE.  Record i is drawn into image `image` of the batch as cv2 would draw it in call number i: a pixel that several records
 *   reach carries the colour of the LAST of them.  colour[0 .. channels - 1] are the bytes written (colour[3] is not read).  Every
 *   record is a set of ROW SPANS -- closed x intervals of one image row -- given below as a closed form of the row, so rows are
 *   independent.  A span is clipped to 0 .. W - 1, rows outside 0 .. H - 1 are not drawn.
 *   A record is SKIPPED (nothing of it is drawn, nothing faults, the records around it are drawn) when: kind is none of MAV_SHAPE_*;
 *   image is outside 0 .. batch - 1; one of x0, y0, x1, y1 is outside -2^20 .. 2^20; thickness is outside 1 .. MAV_SHAPE_MAX_THICKNESS,
 *   except MAV_SHAPE_FILLED for a rectangle; a circle's thickness is not MAV_SHAPE_FILLED (outlined circles are not built) or its radius
 *   x1 is negative (a circle's y1 is range-checked like the rest and otherwise not read).  The host form refuses the call for the same
 *   records with MAV_ERR_ARG, naming the first of them.
 *
 * LINE, thickness 1: the thickness-1 line of mavflow_vis.h (its DRAW FLOW paragraph), byte for byte -- clipLine, then the 8-connected LineIterator, both as mavflow_vis.h
 *   states them.  By rows: with the ends exchanged if x2 < x1, major = max(|dx|, |dy|), minor the other, sy = sign of dy, pixel i
 *   (0 .. major) lies d(i) = floor((2 minor i + major - 1) / (2 major)) steps along the minor axis (d = 0 when major = 0).  |dy| > dx: row
 *   y1 + sy i holds the one pixel x1 + d(i).  Otherwise row y1 + sy d holds the pixels x1 + i for hi(d - 1) < i <= hi(d),
 *   hi(d) = floor((2 major d + major) / (2 minor)), i within 0 .. major (minor = 0: all of them in row y1).
 *
 * LINE, thickness t > 1: OpenCV 4.x ThickLine AS REMEMBERED, pinned to no cv2 build.  XY_ONE = 2^16; P0 = (x0, y0) * XY_ONE,
 *   P1 = (x1, y1) * XY_ONE as int64.
 *   Half-width:  dx = (double)(x0 - x1), dy = (double)(y1 - y0);  r = dx * dx + dy * dy;  only if r > DBL_EPSILON the quadrilateral
 *     exists:  s = ((double)(t << 15) + (double)((t & 1) << 15)) / sqrt(r);  dpx = rint(dy * s), dpy = rint(dx * s), rint rounding a half
 *     to even, each product, the quotient and the root rounded on its own (no FMA).  The odd term makes an odd thickness half a pixel
 *     wider on each side: t = 3 has the half-width 2.0, t = 2 has 1.0.
 *   Vertices, int64:  v0 = P0 + dp, v1 = P0 - dp, v2 = P1 - dp, v3 = P1 + dp, dp = (dpx, dpy).
 *   Fill (FillConvexPoly's span walk, 16.16):  row(v) = (v.y + XY_ONE / 2) >> 16;  m = the first vertex with the smallest v.y;
 *     ymin = row(v_m), ymax = the largest row.  Two chains leave m, u_k = v_(m + k) and u_k = v_(m - k), indices mod 4, k = 0 .. 3.
 *     A chain's edge accumulator at row y: start with (X, D, Y) = (-XY_ONE, 0, ymin), c = 0, ys = ymin; repeat: k = the smallest
 *     k > c, k <= 3, with row(u_k) > ys; none: stop; else ty = row(u_k), (X, D, Y) = (u_(k - 1).x, ((u_k.x - u_(k - 1).x) * 2 + (ty - ys))
 *     / (2 (ty - ys)), ys), the int64 quotient truncated toward zero; c = k; stop if y < ty; ys = ty.  The chain's x(y) = X + (y - Y) D.
 *     Row y, ymin <= y <= ymax, has the span  (min(xa, xb) + XY_ONE / 2) >> 16  ..  (max(xa, xb) + XY_ONE / 2) >> 16  of the two chains'
 *     x(y), arithmetic shifts.
 *     OpenCV's walk stops in front of row ymax and leaves that row to its outline pass (Line2 between the vertices).  This library draws
 *     NO outline pass; it draws row ymax from the accumulators as they stand, which is what the closed form above gives for y = ymax.
 *   Caps:  a filled circle of radius (t * 2^15 + 2^15) >> 16 around (x0, y0) and around (x1, y1).  A zero-length line (r <= DBL_EPSILON)
 *     is the two caps alone.
 * CIRCLE, filled, radius R: row cy +- k, k = 0 .. R, has the span cx - h[k] .. cx + h[k], h = the half-widths of OpenCV's integer
 *   midpoint walk: err = 0, dx = R, dy = 0, plus = 1, minus = 2 R - 1; while dx >= dy: h[dy] = max(h[dy], dx), h[dx] = max(h[dx], dy);
 *   dy += 1, err += plus, plus += 2; if err > 0: err -= minus, dx -= 1, minus -= 2.  (The disc of mav_overlay and draw_FoE; radius 10:
 *   10 9 9 9 9 8 8 7 6 4 0.  The walk keeps err = dx^2 + dy^2 - R^2, so h[k] = floor(sqrt(R^2 - k^2)) for every k, which is how it is evaluated.)
 * RECT, thickness t >= 1: the four lines of thickness t  (x0, y1) - (x0, y0),  (x0, y0) - (x1, y0),  (x1, y0) - (x1, y1),
 *   (x1, y1) - (x0, y1), OpenCV's PolyLine order (the record has one colour, so the order decides no byte; every corner carries a cap).
 *   RECT, MAV_SHAPE_FILLED: rows min(y0, y1) .. max(y0, y1), each the span min(x0, x1) .. max(x0, x1).
 *
 * What to re-check first against a cv2 build: (1) the odd-thickness half-width -- whether t = 3 is 5 pixels wide as stated here, or the
 *   odd term is absent in that build; (2) the row rounding of the polygon fill -- XY_ONE / 2 added to both span ends and to the vertex
 *   rows, and the truncating quotient of the edge slope; (3) the polygon's outline pass -- cv2 draws Line2 between the vertices, which
 *   can add pixels beside the spans and draws row ymax, where this library continues the spans instead; (4) thickness 2 being three
 *   pixels wide (half-width 1.0 plus the rounding); then the thickness-1 items mavflow_vis.h lists.
 *
 * FORMS.  ORDERED (MAV_SHAPES_FORM_ORDERED): pass A rasterises every (record, row) in parallel with an integer atomicMax of
 *   (table index + 1) into an int32 plane, one word per pixel of the batch, which the call clears itself (the caller's scratch may hold
 *   anything); pass B writes the colour of the recorded record where the plane is not 0.  The maximum does not depend on arrival order:
 *   the bytes are the same on every run.  DIRECT (MAV_SHAPES_FORM_DIRECT): one pass stores the colours; taken by the _dev form when
 *   scratch == NULL, the caller's promise that overlapping records share a colour (where they do not, those pixels are unspecified),
 *   and by the host form when every record of the table carries the same colour[0 .. channels - 1].  The bytes written do not depend
 *   on the form.  mav_add_saturate and mav_mosaic move 16-byte words (MAV_SHAPES_FORM_WORDS) when every pointer of the call is aligned
 *   to 16 and there are at least 16 bytes, the last n % 16 bytes as bytes; MAV_SHAPES_FORM_BYTES otherwise. */
#ifndef MAVFLOW_SHAPES_H
#define MAVFLOW_SHAPES_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_SHAPE_LINE   0           /* cv2.line(img, (x0, y0), (x1, y1), colour, thickness), LINE_8, shift 0 */
#define MAV_SHAPE_RECT   1           /* cv2.rectangle(img, (x0, y0), (x1, y1), colour, thickness) */
#define MAV_SHAPE_CIRCLE 2           /* cv2.circle(img, (x0, y0), x1, colour, -1) */
#define MAV_SHAPE_FILLED (-1)
#define MAV_SHAPE_MAX_THICKNESS 255
#define MAV_SHAPE_MAX_COORD (1 << 20)
#define MAV_SHAPES_FORM_ORDERED 0
#define MAV_SHAPES_FORM_DIRECT  1
#define MAV_SHAPES_FORM_BYTES   0
#define MAV_SHAPES_FORM_WORDS   1
#define MAV_MOSAIC_MAX_TILES 16

typedef struct {
    int32_t kind, image, x0, y0, x1, y1, thickness;
    uint8_t colour[4];
} mav_shape;                         /* 32 bytes */

/* img (batch, H, W, channels) uint8, drawn into; channels 1 or 3; shapes: n (n_max) records, host memory for mav_draw_shapes, device
 * memory aligned to 4 for the _dev form; n_dev: NULL (n_max records) or the device's own count -- a negative one, or one above n_max,
 * draws nothing; scratch: NULL (DIRECT) or mav_shapes_scratch_bytes(W, H, batch) bytes aligned to 4 (ORDERED).
 * MAV_ERR_ARG: a NULL context, img or (n > 0) table; channels not 1 or 3; batch < 1 or above the context's max_batch; n < 0;
 * W * H * batch above 2^31 - 1; a pointer not aligned as said; host form: a record the device form would skip.  n = 0 draws nothing. */
size_t mav_shapes_scratch_bytes(int W, int H, int batch);
int mav_draw_shapes(mav_ctx*, uint8_t* img, int channels, int batch, const mav_shape* shapes, int n);
int mav_draw_shapes_dev(mav_ctx*, uint8_t* img, int channels, int batch, const mav_shape* shapes, int n_max, const int32_t* n_dev, void* scratch);
/* The form mav_draw_shapes takes for this (host) table: a pure function; -1 for a NULL table with n > 0, n < 0 or channels not 1 or 3 */
int mav_shapes_form(const mav_shape* shapes, int n, int channels);

/* dst = min(a + b, 255) bytewise, cv2.add of two uint8 images (batch, H, W, channels), channels 1 .. 4; dst may be a or b */
int mav_add_saturate(mav_ctx*, const uint8_t* a, const uint8_t* b, int channels, int batch, uint8_t* dst);
int mav_add_saturate_dev(mav_ctx*, const uint8_t* a, const uint8_t* b, int channels, int batch, uint8_t* dst);
/* MAV_SHAPES_FORM_WORDS / _BYTES of a call of n bytes with these pointers (a pure function); -1 for n < 1 */
int mav_bytes_form(size_t n, const void* a, const void* b, const void* dst);

/* blobs (batch, max_blobs) and counts (batch) as mav_components_dev leaves them: the first min(max(n_blobs, 0), max_blobs) records of
 * every image, image after image, become RECT records (x, y) - (x + w - 1, y + h - 1) of that image with this thickness and colour
 * (four bytes on the host, read by the call) in out[0 .. *n_out - 1]; out holds batch * max_blobs records.  All pointers but colour in
 * device memory, aligned to their elements (blobs to 8); enqueue only.  thickness is checked as a rectangle's. */
int mav_shapes_from_blobs_dev(mav_ctx*, const mav_blob* blobs, const mav_cc_counts* counts, int batch, int max_blobs, int thickness,
                              const uint8_t* colour, mav_shape* out, int32_t* n_out);

/* out (batch, rows * H, cols * W, 3) = np.vstack of the rows' np.hstack of the tiles: tiles[r * cols + c] is (batch, H, W,
 * tile_channels[r * cols + c]) uint8, 1 channel (replicated: GRAY2RGB) or 3; a NULL tile is black.  tiles and tile_channels are host
 * arrays of rows * cols <= MAV_MOSAIC_MAX_TILES entries, read by the call; the tiles themselves are host memory for mav_mosaic and
 * device memory for the _dev form.  out overlaps no tile. */
int mav_mosaic(mav_ctx*, const uint8_t* const* tiles, const int* tile_channels, int rows, int cols, int batch, uint8_t* out);
int mav_mosaic_dev(mav_ctx*, const uint8_t* const* tiles, const int* tile_channels, int rows, int cols, int batch, uint8_t* out);

/* The debug frame's pictures where they are (src/processor.py:288-299), device outputs, (batch, H, W, 3) u8 BGR each, any may be NULL:
 * img_flow = im_helpers.get_flow_vis(flow) of the float32 fields `flow` (device, aligned to 4; read only for img_flow), as
 * mav_flow_to_color renders it; img_warped, img_global = what mav_last_global_motion_render renders from the flow and matrix the most
 * recent global-motion call on this context left resident, MAV_ERR_STATE under its rules.  field: batch * H * W * 2 floats of the
 * caller's, aligned to 4, never NULL: the call's only scratch (its head first holds the renderer's mode bytes, then the field of each
 * global-motion picture).  Enqueue only.  MAV_ERR_ARG: a NULL context or field, img_flow without flow, a misaligned pointer, the batch. */
int mav_motion_pictures_dev(mav_ctx*, const float* flow, int batch, float* field, uint8_t* img_flow, uint8_t* img_warped, uint8_t* img_global);

#ifdef __cplusplus
}
#endif
#endif

/* libmavflow -- the evaluation's other half: the ground-truth flow from depth and pose, and an estimated flow held against it.
 *
 * A header of its own beside mavflow.h (whose list of entry points is the resident-results table's subject): the four entry points
 * here KEEP everything a context holds resident -- every mav_last_* reader returns after them what it returned before.  They run on
 * the context's stream, take staging blocks behind the last call's and give them back, and write nothing but the caller's outputs
 * (and, for the histogram, the context's own copy of the two edge lists).
 *
 * Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message; `_dev` forms take device pointers and only
 * enqueue on the context's stream; the host forms stage, run and synchronise.  Whatever can be judged from the arguments alone is
 * judged before the context is looked at; a refused call has enqueued and written nothing.
 */
#ifndef MAVFLOW_TRUTH_H
#define MAVFLOW_TRUTH_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ground-truth flow: calculate_flow / write_flow of the reference's src/airsim_optical_flow.py --------------------------------
 * Every pixel of frame 2 is reprojected through its depth and the inverse of frame 2's view-projection matrix into the world, moved
 * back by the MAV's displacement where the segmentation says MAV, and projected with frame 1's matrix. */
typedef struct {
    double view_proj_prev[16];   /* row-major 4x4: get_view_proj_mat(state1), M[i][j] = m[4 i + j] */
    double view_proj_inv[16];    /* row-major 4x4: numpy.linalg.inv(get_view_proj_mat(state2)), inverted by the caller */
    double displacement[3];      /* drone_displacement x, y, z (already x delta_time x 100) */
    float  depth_scale;          /* multiplied onto the depth IN float32 (the reference's float32 `pfm.T * 100`); 1.0f = as given */
    int    flags;                /* 0 */
} mav_gt_flow_params;            /* one per pair of the batch */

/* depth (batch, H, W) float32 and seg (batch, H, W) uint8 (the MAV is seg > 0; NULL: no MAV anywhere), both in image layout;
 * params: `batch` blocks; flow (batch, H, W, 2) of out_depth:
 *   MAV_DEPTH_64F  the array write_flow hands to utils.write_flow, -result.swapaxes(0, 1), components (u, v)
 *   MAV_DEPTH_32F  that array rounded to float32: what the .flo file holds and get_gt_of returns
 * Per pixel (x, y), everything in float64, every line one IEEE operation order (no contraction, IEEE division and square root):
 *   nx = x / W;  ny = y / H                       (integer -> double, true division)
 *   sx = 2.0 * (nx - 0.5);  sy = 2.0 * ((1.0 - ny) - 0.5)
 *   row_i(M; a, b, c, d) = ((M[i][0]*a + M[i][1]*b) + M[i][2]*c) + M[i][3]*d
 *   s = Minv (sx, sy, 1.0, 1.0);  e = Minv (sx, sy, 0.5, 1.0)
 *   S_i = s_i / s_3;  E_i = e_i / e_3             (i = 0, 1, 2)
 *   d_i = E_i - S_i;  n = sqrt((d_0*d_0 + d_1*d_1) + d_2*d_2)
 *   z   = (double)(depth * depth_scale)           (the product in float32)
 *   P_i = S_i + (d_i / n) * z;   if seg > 0: P_i = P_i - displacement_i
 *   p = Mprev (P_0, P_1, P_2, 1.0);  rhw = 1.0 / p_3;  px = p_0 * rhw;  py = p_1 * rhw
 *   rx = (px * 0.5 + 0.5) * W - x;   ry = ((-py) * 0.5 + 0.5) * H - y
 *   (u, v) = (-rx, -ry)
 * Infinities are the reference's; a NaN is stored as the canonical quiet NaN (0x7FF8000000000000 / 0x7FC00000).
 * The inverse is the caller's on purpose: the bits of LAPACK's inverse are not this library's business.
 * mav_gt_flow: host pointers, params a host array whose flags are judged (non-zero: MAV_ERR_ARG).  mav_gt_flow_dev: device pointers,
 * params included (their flags cannot be judged and are not read); depth not aligned to 4, params not aligned to 8 or flow not aligned
 * to one (u, v) pair of out_depth (8 / 16 bytes) is MAV_ERR_ARG.
 * MAV_ERR_ARG also for NULL depth / params / flow, batch outside [1, max_batch], out_depth neither of the two. */
int mav_gt_flow(mav_ctx*, const float* depth, const uint8_t* seg, const mav_gt_flow_params* params, int batch, int out_depth, void* flow);
int mav_gt_flow_dev(mav_ctx*, const float* depth, const uint8_t* seg, const mav_gt_flow_params* params, int batch, int out_depth, void* flow);

/* ---- radial-error histogram: Processor.analyze_radial_error + plot_radial_error.py's histogram2d --------------------------------
 * flow, gt_flow (batch, H, W, 2) float32; sky (batch, H, W) uint8, non-zero = sky, or NULL (no sky).  Per non-sky pixel, in float32:
 *   mag = sqrtf(u*u + v*v)                                   (numpy.linalg.norm(axis=-1) on float32, bit for bit)
 *   err = (atan2f(v, u) - atan2f(gv, gu)) * (180.0f / pi_f)  (numpy.rad2deg on float32; the device's atan2f is not glibc's)
 * and the pixel is counted in cell (i, j) iff mag_edges[i] <= mag < mag_edges[i+1] and err_edges[j] <= err < err_edges[j+1], compared
 * in float64 against the edges as passed, the last bin of either list closed on the right: numpy.histogram2d's rule.  A value outside
 * its range, or NaN, puts the pixel in no cell.
 * Edge lists: HOST arrays in both forms (copied before the call returns), strictly increasing, finite, 2 .. MAV_RADIAL_MAX_EDGES
 * entries each, (n_mag_edges - 1) * (n_err_edges - 1) <= MAV_RADIAL_MAX_CELLS; anything else is MAV_ERR_ARG.
 * table: MAV_RADIAL_TABLE_WORDS(bins_mag, bins_err) int64 words: non_sky_pixels, in_range_pixels, then counts[i][j], i over magnitude.
 * The call ADDS into it (the caller zeroes it): a sequence's histogram builds up on the device and only the table ever comes back.
 * _dev: device pointers (table and the two fields aligned to 8: one float32 pair), enqueue only.  Host form: stages its inputs, adds into the host table. */
#define MAV_RADIAL_MAX_EDGES 257
#define MAV_RADIAL_MAX_CELLS 65536
#define MAV_RADIAL_TABLE_WORDS(bins_mag, bins_err) (2 + (bins_mag) * (bins_err))
int mav_radial_error_hist(mav_ctx*, const float* flow, const float* gt_flow, const uint8_t* sky, int batch, const double* mag_edges,
                          int n_mag_edges, const double* err_edges, int n_err_edges, int64_t* table);
int mav_radial_error_hist_dev(mav_ctx*, const float* flow, const float* gt_flow, const uint8_t* sky, int batch, const double* mag_edges,
                              int n_mag_edges, const double* err_edges, int n_err_edges, int64_t* table);

#ifdef __cplusplus
}
#endif
#endif

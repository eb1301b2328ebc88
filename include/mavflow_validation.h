/* libmavflow -- the validation tail of the reference's loop (src/processor.py:315-317, 343-347) on the device: the MAV's pixel count, the
 * raster-order list of its pixels, get_simple_bounding_box of the segmentation, Dataset.validate_sky_segment's four counts and the sum
 * of the derotated ground-truth flow over the MAV, for one frame or a batch, in one call.
 *
 * A header of its own beside mavflow.h (whose list of entry points is the resident-results table's subject), like mavflow_truth.h: the
 * entry points here KEEP everything a context holds resident -- every mav_last_* reader returns after them what it returned before.
 * They run on the context's stream, write nothing but the caller's outputs and a scratch block of the context's own (taken from the
 * context's memory owner by the first call, grown when a call needs more, counted by mav_mem_info, freed by mav_destroy); the host form
 * takes staging blocks behind the last call's and gives them back.
 *
 * Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message; the `_dev` form takes device pointers and only
 * enqueues on the context's stream; the host form stages, runs and synchronises.  Whatever can be judged from the arguments alone is
 * judged before the context is looked at; a refused call has enqueued and written nothing.
 */
#ifndef MAVFLOW_VALIDATION_H
#define MAVFLOW_VALIDATION_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_GT_STATS_FRAME0   1     /* params.flags: frame index 0, no derotation (detector.py:80-81) */
#define MAV_GT_STATS_THR_F64  2     /* params.flags: the depth threshold by numpy 1.x's value-based casting (below) */
#define MAV_GT_STATS_TRUNCATED 1u   /* record.flags: drone_pixels > max_pixels; the list holds the first max_pixels, flow_sum is zero */
#define MAV_GT_STATS_DEPTH_NAN 2u   /* record.flags: a depth is NaN: depth_max is NaN and no pixel is above the threshold */
#define MAV_GT_STATS_MAX_PIXELS (1 << 20)

typedef struct {
    double omega[3];        /* as mav_detect takes them: angular difference / dt */
    double dt;
    double box_fraction;    /* 0.1: get_simple_bounding_box's threshold = box_fraction * max(seg), compared in float64 */
    float  depth_fraction;  /* 0.8f */
    int    seg_threshold;   /* 127: the MAV is seg > seg_threshold */
    int    flags;           /* MAV_GT_STATS_FRAME0 | MAV_GT_STATS_THR_F64 */
    int    pad;             /* 0 */
} mav_gt_stats_params;      /* one per pair of the batch; 56 bytes */

typedef struct {
    int64_t  drone_pixels;  /* #{seg > seg_threshold} */
    int64_t  sky[4];        /* pos, neg, tp, fp of calculate_tpr_fpr((depth > thr) * 255, sky != 0); zeros when depth is NULL */
    double   flow_sum[2];   /* see below; zeros when gt_flow is NULL or the list is truncated */
    int32_t  box[4];        /* start_x, start_y, end_x, end_y of seg > box_fraction * max(seg); all -1 when no pixel passes */
    int32_t  seg_max;
    int32_t  listed;        /* min(drone_pixels, max_pixels) */
    float    depth_max;     /* np.max's: NaN (canonical quiet NaN 0x7FC00000) as soon as one depth is NaN; +0 ranks above -0; 0 when depth is NULL */
    uint32_t flags;         /* MAV_GT_STATS_TRUNCATED | MAV_GT_STATS_DEPTH_NAN */
    uint32_t pad[2];        /* 0 */
} mav_gt_stats_record;      /* 96 bytes, a multiple of 16; every byte is written */

/* Per image of the batch:
 *   MAV pixel        seg > seg_threshold
 *   box              get_simple_bounding_box (src/im_helpers.py:55-84): first / last column and row with a pixel whose
 *                    (double)seg > box_fraction * (double)max(seg)
 *   depth threshold  default:              thr = depth_fraction * max(depth), one float32 product -- numpy >= 2, where the Python
 *                                          float 0.80 takes the float32 of np.max's result
 *                    MAV_GT_STATS_THR_F64: thr = (float)(F * (double)max(depth)), numpy 1.x's value-based casting: the product in
 *                                          float64, the scalar rounded to the float32 of the array it is compared with.  F is the
 *                                          fraction AS GIVEN in decimal: the double nearest to the shortest decimal n / 10^d (d = 1 .. 9)
 *                                          that rounds to depth_fraction -- 0.8 for 0.8f; (double)depth_fraction if there is none
 *   sky counts       gt = depth > thr (float32 comparison; false for NaN on either side), s = sky != 0:
 *                    pos = #gt, neg = #!gt, tp = #(gt && s), fp = #(!gt && s): calculate_tpr_fpr's four sums (src/im_helpers.py:244-252)
 *                    of Dataset.validate_sky_segment (src/datasets/dataset.py:173-175)
 *   list             the linear indices y * W + x of the first `listed` MAV pixels in raster order -- the order of
 *                    flow[segmentation > 127] --, unused entries -1
 *   flow_sum[c]      the float64 sum over the listed pixels in raster order, accumulated SEQUENTIALLY from 0.0, of
 *                    (double)gt_flow[y][x][c] - derotation_c(x, y): Detector.derotate's operation order (src/detector.py:83-117), the
 *                    detection kernels' own derot_apply.  np.average(a, axis=0) of an (n, 2) float64 array is this row-by-row sum
 *                    divided by n, so flow_sum / drone_pixels is the reference's drone_flow_avg_gt to the bit.
 *                    With MAV_GT_STATS_FRAME0 the reference averages the float32 rows themselves: flow_sum is then the same sequential
 *                    sum taken IN float32 (stored as the double of that float32), and (float)flow_sum / (float)drone_pixels is
 *                    np.average's float32.
 * Only integer atomics are used: the same bytes come out on every run and at every batch position.
 *
 * seg, sky (batch, H, W) uint8; depth (batch, H, W) float32; gt_flow (batch, H, W, 2) float32; gt_flow, sky and depth may each be NULL
 * (a NULL sky: no sky anywhere); params, records: `batch` blocks; indices (batch, max_pixels) int32 or NULL.
 * MAV_ERR_ARG: NULL seg / params / records; batch outside [1, max_batch]; max_pixels outside [1, MAV_GT_STATS_MAX_PIXELS];
 *   host form: a non-finite omega or dt, dt == 0 without MAV_GT_STATS_FRAME0, unknown flag bits;
 *   _dev form (the parameter blocks are on the device and are not judged): depth not aligned to 4, gt_flow to 8, params to 8,
 *   records to 16, indices to 4. */
void mav_gt_stats_defaults(mav_gt_stats_params*);
int mav_gt_stats(mav_ctx*, const uint8_t* seg, const float* gt_flow, const uint8_t* sky, const float* depth, const mav_gt_stats_params* params,
                 int batch, int max_pixels, mav_gt_stats_record* records, int32_t* indices);
int mav_gt_stats_dev(mav_ctx*, const uint8_t* seg, const float* gt_flow, const uint8_t* sky, const float* depth, const mav_gt_stats_params* params,
                     int batch, int max_pixels, mav_gt_stats_record* records, int32_t* indices);

#ifdef __cplusplus
}
#endif
#endif

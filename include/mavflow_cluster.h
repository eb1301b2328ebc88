/* libmavflow -- k-means clustering on the device: the algorithm of cv2.kmeans with caller-supplied initial centres (the clustering step
 * of the reference's Detector.clustering, src/detector.py:396-428), for one sample set or a batch, and the arithmetic that method does
 * after the cv2 call (the centres as a grey-level table, the painted image, the >= 225 mask).
 *
 * A header of its own beside mavflow.h, like mavflow_truth.h and mavflow_validation.h: the entry points here KEEP everything a context
 * holds resident -- every mav_last_* reader returns after them what it returned before.  They run on the context's stream and hold no
 * device memory of the context's: the `_dev` form works in a caller's workspace (mav_kmeans_workspace_bytes), the host form takes staging
 * blocks behind the last call's and gives them back.
 *
 * Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message; the `_dev` form takes device pointers and only
 * enqueues on the context's stream; the host form stages, runs and synchronises.  A refused call has enqueued and written nothing.
 *
 * THE ALGORITHM.  N samples x_i of D components (1..4), float32 or uint8 (a uint8 component is its float32 value); K clusters (1..16);
 * A attempts (1..16), each from the caller's initial centres init[a][k][d] (the random draw is the caller's: cv2 draws from a private
 * generator no implementation can follow).  max_iter is clamped to [2, 100]; eps is compared squared when > 0, else 0.  N >= K.
 * Per attempt, with cv2.kmeans' loop structure (OpenCV 4.x modules/core/src/kmeans.cpp as remembered; not pinned to a cv2 build):
 *
 *   c = init[a]
 *   for it = 1 .. max_iter - 1:
 *       assign:  label_i = the FIRST k minimising dist(x_i, c_k);  dist = the float32 sum over d ascending of (x_d - c_kd)^2, from 0,
 *                every operation rounded on its own (no FMA)
 *       sums:    n_k = #{label = k},  S_kd = the float64 sum of (double)x_id over the cluster (order: below)
 *       repair, for every k with n_k = 0, in ascending k:
 *                donor = the FIRST cluster with the largest n;  m_d = (float)(S_donor,d / (double)n_donor)
 *                j = the donor's sample with the largest dist(x_j, m), the HIGHEST index among equals
 *                label_j = k;  n_donor -= 1, n_k += 1;  S_donor,d = S_donor,d - (double)x_jd;  S_kd = S_kd + (double)x_jd
 *       new_kd = (float)(S_kd / (double)n_k)
 *       shift  = max over k of the float64 sum over d ascending of t * t,  t = (double)(float)(new_kd - c_kd)
 *       c = new
 *       if it == max_iter - 1 or shift <= eps * eps: stop
 *   compactness = the float64 sum over i of (double)dist(x_i, c[label_i])
 *
 * The labels are the last assignment's (repairs included), the centres the means of those labels; the result is the attempt with the
 * FIRST strictly smallest compactness.  tests/kmeans_ref.py is this text in numpy.
 *
 * THE ORDER OF THE SUMS depends on N alone -- not on the grid, the batch position, the context or the run.  Samples are cut into chunks
 * of MAV_KMEANS_CHUNK = 4096 consecutive samples; within chunk c, lane t (0..255) holds samples c * 4096 + j * 256 + t, j = 0..15.
 *   lane sum   sequentially over j ascending from 0.0 (a sample outside the cluster or past N adds nothing)
 *   wave sum   lanes 64w .. 64w + 63: six butterfly steps, v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1
 *   chunk sum  ((wave 0 + wave 1) + wave 2) + wave 3
 *   total      sequentially over the chunks ascending from 0.0
 * S_kd and the compactness are both taken this way; n_k is an integer.  No floating-point atomic is used anywhere (the repair's argmax
 * is an integer maximum of (dist bits << 32 | index)): the same bytes come out on every run and at every batch position.  Where every
 * sample is a multiple of 2^-8 below 2^12 and N <= 2^20 (uint8 samples always), S is exact in any order.
 *
 * A NaN component fails every comparison: the host form refuses non-finite samples and centres; in the `_dev` form, which does not see
 * the values, such a sample keeps label 0 and poisons that cluster's sum.
 */
#ifndef MAVFLOW_CLUSTER_H
#define MAVFLOW_CLUSTER_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_KMEANS_F32 0            /* params.depth: float32 samples */
#define MAV_KMEANS_U8  1            /* params.depth: uint8 samples */
#define MAV_KMEANS_MAX_K 16
#define MAV_KMEANS_MAX_ATTEMPTS 16
#define MAV_KMEANS_MAX_DIMS 4
#define MAV_KMEANS_MAX_N (1 << 30)
#define MAV_KMEANS_CHUNK 4096       /* samples per chunk of the summation order (above) */

typedef struct {
    int    K;           /* 8: clusters, 1..16 */
    int    attempts;    /* 10: 1..16 */
    int    max_iter;    /* 10: >= 1, clamped to [2, 100]; an attempt runs at most max_iter - 1 assignments */
    int    dims;        /* 3: components per sample, 1..4 */
    int    depth;       /* MAV_KMEANS_F32 | MAV_KMEANS_U8 */
    int    flags;       /* 0: no flag is defined */
    double eps;         /* 1.0: an attempt stops when no centre moved further than eps (compared squared); <= 0: only when none moved */
} mav_kmeans_params;    /* 32 bytes; on the host in both call forms */

typedef struct {
    double  compactness;    /* the best attempt's */
    double  shift;          /* of the best attempt's last update */
    int32_t best_attempt;
    int32_t iterations;     /* assignments the best attempt ran */
    int32_t repairs;        /* samples moved into empty clusters, total over the attempts */
    int32_t skipped;        /* launches of the call's sequence that left at once for this image (all its attempts done / no cluster empty) */
    int32_t counts[16];     /* n_k of the best attempt; 0 for k >= K */
} mav_kmeans_record;        /* 96 bytes, a multiple of 16; every byte is written */

/* samples (batch, n, dims) float32 or uint8; init (batch, attempts, K, dims) float32; labels (batch, n) int32; centers (batch, K, dims)
 * float32; records: `batch` blocks.  n is not tied to the frame size.
 * MAV_ERR_ARG: a NULL pointer; K, attempts, dims or depth out of range; max_iter < 1; flags != 0; a non-finite eps; n < K or
 *   n > MAV_KMEANS_MAX_N; batch outside [1, max_batch];
 *   host form: batch * n * dims > max_batch * W * H * 4; a non-finite sample or centre;
 *   _dev form: samples not aligned to the element size, init / centers / labels to 4, records to 16, workspace to 16; workspace_bytes less
 *   than mav_kmeans_workspace_bytes(n, batch, params).
 * The _dev form's launch sequence is a function of (attempts, K, max_iter, batch, n) alone: max_iter - 1 rounds of assignment, sums,
 * K - 1 guarded repair rounds and update, then compactness, choice and copy.  Which attempts are done, which clusters are empty, the
 * donor and the best attempt live in the workspace; a launch with nothing to do for its image leaves at once.  All attempts of an image
 * advance in the same launches. */
void   mav_kmeans_defaults(mav_kmeans_params*);
size_t mav_kmeans_workspace_bytes(int n, int batch, const mav_kmeans_params* params);      /* 0 for parameters a call would refuse */
int mav_kmeans(mav_ctx*, const void* samples, int n, int batch, const mav_kmeans_params* params, const float* init, int32_t* labels, float* centers,
               mav_kmeans_record* records);
int mav_kmeans_dev(mav_ctx*, const void* samples, int n, int batch, const mav_kmeans_params* params, const float* init, int32_t* labels,
                   float* centers, mav_kmeans_record* records, void* workspace, size_t workspace_bytes);

/* Detector.clustering after the cv2 call (src/detector.py:414-427), per image of the batch, all on the device:
 *   max = the largest of the K * dims centre values, 1.0 when it is 0
 *   lut[k][d] = (uint8)(center[k][d] * 255 / max): the float32 product, the float32 quotient, truncated toward zero as np.uint8() does
 *               (a negative or > 255 quotient wraps modulo 256, which is what numpy does on x86; not pinned)
 *   res[i][d]  = lut[label_i][d]            (batch, n, dims) uint8
 *   mask[i]    = res[i][0] >= 225           (batch, n) uint8, 0 or 1; may be NULL
 * labels (batch, n) int32 in [0, K) (the _dev form reads label & 15), centers (batch, K, dims) float32.
 * MAV_ERR_ARG: a NULL labels / centers / res; K, dims, n, batch out of range as above; host form: the size bound above;
 *   _dev form: labels or centers not aligned to 4. */
int mav_kmeans_paint(mav_ctx*, const int32_t* labels, const float* centers, int n, int batch, int K, int dims, uint8_t* res, uint8_t* mask);
int mav_kmeans_paint_dev(mav_ctx*, const int32_t* labels, const float* centers, int n, int batch, int K, int dims, uint8_t* res, uint8_t* mask);

#ifdef __cplusplus
}
#endif
#endif

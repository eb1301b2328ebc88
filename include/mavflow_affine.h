/* libmavflow -- a robust 2-D affine fit on the device: the algorithm of cv2.estimateAffine2D(from, to, method=RANSAC,
 * ransacReprojThreshold=3, maxIters=2000, confidence=0.99, refineIters=10) (reference src/detector.py:141-143) with the CALLER's sample
 * triples, for one pair set or a batch, and the same from the pairs of a float32 flow field (detector.py:126-128).
 *
 * A header of its own beside mavflow.h, like mavflow_cluster.h and mavflow_warp.h: the entry points here KEEP everything a context holds
 * resident -- every mav_last_* reader returns after them what it returned before.  They run on the context's stream and hold no device
 * memory of the context's: the `_dev` forms take device pointers and a caller's workspace and only enqueue, the host forms take staging
 * blocks behind the last call's, run, synchronise and give the blocks back.  Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*,
 * mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * What follows is OpenCV 4.x modules/calib3d/src/ptsetreg.cpp AS REMEMBERED and is NOT pinned against a cv2 build (none is available to
 * this project).  OpenCV draws its samples from a private generator, so no implementation can equal its draw: the triples are an
 * argument (mavflow.affine.sample_triples draws them from the caller's rng) and everything after the draw is deterministic.  What to
 * re-check first against a cv2 build: (1) OpenCV evaluates models and errors in float32 Point2f, here everything is float64; (2) its
 * subset check (here: the 0.996 cosine test at the third point alone, squared); (3) its refinement, Levenberg-Marquardt on the inliers,
 * where this takes the exact minimiser LM iterates towards; (4) its getSubset retry loop, which redraws a degenerate sample where this
 * counts the hypothesis as invalid.  tests/affine_ref.py is this text in numpy; the device equals it byte for byte.
 *
 * Everything is float64, every operation rounded on its own (no FMA contraction), expressions grouped as written, left to right.
 *
 * INPUTS.  src, dst: (batch, n, 2) float64 (x, y) -> (X, Y), 3 <= n <= MAV_AFFINE_MAX_PAIRS.  triples: (batch, max_iters, 3) int32,
 *   1 <= max_iters <= MAV_AFFINE_MAX_ITERS.  threshold >= 0, 0 < confidence < 1, refine 0 or not.  t2 = threshold * threshold.
 *
 * HYPOTHESIS `it` of an item, with (i0, i1, i2) = triples[it], a = src[i0], b = src[i1], c = src[i2], A = dst[i0], B = dst[i1], C = dst[i2],
 *   is VALID when all of these hold, tested in this order:
 *   1. 0 <= i0, i1, i2 < n and i0 != i1, i0 != i2, i1 != i2  (nothing is read through an index that fails this);
 *   2. in src and in dst, the angle at the third point is not flat: d1 = p[i1] - p[i2], d2 = p[i0] - p[i2], l1 = d1x*d1x + d1y*d1y,
 *      l2 = d2x*d2x + d2y*d2y, dot = d1x*d2x + d1y*d2y; rejected when l1 == 0 or l2 == 0 or dot*dot > (0.996*0.996) * (l1*l2)
 *      (OpenCV's cosine test without the square root; a NaN comparison rejects nothing here);
 *   3. THE MODEL: differences from the first point, two Cramer quotients per row, translation last:
 *        dx1 = bx - ax;  dy1 = by - ay;  dx2 = cx - ax;  dy2 = cy - ay;      det = dx1*dy2 - dx2*dy1;       det != 0 (else invalid)
 *        dX1 = Bx - Ax;  dX2 = Cx - Ax;  dY1 = By - Ay;  dY2 = Cy - Ay
 *        m00 = (dX1*dy2 - dX2*dy1) / det;   m01 = (dx1*dX2 - dx2*dX1) / det;   m02 = (Ax - m00*ax) - m01*ay
 *        m10 = (dY1*dy2 - dY2*dy1) / det;   m11 = (dx1*dY2 - dx2*dY1) / det;   m12 = (Ay - m10*ax) - m11*ay
 *      and all six entries are finite.
 * SCORE.  err(m, k) = e0*e0 + e1*e1 with e0 = ((m00*x + m01*y) + m02) - X, e1 = ((m10*x + m11*y) + m12) - Y for pair k.
 *   count[it] = the number of pairs k with err(m, k) <= t2: an integer; a NaN error is no inlier; an invalid hypothesis has count 0.
 * CHOICE, the sequential loop's semantics: niters = max_iters, best = -1, best_count = 2; for it = 0, 1, ... while it < niters: when
 *   hypothesis `it` is valid and count[it] > best_count, then best = it, best_count = count[it], niters = min(niters, need[count[it]]).
 *   The first of equal counts wins.  need[g], g = 0 .. n, is OpenCV's RANSACUpdateNumIters(confidence, (n - g) / n, 3, max_iters):
 *        g < 3: max_iters (never consulted: best_count starts at 2);   w = (double)g / (double)n;  den = 1 - (w*w)*w;
 *        den < DBL_MIN: 0 (so need[n] = 0);   ln = log(1 - confidence), ld = log(den);
 *        ld >= 0 or -ln >= max_iters * (-ld): max_iters;   else the quotient ln / ld rounded half to even.
 *   THE HOST BUILDS need[] and the device only looks it up: no log runs on the device, so a one-ulp difference between two logs can
 *   never change which hypothesis wins.  The table is the head of the workspace; THE LIBRARY FILLS IT (the caller passes none): each call
 *   computes the n + 1 entries on the host and brings them over with one asynchronous copy on the context's stream, from a block of its
 *   own that it keeps until the copy has taken the bytes.  tests hold the quotients of the tested (n, confidence) to lie more than 1e-6
 *   from a rounding tie, so the table does not depend on the log in use.
 *   best == -1: ok = 0, M is all zero, the mask is all zero.
 * INLIER MASK.  inliers[k] = 1 where err(best model, k) <= t2, else 0: the best MINIMAL model's, as cv2 returns it.  It is not
 *   recomputed after the refinement.
 * REFINEMENT (refine != 0 and ok): the exact least-squares affine map over the inliers -- the minimiser OpenCV's LM iterates towards,
 *   the residual being linear in the six unknowns.  Every sum below runs over k = 0 .. n - 1 in plain index order with one accumulator
 *   starting at +0.0; the term of a pair that is no inlier is +0.0 (which changes no bit of a sum).  g = the inlier count as a double.
 *        mx = (sum x) / g;  my = (sum y) / g;  mX = (sum X) / g;  mY = (sum Y) / g
 *        u = x - mx;  v = y - my;  P = X - mX;  Q = Y - mY
 *        Suu = sum u*u;  Suv = sum u*v;  Svv = sum v*v;  SuP = sum u*P;  SvP = sum v*P;  SuQ = sum u*Q;  SvQ = sum v*Q
 *        D = Suu*Svv - Suv*Suv;   T = Suu + Svv
 *        r00 = (SuP*Svv - SvP*Suv) / D;   r01 = (Suu*SvP - Suv*SuP) / D;   r02 = (mX - r00*mx) - r01*my
 *        r10 = (SuQ*Svv - SvQ*Suv) / D;   r11 = (Suu*SvQ - Suv*SuQ) / D;   r12 = (mY - r10*mx) - r11*my
 *   RANK TEST: the refined matrix is returned (record.refined = 1) when D > MAV_AFFINE_RANK_RATIO * (T*T) and its six entries are
 *   finite; otherwise the inliers do not determine a map (they lie on a line as far as float64 can tell: the smaller eigenvalue of the
 *   second-moment matrix is below 1e-12 of the larger) and the minimal model is returned with record.refined = 0.
 * RECORD.  sq_error = sum over the inliers (the mask's), in index order as above, of err(returned M, k). */
#ifndef MAVFLOW_AFFINE_H
#define MAVFLOW_AFFINE_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_AFFINE_MAX_PAIRS 65536      /* as MAV_HOMOGRAPHY_MAX_PAIRS */
#define MAV_AFFINE_MAX_ITERS 4096
#define MAV_AFFINE_RANK_RATIO 1e-12

typedef struct {
    double  threshold;      /* 3.0: ransacReprojThreshold, in pixels; finite, >= 0 */
    double  confidence;     /* 0.99; inside (0, 1) */
    int32_t max_iters;      /* 2000; 1 .. MAV_AFFINE_MAX_ITERS: the hypotheses per item in `triples` */
    int32_t refine;         /* 1: least-squares refinement on the inliers (cv2's refineIters != 0) */
    int32_t flags;          /* 0: no flag is defined */
    int32_t pad;            /* ignored */
} mav_affine_params;        /* 32 bytes */

typedef struct {
    int32_t ok;             /* 1: a model was found; 0: M and the mask are zero */
    int32_t inliers;        /* count[best], the number of ones in the mask */
    int32_t best_iter;      /* the winning hypothesis, or -1 */
    int32_t iters_run;      /* the final niters */
    int32_t valid;          /* valid hypotheses among the iters_run that ran */
    int32_t refined;        /* 1: M is the least-squares map over the inliers; 0: the minimal model (refine == 0, or the rank test) */
    double  sq_error;       /* the inliers' summed squared error under the returned M */
} mav_affine_record;        /* 32 bytes; every byte is written */

void mav_affine_defaults(mav_affine_params* p);
/* Bytes of workspace the _dev forms need for these shapes (the flow form's pair buffers included); 0 when the arguments would be refused. */
size_t mav_estimate_affine_workspace_bytes(int n, int batch, const mav_affine_params* params);

/* M (batch, 2, 3) float64, row-major: the layout mav_global_motion(_dev) and mav_warp_affine(_dev) read; inliers (batch, n) uint8;
 * records: `batch` blocks.
 * MAV_ERR_ARG, before anything is enqueued, the function's name in the message, the outputs untouched: a NULL pointer; n outside
 *   [3, MAV_AFFINE_MAX_PAIRS]; max_iters outside [1, MAV_AFFINE_MAX_ITERS]; batch outside [1, max_batch]; a threshold that is negative
 *   or not finite; a confidence outside (0, 1); flags != 0;
 *   host forms: a triple with an index outside [0, n) or a repeated index;
 *   _dev forms (where such a triple is an invalid hypothesis, and nothing is read out of bounds whatever the triples hold): src, dst,
 *   M not aligned to 8, triples to 4, records and workspace to 16; a workspace smaller than mav_estimate_affine_workspace_bytes. */
int mav_estimate_affine(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_affine_params* params, const int32_t* triples,
                        double* M, uint8_t* inliers, mav_affine_record* records);
int mav_estimate_affine_dev(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_affine_params* params, const int32_t* triples,
                            double* M, uint8_t* inliers, mav_affine_record* records, void* workspace, size_t workspace_bytes);
/* The pairs coords[k] -> coords[k] + flow[y][x] of float32 fields (batch, H, W, 2) at n host (x, y) int32 coords, every one inside the
 * frame (as mav_flow_homography(_dev): range-checked on the host, copied with the call), then the fit.  The _dev form gathers the pairs
 * into its workspace; flow aligned to 8.  pairs_dst (host form, may be NULL): the (batch, n, 2) float64 destination points. */
int mav_flow_affine(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_affine_params* params, const int32_t* triples,
                    double* M, uint8_t* inliers, mav_affine_record* records, double* pairs_dst);
int mav_flow_affine_dev(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_affine_params* params, const int32_t* triples,
                        double* M, uint8_t* inliers, mav_affine_record* records, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif

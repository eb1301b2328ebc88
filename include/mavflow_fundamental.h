/* libmavflow -- a robust fundamental-matrix fit on the device: the algorithm of cv2.findFundamentalMat(points1, points2, FM_RANSAC,
 * ransacReprojThreshold=3, confidence=0.99, maxIters=1000) (reference src/detector.py:135-139) with the CALLER's sample subsets, for one
 * pair set or a batch, the same from the pairs of a float32 flow field, and the DENSE EPIPOLAR RESIDUAL: for every pixel p of a flow
 * field, the distance in pixels of p + flow(p) from the epipolar line of p (and of p from the line of p + flow(p); the larger of the two).
 *
 * A header of its own beside mavflow.h, like mavflow_affine.h: the entry points here KEEP everything a context holds resident -- every
 * mav_last_* reader returns after them what it returned before.  They run on the context's stream and hold no device memory of the
 * context's: the `_dev` forms take device pointers (and a caller's workspace) and only enqueue, the host forms take staging blocks behind
 * the last call's, run, synchronise and give the blocks back.  Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*, mav_last_error()
 * has the message.  A refused call has enqueued and written nothing.
 *
 * What follows is OpenCV 4.x modules/calib3d/src/fundam.cpp / ptsetreg.cpp AS REMEMBERED, PINNED TO NO cv2 BUILD (none is available to
 * this project).  OpenCV draws its samples from a private generator, so no implementation can equal its draw: the subsets are an argument
 * (mavflow.fundamental.sample_subsets draws them from the caller's rng) and everything after the draw is deterministic.  What to re-check
 * first against a cv2 build: (1) OpenCV's float32 point arithmetic in the error, here everything is float64; (2) its SVD null space of
 * the 7 x 9 system, where this uses elimination with full pivoting; (3) its closed-form solveCubic, where this brackets and bisects;
 * (4) its scaling of every model to F[2][2] = 1, where this returns unit Frobenius norm (mavflow.fundamental.findFundamentalMat applies
 * cv2's scaling); (5) its direct 7-point path at n == 7, where this runs the same RANSAC loop; (6) its getSubset retry loop, which
 * redraws a degenerate sample where this counts the hypothesis as invalid.  tests/fundamental_ref.py is this text in numpy; the device
 * equals it byte for byte.
 *
 * Everything is float64, every operation rounded on its own (no FMA contraction), expressions grouped as written, left to right.  No
 * transcendental function lies on a path that decides a winner or a returned bit; square root and division are correctly rounded.
 * finite(v) means v - v == 0.
 *
 * INPUTS.  src, dst: (batch, n, 2) float64 (x, y) -> (X, Y), 7 <= n <= MAV_FUNDAMENTAL_MAX_PAIRS.  subsets: (batch, max_iters, 7) int32,
 *   1 <= max_iters <= MAV_FUNDAMENTAL_MAX_ITERS.  threshold >= 0, 0 < confidence < 1.  t2 = threshold * threshold.
 *
 * det3(m), the one 3 x 3 determinant of this text, m row-major:
 *        det3(m) = (m0*(m4*m8 - m5*m7) - m1*(m3*m8 - m5*m6)) + m2*(m3*m7 - m4*m6)
 * horner(l) = ((c3*l + c2)*l + c1)*l + c0.
 *
 * HYPOTHESIS `it` of an item, with (i0 .. i6) = subsets[it]:
 *   1. VALID INDICES: 0 <= ij < n for all seven and pairwise distinct; otherwise the hypothesis is invalid and nothing is read through it.
 *   2. THE SYSTEM, 7 x 9, row r from pair ir, in pixel coordinates, no normalisation:   (X*x, X*y, X, Y*x, Y*y, Y, x, y, 1).
 *   3. GAUSS-JORDAN WITH FULL PIVOTING, a column permutation perm[0..8] starting as the identity.  Step k = 0 .. 6:
 *        pv = 0, (pr, pc) = (k, k); for r = k .. 6, for c = k .. 8, in this (row-major) order: v = |A[r][c]|; v > pv: pv = v, (pr, pc) = (r, c)
 *          (strict, so the first of equals wins and a NaN never wins);
 *        the hypothesis is INVALID unless pv > 0 and finite(pv);
 *        rows k and pr change places, columns k and pc change places (all seven rows; perm[k] and perm[pc] too);
 *        p = A[k][k];  A[k][c] = A[k][c] / p for c = k + 1 .. 8;
 *        for every row r != k, r = 0 .. 6:  m = A[r][k];  A[r][c] = A[r][c] - m * A[k][c] for c = k + 1 .. 8.
 *      (Columns 0 .. 6 are not read again: they stand for the identity.)
 *   4. NULL VECTORS, un-permuted, all entries +0.0 first:   f1[perm[i]] = -A[i][7], f2[perm[i]] = -A[i][8] for i = 0 .. 6;
 *        f1[perm[7]] = 1;  f2[perm[8]] = 1.
 *   5. THE CUBIC det(l*f1 + f2) = c3 l^3 + c2 l^2 + c1 l + c0:   c3 = det3(f1);  c0 = det3(f2);
 *        c2 = (det3(f1 with row 0 from f2) + det3(f1 with row 1 from f2)) + det3(f1 with row 2 from f2);
 *        c1 = (det3(f2 with row 0 from f1) + det3(f2 with row 1 from f1)) + det3(f2 with row 2 from f1).
 *      NO MODEL (zero slots) when c3 == 0 or a coefficient is not finite (the solution at infinity is not returned, as in OpenCV), or
 *      when R below is not finite.
 *   6. REAL ROOTS in ascending order, at most three.  R = 1 + max(|c2 / c3|, |c1 / c3|, |c0 / c3|) (max: a > b ? a : b, from the left).
 *        disc = c2*c2 - (3*c3)*c1.  disc > 0: q = sqrt(disc), u = (-c2 - q) / (3*c3), v = (-c2 + q) / (3*c3), ta = the smaller, tb = the
 *        larger (u < v ? u : v), each clamped into [-R, R]; the points are e = (-R, ta, tb, R).  Otherwise e = (-R, R).
 *        With v[j] = horner(e[j]):  for j = 0, 1, ...: when v[j] == 0, e[j] is a root; when there is a next point and v[j], v[j + 1] have
 *        strictly opposite signs (one < 0, the other > 0), the interval holds one root by BISECTION: lo = e[j], hi = e[j + 1], at most 128
 *        steps of: mid = 0.5*(lo + hi); stop when mid == lo or mid == hi; fm = horner(mid); fm == 0: lo = mid, stop;
 *        (fm < 0) == (v[j] < 0): lo = mid, else hi = mid.  The root is lo.  A fourth root is not taken.  A double root without a sign
 *        change is not returned.
 *   7. MODEL SLOTS: root number s (s = 0, 1, 2) gives slot s:  F[j] = l*f1[j] + f2[j], j = 0 .. 8;  q = sum F[j]*F[j] in index order, one
 *        accumulator starting at +0.0;  nrm = sqrt(q);  the slot is INVALID unless nrm > 0 and finite(nrm);  F[j] = F[j] / nrm;  the
 *        entry of largest magnitude (strict >, the first of equals) is made positive: when it is < 0, F[j] = -F[j] for all j.
 *        Slots without a root are invalid.
 * SCORE.  For a pair (x, y) -> (X, Y) and row-major f[0..8]:
 *        a  = (f0*x + f1*y) + f2;   b  = (f3*x + f4*y) + f5;   c  = (f6*x + f7*y) + f8;   d2 = (X*a + Y*b) + c;    s2 = 1 / (a*a + b*b)
 *        a' = (f0*X + f3*Y) + f6;   b' = (f1*X + f4*Y) + f7;   c' = (f2*X + f5*Y) + f8;   d1 = (x*a' + y*b') + c';  s1 = 1 / (a'*a' + b'*b')
 *        e1 = (d1*d1)*s1;  e2 = (d2*d2)*s2;  err = (e1 > e2 or e1 is a NaN) ? e1 : e2      (a NaN on either side gives a NaN)
 *   OpenCV's symmetric squared distance to the epipolar lines.  count[it][slot] = the number of pairs with err <= t2: an integer; a NaN
 *   error is no inlier; an invalid slot has count -1.
 * CHOICE, the sequential loop's semantics: niters = max_iters, best = none, best_count = 6; for it = 0, 1, ... while it < niters: for
 *   slot = 0, 1, 2: when the slot is valid and count[it][slot] > best_count, then best = (it, slot), best_count = that count, niters =
 *   min(niters, need[best_count]).  All three slots of an iteration that began are visited; the first of equal counts wins.
 *   need[g], g = 0 .. n, is OpenCV's RANSACUpdateNumIters(confidence, (n - g) / n, 7, max_iters):
 *        g < 7: max_iters (never consulted);   w = (double)g / (double)n;  w2 = w*w;  w4 = w2*w2;  den = 1 - (w4*w2)*w;
 *        den < DBL_MIN: 0 (so need[n] = 0);   ln = log(1 - confidence), ld = log(den);
 *        ld >= 0 or -ln >= max_iters * (-ld): max_iters;   else the quotient ln / ld rounded half to even.
 *   THE HOST BUILDS need[] and the device only looks it up, exactly as in mavflow_affine.h: the table is the head of the workspace, the
 *   library fills it with one asynchronous copy on the context's stream from a block of its own.
 *   iters_run = the number of iterations that began: max_iters without a winner, else max(final niters, best_iter + 1).
 *   No winner: ok = 0, F all zero, the mask all zero.
 * OUTPUTS.  F (batch, 3, 3) float64: the best MINIMAL model, of unit Frobenius norm; no refinement (cv2 has none for this estimator).
 *   inliers[k] = 1 where err(F, k) <= t2, else 0.   sq_error = the sum over k = 0 .. n - 1 in index order, one accumulator starting at
 *   +0.0, of err(F, k) where pair k is an inlier and +0.0 where it is none.
 *
 * THE DENSE PASS.  Per pixel of image b: (x, y) = its column and row as doubles; (X, Y) = (x + (double)u, y + (double)v) with (u, v) the
 *   float32 flow; err as above under F[b];  finite(err): residual = (float)sqrt(err), mask = err > threshold*threshold ? 255 : 0;
 *   otherwise residual = 0, mask = 0 and the pixel is counted in not_finite.  An all-zero F (what a failed fit leaves) makes every err
 *   a NaN: the map and the mask are zero.  Integer atomics only: the bytes do not depend on the order of execution. */
#ifndef MAVFLOW_FUNDAMENTAL_H
#define MAVFLOW_FUNDAMENTAL_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_FUNDAMENTAL_MAX_PAIRS 65536     /* as MAV_AFFINE_MAX_PAIRS */
#define MAV_FUNDAMENTAL_MAX_ITERS 4096

typedef struct {
    double  threshold;      /* 3.0: ransacReprojThreshold, in pixels; finite, >= 0 */
    double  confidence;     /* 0.99; inside (0, 1) */
    int32_t max_iters;      /* 1000; 1 .. MAV_FUNDAMENTAL_MAX_ITERS: the hypotheses per item in `subsets` */
    int32_t flags;          /* 0: no flag is defined */
    int32_t pad[2];         /* ignored */
} mav_fundamental_params;   /* 32 bytes */

typedef struct {
    int32_t ok;             /* 1: a model was found; 0: F and the mask are zero */
    int32_t inliers;        /* the winner's count, the number of ones in the mask */
    int32_t best_iter;      /* the winning hypothesis, or -1 */
    int32_t best_slot;      /* its slot (the root's rank, 0 .. 2), or -1 */
    int32_t iters_run;      /* the iterations that began */
    int32_t valid;          /* valid slots among the iterations that began */
    double  sq_error;       /* the inliers' summed err under F */
} mav_fundamental_record;   /* 32 bytes; every byte is written */

typedef struct {
    float   max_residual;   /* the largest residual over the pixels whose err is finite; 0 where there is none */
    int32_t max_row;        /* its first position in raster order; -1 where no pixel is finite */
    int32_t max_col;
    int32_t movers;         /* pixels with err > threshold^2 (the mask's 255s, whether or not a mask is written) */
    int32_t not_finite;     /* pixels whose err is not finite */
    int32_t pad[3];         /* written as 0 */
} mav_epipolar_record;      /* 32 bytes; every byte is written */

void mav_fundamental_defaults(mav_fundamental_params* p);
/* Bytes of workspace the _dev forms need for these shapes (the flow form's pair buffers included); 0 when the arguments would be refused. */
size_t mav_find_fundamental_workspace_bytes(int n, int batch, const mav_fundamental_params* params);

/* F (batch, 3, 3) float64, row-major: the layout mav_epipolar_residual(_dev) reads; inliers (batch, n) uint8; records: `batch` blocks.
 * MAV_ERR_ARG, before anything is enqueued, the function's name in the message, the outputs untouched: a NULL pointer; n outside
 *   [7, MAV_FUNDAMENTAL_MAX_PAIRS]; max_iters outside [1, MAV_FUNDAMENTAL_MAX_ITERS]; batch outside [1, max_batch]; a threshold that is
 *   negative or not finite; a confidence outside (0, 1); flags != 0;
 *   host forms: a subset with an index outside [0, n) or a repeated index;
 *   _dev forms (where such a subset is an invalid hypothesis, and nothing is read out of bounds whatever the subsets hold): src, dst,
 *   F not aligned to 8, subsets to 4, records and workspace to 16; a workspace smaller than mav_find_fundamental_workspace_bytes. */
int mav_find_fundamental(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_fundamental_params* params,
                         const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records);
int mav_find_fundamental_dev(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_fundamental_params* params,
                             const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, void* workspace,
                             size_t workspace_bytes);
/* The pairs coords[k] -> coords[k] + flow[y][x] of float32 fields (batch, H, W, 2) at n host (x, y) int32 coords, every one inside the
 * frame (as mav_flow_affine(_dev): range-checked on the host, copied with the call), then the fit.  The _dev form gathers the pairs
 * into its workspace; flow aligned to 8.  pairs_dst (host form, may be NULL): the (batch, n, 2) float64 destination points. */
int mav_flow_fundamental(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_fundamental_params* params,
                         const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, double* pairs_dst);
int mav_flow_fundamental_dev(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_fundamental_params* params,
                             const int32_t* subsets, double* F, uint8_t* inliers, mav_fundamental_record* records, void* workspace,
                             size_t workspace_bytes);

/* The dense epipolar residual of flow (batch, H, W, 2) float32 under F (batch, 3, 3) float64 (any values; not looked at on the host):
 * residual (batch, H, W) float32 or NULL, mask (batch, H, W) uint8 0/255 or NULL (the layout mav_components takes), records: `batch`
 * blocks.  MAV_ERR_ARG: a NULL context, flow, F or records; batch outside [1, max_batch]; a threshold that is negative or not finite;
 * _dev form: flow, residual not aligned to 4, F to 8, records to 16. */
int mav_epipolar_residual(mav_ctx*, const float* flow, const double* F, double threshold, int batch, float* residual, uint8_t* mask,
                          mav_epipolar_record* records);
int mav_epipolar_residual_dev(mav_ctx*, const float* flow, const double* F, double threshold, int batch, float* residual, uint8_t* mask,
                              mav_epipolar_record* records);

#ifdef __cplusplus
}
#endif
#endif

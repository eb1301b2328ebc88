/* libmavflow -- a robust essential-matrix fit on the device: the algorithm of cv2.findEssentialMat(points1, points2, focal, pp, RANSAC,
 * prob=0.999, threshold=1.0) (reference src/detector.py:147-149) with the CALLER's sample subsets and Nister's five-point minimal solver,
 * for one pair set or a batch, and the same from the pairs of a float32 flow field.  Beside the best model E (normalised coordinates) a
 * call returns F = K^-T E K^-1 (pixel coordinates) in the layout mav_epipolar_residual(_dev) of mavflow_fundamental.h reads, so that
 * fit -> dense residual -> mask -> components runs with no host round trip.
 *
 * A header of its own beside mavflow.h, like mavflow_fundamental.h: the entry points here KEEP everything a context holds resident --
 * every mav_last_* reader returns after them what it returned before.  They run on the context's stream and hold no device memory of
 * the context's: the `_dev` forms take device pointers (and a caller's workspace) and only enqueue, the host forms take staging blocks
 * behind the last call's, run, synchronise and give the blocks back.  Conventions are mavflow.h's: 0 = OK, < 0 = MAV_ERR_*,
 * mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * What follows is the RANSAC frame of OpenCV 4.x modules/calib3d/src/five-point.cpp / ptsetreg.cpp AS REMEMBERED, PINNED TO NO cv2 BUILD
 * (none is available to this project), around a minimal solver that is NOT OpenCV's.  The subsets are an argument
 * (mavflow.essential.sample_subsets draws them from the caller's rng) and everything after the draw is deterministic.  What to re-check
 * first against a cv2 build: (1) OpenCV's Stewenius/Groebner action-matrix eigen-solver (a 10 x 10 eigen-decomposition), where this
 * uses Nister's tenth-degree polynomial and bisection: the real solutions are the same in exact arithmetic, their rounding and their
 * order are not; (2) its SVD null space of the 5 x 9 system, where this uses elimination with full pivoting; (3) its float32 points
 * in places, here everything is float64; (4) its getSubset retry loop, which redraws a degenerate sample where this counts the
 * hypothesis as invalid; (5) its returned scale and sign (OpenCV's E comes out of its solver with its own norm; this returns unit
 * Frobenius norm with the largest entry positive); (6) the several stacked E matrices (3k x 3) that it can return at n == 5, where this
 * runs the same RANSAC loop and returns one; (7) its inlier test on the Sampson error against threshold^2 after dividing the threshold
 * by the mean focal length, reproduced here as remembered; (8) the reference's swapped or literal arguments;
 * (9) the POLISH of step 10: OpenCV's solver has no such step, its models are its eigen-solver's as they come.  tests/essential_ref.py is
 * this text in numpy; the device equals it byte for byte.
 *
 * Everything is float64, every operation rounded on its own (no FMA contraction), expressions grouped as written, left to right.  No
 * transcendental function lies on a path that decides a winner or a returned bit; square root and division are correctly rounded.
 * finite(v) means v - v == 0.  -v is the exact negation.
 *
 * INPUTS.  src, dst: (batch, n, 2) float64 pixels (px, py) -> (PX, PY), 5 <= n <= MAV_ESSENTIAL_MAX_PAIRS.  subsets: (batch, max_iters, 5)
 *   int32, 1 <= max_iters <= MAV_ESSENTIAL_MAX_ITERS.  The camera fx, fy (finite, > 0), cx, cy (finite).  threshold >= 0, 0 < confidence < 1.
 *   NORMALISED POINTS, wherever a pair is used:  x = (px - cx) / fx, y = (py - cy) / fy, X = (PX - cx) / fx, Y = (PY - cy) / fy.
 *   t = threshold / ((fx + fy) / 2);  t2 = t * t.
 *
 * POLYNOMIALS.  A linear form in (x, y, z) is four coefficients in the order (x, y, z, 1); a quadratic is ten, in the order
 *   Q = (x^2, xy, xz, x, y^2, yz, y, z^2, z, 1); a cubic is twenty, in Nister's order
 *   C = (x^3, y^3, x^2y, xy^2, x^2z, x^2, y^2z, y^2, xyz, xy, xz^2, xz, x, yz^2, yz, y, z^3, z^2, z, 1).
 *   mul2(a, b), linear times linear: ten accumulators q[m] = +0.0; for i = 0 .. 3, for j = 0 .. 3 (i outer): q[m(i, j)] = q[m(i, j)] + a[i]*b[j],
 *     m(i, j) the place in Q of the product of the two monomials.
 *   mul3(q, l), quadratic times linear: twenty accumulators c[m] = +0.0; for i = 0 .. 9, for j = 0 .. 3 (i outer): c[m(i, j)] = c[m(i, j)] + q[i]*l[j].
 *   Sums, differences and multiples of polynomials are taken coefficient by coefficient.
 *   conv(a, b) of polynomials in z alone (coefficients in ASCENDING degree, da and db the degrees): accumulators o[m] = +0.0, m = 0 .. da + db;
 *     for i = 0 .. da, for j = 0 .. db (i outer): o[i + j] = o[i + j] + a[i]*b[j].
 *   horner(a, d, t), a in ascending degree: v = a[d]; for j = d - 1 down to 0: v = v*t + a[j].
 *
 * HYPOTHESIS `it` of an item, with (i0 .. i4) = subsets[it]:
 *   1. VALID INDICES: 0 <= ij < n for all five and pairwise distinct; otherwise the hypothesis is invalid and nothing is read through it.
 *   2. THE SYSTEM, 5 x 9, row r from pair ir on normalised points:   (X*x, X*y, X, Y*x, Y*y, Y, x, y, 1).
 *   3. GAUSS-JORDAN WITH FULL PIVOTING, a column permutation perm[0..8] starting as the identity.  Step k = 0 .. 4:
 *        pv = 0, (pr, pc) = (k, k); for r = k .. 4, for c = k .. 8, in this (row-major) order: v = |A[r][c]|; v > pv: pv = v, (pr, pc) = (r, c)
 *          (strict, so the first of equals wins and a NaN never wins);
 *        the hypothesis is INVALID unless pv > 0 and finite(pv);
 *        rows k and pr change places, columns k and pc change places (all five rows; perm[k] and perm[pc] too);
 *        p = A[k][k];  A[k][c] = A[k][c] / p for c = k + 1 .. 8;
 *        for every row r != k, r = 0 .. 4:  m = A[r][k];  A[r][c] = A[r][c] - m * A[k][c] for c = k + 1 .. 8.
 *   4. NULL VECTORS e1 .. e4, un-permuted, all entries +0.0 first:  for j = 1 .. 4:  ej[perm[i]] = -A[i][4 + j] for i = 0 .. 4;
 *        ej[perm[4 + j]] = 1.   E(x, y, z) = x*e1 + y*e2 + z*e3 + e4: entry m (row-major, m = 3*r + c) is the linear form
 *        E[r][c] = (e1[m], e2[m], e3[m], e4[m]).
 *   5. THE TEN CUBICS, rows of a 10 x 20 matrix M in the order C:
 *        row 0, det E:   P0 = mul2(E[1][1], E[2][2]) - mul2(E[1][2], E[2][1]);  P1 = mul2(E[1][0], E[2][2]) - mul2(E[1][2], E[2][0]);
 *                        P2 = mul2(E[1][0], E[2][1]) - mul2(E[1][1], E[2][0]);
 *                        row 0 = (mul3(P0, E[0][0]) - mul3(P1, E[0][1])) + mul3(P2, E[0][2]);
 *        S[i][j] = (mul2(E[i][0], E[j][0]) + mul2(E[i][1], E[j][1])) + mul2(E[i][2], E[j][2]) for i <= j, S[j][i] = S[i][j]   (E E^T);
 *        T = (S[0][0] + S[1][1]) + S[2][2];   L[i][j] = S[i][j] for i != j,  L[i][i] = S[i][i] - 0.5*T;
 *        row 1 + 3*i + j = (mul3(L[i][0], E[0][j]) + mul3(L[i][1], E[1][j])) + mul3(L[i][2], E[2][j])     (E E^T E - tr(E E^T) E / 2).
 *   6. GAUSS-JORDAN OF M WITH PARTIAL (ROW) PIVOTING.  Step k = 0 .. 9:
 *        pv = 0, pr = k; for r = k .. 9: v = |M[r][k]|; v > pv: pv = v, pr = r;   INVALID unless pv > 0 and finite(pv);
 *        rows k and pr change places (columns k .. 19);   p = M[k][k];  M[k][c] = M[k][c] / p for c = k + 1 .. 19;
 *        for every row r != k with r > k or r >= 4:  m = M[r][k];  M[r][c] = M[r][c] - m * M[k][c] for c = k + 1 .. 19.
 *      (Rows 0 .. 3 are not read again once they have been a pivot row; columns 0 .. 9 stand for the identity.)
 *   7. B(z).  With e, f, g, h, i, j = rows 4 .. 9 (the leading monomials x^2z, x^2, y^2z, y^2, xyz, xy) and r[c] = M[r][c], the row
 *      (e, f) gives three polynomials in z, ascending degree:
 *        bx = (e[12], e[11] - f[12], e[10] - f[11], -f[10]);   by = (e[15], e[14] - f[15], e[13] - f[14], -f[13]);
 *        b1 = (e[19], e[18] - f[19], e[17] - f[18], e[16] - f[17], -f[16])
 *      and is row 0 of B; (g, h) gives row 1 and (i, j) row 2 the same way.  B(z) (x, y, 1)^T = 0.
 *   8. n(z) = det B(z), eleven coefficients c[0 .. 10] in ascending degree:
 *        p1 = conv(B[1][1], B[2][2]) - conv(B[1][2], B[2][1])   (degree 7);   p2 = conv(B[1][0], B[2][2]) - conv(B[1][2], B[2][0])   (degree 7);
 *        p3 = conv(B[1][0], B[2][1]) - conv(B[1][1], B[2][0])   (degree 6);
 *        c = (conv(B[0][0], p1) - conv(B[0][1], p2)) + conv(B[0][2], p3).
 *   9. REAL ROOTS in ascending order, at most ten.  NO MODEL (zero slots) when c[10] == 0 or a coefficient is not finite, or when R is
 *      not finite:   R = 1 + max over i = 0 .. 9, from i = 0 upwards, of |c[i] / c[10]|  (max: a > b ? a : b, starting from 0).
 *        D[0] = c;  D[k + 1][j - 1] = (double)j * D[k][j] for j = 1 .. 10 - k   (the k-th derivative, degree 10 - k).
 *        clamp(t) = t < -R ? -R : (t > R ? R : t).   The list of level 9 is the one value clamp((-D[9][0]) / D[9][1]).
 *        Level k = 8 down to 0: the points are e = (-R, the list of level k + 1 in its order, R); v[j] = horner(D[k], 10 - k, e[j]).
 *        The new list, for j = 0, 1, ...: when v[j] == 0, e[j] joins it; when there is a next point and v[j], v[j + 1] have strictly
 *        opposite signs (one < 0, the other > 0), the interval gives one value by BISECTION, mavflow_fundamental.h's unchanged:
 *        lo = e[j], hi = e[j + 1], at most 128 steps of: mid = 0.5*(lo + hi); stop when mid == lo or mid == hi; fm = horner(mid);
 *        fm == 0: lo = mid, stop; (fm < 0) == (v[j] < 0): lo = mid, else hi = mid.  The value is lo.  A list takes no more than
 *        10 - k values (its polynomial's degree).  The roots are the list of level 0.  A multiple root without a sign change is not
 *        returned.
 *  10. MODEL SLOTS: root number s (s = 0 .. 9), z = the root, gives slot s:
 *        kx = horner(B[0][0], 3, z), ky = horner(B[0][1], 3, z), k1 = horner(B[0][2], 4, z); lx, ly, l1 the same of row 1 of B;
 *        v0 = ky*l1 - k1*ly;  v1 = k1*lx - kx*l1;  v2 = kx*ly - ky*lx;   x = v0 / v2;  y = v1 / v2;
 *        the slot is INVALID unless v2 != 0 and finite(x) and finite(y);
 *        POLISH, four Gauss-Newton steps of p = (x, y, z) on the ten constraints, evaluated on the 3 x 3 matrix itself (the hidden-variable
 *        polynomial loses digits where roots lie close together; the constraints at the matrix do not).  With 3 x 3 matrices row-major,
 *        (A B)[i][j] = (A[i][0]*B[0][j] + A[i][1]*B[1][j]) + A[i][2]*B[2][j], (A B^T)[i][j] = (A[i][0]*B[j][0] + A[i][1]*B[j][1]) +
 *        A[i][2]*B[j][2], tr3(A) = (A[0][0] + A[1][1]) + A[2][2] and det3 as in mavflow_fundamental.h, one step is:
 *          G[m] = ((p0*e1[m] + p1*e2[m]) + p2*e3[m]) + e4[m];   S = G G^T;   h = 0.5*tr3(S);
 *          r[0] = det3(G);   r[1 + 3i + j] = (S G)[i][j] - h*G[i][j];
 *          C = the cofactors of G:  C0 = G4*G8 - G5*G7, C1 = G5*G6 - G3*G8, C2 = G3*G7 - G4*G6, C3 = G2*G7 - G1*G8, C4 = G0*G8 - G2*G6,
 *              C5 = G1*G6 - G0*G7, C6 = G1*G5 - G2*G4, C7 = G2*G3 - G0*G5, C8 = G0*G4 - G1*G3;
 *          for q = 0, 1, 2 with D = e(q+1):   J[q][0] = sum C[m]*D[m] in index order from +0.0;   T = D G^T;   dS[i][j] = T[i][j] + T[j][i];
 *              dh = 0.5*tr3(dS);   J[q][1 + 3i + j] = (((dS G)[i][j] + (S D)[i][j]) - dh*G[i][j]) - h*D[i][j];
 *          N[a][b] = sum over k = 0 .. 9 of J[a][k]*J[b][k] (a <= b; N[b][a] = N[a][b]),  g[a] = sum over k of J[a][k]*r[k], in index
 *              order, one accumulator each starting at +0.0;
 *          dd = det3(N);   delta[a] = det3(N with column a replaced by g) / dd;
 *          when dd != 0 and all three delta are finite:  p[a] = p[a] - delta[a];  otherwise p stays.
 *        Then (x, y, z) = p and
 *        G[m] = ((x*e1[m] + y*e2[m]) + z*e3[m]) + e4[m], m = 0 .. 8;  then mavflow_fundamental.h's step 7:  q = sum G[m]*G[m] in index
 *        order, one accumulator starting at +0.0;  nrm = sqrt(q);  INVALID unless nrm > 0 and finite(nrm);  G[m] = G[m] / nrm;  the entry
 *        of largest magnitude (strict >, the first of equals) is made positive: when it is < 0, G[m] = -G[m] for all m.
 *        Slots without a root are invalid; an invalid slot is stored as zero.
 * SCORE.  For a pair's normalised (x, y) -> (X, Y) and row-major E[0..8], the Sampson error:
 *        a0 = (E0*x + E1*y) + E2;   a1 = (E3*x + E4*y) + E5;   a2 = (E6*x + E7*y) + E8;          (E (x, y, 1)^T)
 *        b0 = (E0*X + E3*Y) + E6;   b1 = (E1*X + E4*Y) + E7;                                      (E^T (X, Y, 1)^T)
 *        d = (X*a0 + Y*a1) + a2;    err = (d*d) / (((a0*a0 + a1*a1) + b0*b0) + b1*b1)
 *   count[it][slot] = the number of pairs with err <= t2: an integer; a NaN error is no inlier; an invalid slot has count -1.
 * CHOICE, the sequential loop of mavflow_fundamental.h with ten slots: niters = max_iters, best = none, best_count = 4; for it = 0, 1, ...
 *   while it < niters: for slot = 0 .. 9: when the slot is valid and count[it][slot] > best_count, then best = (it, slot), best_count =
 *   that count, niters = min(niters, need[best_count]).  All ten slots of an iteration that began are visited; the first of equal
 *   counts wins.  need[g], g = 0 .. n, is OpenCV's RANSACUpdateNumIters(confidence, (n - g) / n, 5, max_iters):
 *        g < 5: max_iters (never consulted);   w = (double)g / (double)n;  w2 = w*w;  den = 1 - (w2*w2)*w;
 *        den < DBL_MIN: 0 (so need[n] = 0);   ln = log(1 - confidence), ld = log(den);
 *        ld >= 0 or -ln >= max_iters * (-ld): max_iters;   else the quotient ln / ld rounded half to even.
 *   THE HOST BUILDS need[] and the device only looks it up, exactly as in mavflow_affine.h and mavflow_fundamental.h.
 *   iters_run = the number of iterations that began: max_iters without a winner, else max(final niters, best_iter + 1).
 *   valid = the valid slots among them.  No winner: ok = 0, E, F and the mask all zero.
 * OUTPUTS.  E (batch, 3, 3) float64: the best MINIMAL model, of unit Frobenius norm; no refinement.
 *   F (batch, 3, 3) float64 = K^-T E K^-1 for K = (fx 0 cx; 0 fy cy; 0 0 1), in pixel coordinates:
 *        for i = 0 .. 2:  G[i][0] = E[i][0] / fx;  G[i][1] = E[i][1] / fy;  G[i][2] = (E[i][2] - G[i][0]*cx) - G[i][1]*cy;      (E K^-1)
 *        for j = 0 .. 2:  H[0][j] = G[0][j] / fx;  H[1][j] = G[1][j] / fy;  H[2][j] = (G[2][j] - H[0][j]*cx) - H[1][j]*cy;      (K^-T G)
 *        then step 10's normalisation of H (unit Frobenius norm, the largest entry positive); F is all zero where that norm is not
 *        > 0 and finite.
 *   inliers[k] = 1 where err(E, k) <= t2, else 0.   sq_error = the sum over k = 0 .. n - 1 in index order, one accumulator starting at
 *   +0.0, of err(E, k) where pair k is an inlier and +0.0 where it is none (normalised units). */
#ifndef MAVFLOW_ESSENTIAL_H
#define MAVFLOW_ESSENTIAL_H

#include "mavflow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MAV_ESSENTIAL_MAX_PAIRS 65536       /* as MAV_FUNDAMENTAL_MAX_PAIRS */
#define MAV_ESSENTIAL_MAX_ITERS 4096

typedef struct {
    double  threshold;      /* 1.0, in pixels; finite, >= 0 */
    double  confidence;     /* 0.999; inside (0, 1) */
    double  fx, fy;         /* 1.0, 1.0: the focal lengths in pixels; finite, > 0 */
    double  cx, cy;         /* 0, 0: the principal point; finite */
    int32_t max_iters;      /* 1000; 1 .. MAV_ESSENTIAL_MAX_ITERS: the hypotheses per item in `subsets` */
    int32_t flags;          /* 0: no flag is defined */
} mav_essential_params;     /* 56 bytes */

typedef struct {
    int32_t ok;             /* 1: a model was found; 0: E, F and the mask are zero */
    int32_t inliers;        /* the winner's count, the number of ones in the mask */
    int32_t best_iter;      /* the winning hypothesis, or -1 */
    int32_t best_slot;      /* its slot (the root's rank, 0 .. 9), or -1 */
    int32_t iters_run;      /* the iterations that began */
    int32_t valid;          /* valid slots among the iterations that began */
    double  sq_error;       /* the inliers' summed err under E */
} mav_essential_record;     /* 32 bytes; every byte is written */

void mav_essential_defaults(mav_essential_params* p);
/* Bytes of workspace the _dev forms need for these shapes (the flow form's pair buffers included); 0 when the arguments would be refused. */
size_t mav_find_essential_workspace_bytes(int n, int batch, const mav_essential_params* params);

/* E, F (batch, 3, 3) float64, row-major; inliers (batch, n) uint8; records: `batch` blocks.
 * MAV_ERR_ARG, before anything is enqueued, the function's name in the message, the outputs untouched: a NULL pointer; n outside
 *   [5, MAV_ESSENTIAL_MAX_PAIRS]; max_iters outside [1, MAV_ESSENTIAL_MAX_ITERS]; batch outside [1, max_batch]; a threshold that is
 *   negative or not finite; a confidence outside (0, 1); fx or fy not finite or not > 0; cx or cy not finite; flags != 0;
 *   host forms: a subset with an index outside [0, n) or a repeated index;
 *   _dev forms (where such a subset is an invalid hypothesis, and nothing is read out of bounds whatever the subsets hold): src, dst,
 *   E, F not aligned to 8, subsets to 4, records and workspace to 16; a workspace smaller than mav_find_essential_workspace_bytes. */
int mav_find_essential(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_essential_params* params,
                       const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records);
int mav_find_essential_dev(mav_ctx*, const double* src, const double* dst, int n, int batch, const mav_essential_params* params,
                           const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, void* workspace,
                           size_t workspace_bytes);
/* The pairs coords[k] -> coords[k] + flow[y][x] of float32 fields (batch, H, W, 2) at n host (x, y) int32 coords, every one inside the
 * frame (as mav_flow_fundamental(_dev): range-checked on the host, copied with the call), then the fit.  The _dev form gathers the
 * pairs into its workspace; flow aligned to 8.  pairs_dst (host form, may be NULL): the (batch, n, 2) float64 destination points. */
int mav_flow_essential(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_essential_params* params,
                       const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, double* pairs_dst);
int mav_flow_essential_dev(mav_ctx*, const float* flow, const int32_t* coords, int n, int batch, const mav_essential_params* params,
                           const int32_t* subsets, double* E, double* F, uint8_t* inliers, mav_essential_record* records, void* workspace,
                           size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif

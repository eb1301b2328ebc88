// Robust affine fit (include/mavflow_affine.h has the algorithm; tests/affine_ref.py restates it in numpy and the device equals it byte
// for byte).  Three kernels on one stream: the hypotheses' inlier counts, the sequential choice, and the winner's mask, refinement and
// record.  float64 throughout, compiled with -ffp-contract=off; integer counts from ballots, no atomics of any kind: the same bytes on
// every run, at every batch position and in every context.  Every loop has a fixed bound; nothing is read through an index that was not
// range-checked first, whatever the triples hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mavflow_internal.h"
#include "../../include/mavflow_affine.h"

#define AFF_THREADS 256
#define AFF_WAVES (AFF_THREADS / 64)
#define AFF_CHUNK 1024                  // pairs of one LDS chunk: 4 planes of doubles, 32 B per pair, 32 KiB (two workgroups fit a CU's LDS)
#define AFF_HYP_PER_WAVE 4              // hypotheses a wave scores per staged chunk where the grid is not capped
#define AFF_GRID_CAP 2048               // workgroups of the score kernel in all items of a call

struct AffModel { double m[6]; bool valid; };

// "the angle at c is flat": OpenCV's 0.996 cosine test without the square root
__device__ static inline bool aff_flat(double ax, double ay, double bx, double by, double cx, double cy)
{
    const double d1x = bx - cx, d1y = by - cy, d2x = ax - cx, d2y = ay - cy;
    const double l1 = d1x * d1x + d1y * d1y, l2 = d2x * d2x + d2y * d2y, dot = d1x * d2x + d1y * d2y;
    return l1 == 0.0 || l2 == 0.0 || dot * dot > (0.996 * 0.996) * (l1 * l2);
}
__device__ static inline bool aff_finite(double v) { return v - v == 0.0; }
// the model through the three pairs of one triple (the same value in every lane that calls it)
__device__ static AffModel aff_model(const double* __restrict__ src, const double* __restrict__ dst, const int32_t* __restrict__ tri, int n)
{
    AffModel r;
    for (int j = 0; j < 6; j++) r.m[j] = 0.0;
    r.valid = false;
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || i0 == i1 || i0 == i2 || i1 == i2) return r;
    const double ax = src[2 * i0], ay = src[2 * i0 + 1], bx = src[2 * i1], by = src[2 * i1 + 1], cx = src[2 * i2], cy = src[2 * i2 + 1];
    const double Ax = dst[2 * i0], Ay = dst[2 * i0 + 1], Bx = dst[2 * i1], By = dst[2 * i1 + 1], Cx = dst[2 * i2], Cy = dst[2 * i2 + 1];
    if (aff_flat(ax, ay, bx, by, cx, cy) || aff_flat(Ax, Ay, Bx, By, Cx, Cy)) return r;
    const double dx1 = bx - ax, dy1 = by - ay, dx2 = cx - ax, dy2 = cy - ay;
    const double det = dx1 * dy2 - dx2 * dy1;
    if (!(det != 0.0)) return r;
    const double dX1 = Bx - Ax, dX2 = Cx - Ax, dY1 = By - Ay, dY2 = Cy - Ay;
    const double m00 = (dX1 * dy2 - dX2 * dy1) / det, m01 = (dx1 * dX2 - dx2 * dX1) / det, m02 = (Ax - m00 * ax) - m01 * ay;
    const double m10 = (dY1 * dy2 - dY2 * dy1) / det, m11 = (dx1 * dY2 - dx2 * dY1) / det, m12 = (Ay - m10 * ax) - m11 * ay;
    if (!(aff_finite(m00) && aff_finite(m01) && aff_finite(m02) && aff_finite(m10) && aff_finite(m11) && aff_finite(m12))) return r;
    r.m[0] = m00; r.m[1] = m01; r.m[2] = m02; r.m[3] = m10; r.m[4] = m11; r.m[5] = m12;
    r.valid = true;
    return r;
}
__device__ static inline double aff_err(const double* m, double x, double y, double X, double Y)
{
    const double e0 = ((m[0] * x + m[1] * y) + m[2]) - X, e1 = ((m[3] * x + m[4] * y) + m[5]) - Y;
    return e0 * e0 + e1 * e1;
}

// ---- the hypotheses' counts ----------------------------------------------------------------------------------------------------------
// grid (x, B).  A workgroup stages the item's pairs chunk by chunk in LDS; each of its four wavefronts scores one hypothesis at a time
// against the chunk, lanes striding over it, inliers counted by ballot and population count; lane 0 stores count[it] (first chunk) or
// adds the chunk's count to it (later chunks; only this wavefront ever touches count[it]).  An invalid hypothesis is stored as -1.
__global__ __launch_bounds__(AFF_THREADS) void k_affine_score(AffCall a)
{
    __shared__ double sx[AFF_CHUNK], sy[AFF_CHUNK], sX[AFF_CHUNK], sY[AFF_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double* src = a.src + (size_t)b * a.n * 2;
    const double* dst = a.dst + (size_t)b * a.n * 2;
    const int32_t* tri = a.triples + (size_t)b * a.max_iters * 3;
    int32_t* count = (int32_t*)(a.ws + aff_counts_offset(a.n)) + (size_t)b * a.max_iters;
    const int first = blockIdx.x * AFF_WAVES + wave, stride = gridDim.x * AFF_WAVES;
    for (int base = 0; base < a.n; base += AFF_CHUNK) {
        const int len = a.n - base < AFF_CHUNK ? a.n - base : AFF_CHUNK;
        __syncthreads();                                  // the previous chunk's readers are done
        for (int k = tid; k < len; k += AFF_THREADS) {
            const size_t o = 2 * (size_t)(base + k);
            sx[k] = src[o]; sy[k] = src[o + 1]; sX[k] = dst[o]; sY[k] = dst[o + 1];
        }
        __syncthreads();
        for (int it = first; it < a.max_iters; it += stride) {
            const AffModel m = aff_model(src, dst, tri + 3 * (size_t)it, a.n);
            int cnt = 0;
            if (m.valid)
                for (int k0 = 0; k0 < len; k0 += 64) {
                    const int k = k0 + lane;
                    bool in = false;
                    if (k < len) in = aff_err(m.m, sx[k], sy[k], sX[k], sY[k]) <= a.t2;        // a NaN error is no inlier
                    cnt += __popcll(__ballot(in));
                }
            if (lane == 0) count[it] = !m.valid ? -1 : base == 0 ? cnt : count[it] + cnt;
        }
    }
}

// ---- the choice --------------------------------------------------------------------------------------------------------------------------
// One wavefront per item reproduces the sequential loop 64 hypotheses at a time: within a block of 64 the next hypothesis the loop would
// accept is the FIRST lane whose count beats best_count and whose index is still below niters; accepting it moves both, and the ballot
// is taken again.  The loop's result, early stop included.  choice[b] = (best, niters, valid, best_count).
__global__ __launch_bounds__(64) void k_affine_choose(AffCall a)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* need = (const int32_t*)a.ws;
    const int32_t* count = (const int32_t*)(a.ws + aff_counts_offset(a.n)) + (size_t)b * a.max_iters;
    int32_t* choice = (int32_t*)(a.ws + aff_choice_offset(a.n, a.B, a.max_iters)) + 4 * (size_t)b;
    int niters = a.max_iters, best = -1, best_count = 2;
    for (int base = 0; base < a.max_iters; base += 64) {
        if (base >= niters) break;
        const int it = base + lane;
        const int c = it < a.max_iters ? count[it] : -1;
        for (int r = 0; r < 64; r++) {
            const unsigned long long cand = __ballot(c > best_count && it < niters);
            if (!cand) break;
            const int f = __ffsll((long long)cand) - 1;
            int cf = __shfl(c, f);
            cf = cf > a.n ? a.n : cf;                     // (a count never exceeds n; the table has n + 1 entries)
            best = base + f;
            best_count = cf;
            const int nd = need[cf];
            niters = nd < niters ? nd : niters;
        }
    }
    int valid = 0;
    for (int base = 0; base < a.max_iters; base += 64) {
        const int it = base + lane;
        valid += __popcll(__ballot(it < niters && count[it] >= 0));
    }
    if (lane == 0) { choice[0] = best; choice[1] = niters; choice[2] = valid; choice[3] = best < 0 ? 0 : best_count; }
}

// ---- mask, refinement, record ---------------------------------------------------------------------------------------------------------
// NS sums over k = 0 .. n - 1 in plain index order, one accumulator per sum, one lane per accumulator (the homography fit's form): all
// threads compute a chunk's terms into LDS, then lanes 0 .. NS - 1 add them up in order.  Planes are AFF_CHUNK + 1 doubles apart so that
// the adding lanes hit different banks.  The sums are in acc[0 .. NS) for every thread on return.
template <int NS, class F>
__device__ static void aff_sums(double (*term)[AFF_CHUNK + 1], double* acc, int n, F f)
{
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int base = 0; base < n; base += AFF_CHUNK) {
        const int len = n - base < AFF_CHUNK ? n - base : AFF_CHUNK;
        __syncthreads();
        for (int k = tid; k < len; k += AFF_THREADS) {
            double t[NS];
            f(base + k, t);
            for (int j = 0; j < NS; j++) term[j][k] = t[j];
        }
        __syncthreads();
        if (tid < NS)
            for (int k = 0; k < len; k++) s = s + term[tid][k];
    }
    if (tid < NS) acc[tid] = s;
    __syncthreads();
}

__global__ __launch_bounds__(AFF_THREADS) void k_affine_finish(AffCall a)
{
    __shared__ double term[7][AFF_CHUNK + 1];
    __shared__ double acc[8];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
    const double* src = a.src + (size_t)b * n * 2;
    const double* dst = a.dst + (size_t)b * n * 2;
    const int32_t* choice = (const int32_t*)(a.ws + aff_choice_offset(n, a.B, a.max_iters)) + 4 * (size_t)b;
    double* M = a.M + 6 * (size_t)b;
    uint8_t* inl = a.inliers + (size_t)b * n;
    mav_affine_record* rec = (mav_affine_record*)a.records + b;
    const int best = choice[0], niters = choice[1], valid = choice[2], g = choice[3];
    if (best < 0 || best >= a.max_iters) {                // (uniform over the workgroup)
        for (int k = tid; k < n; k += AFF_THREADS) inl[k] = 0;
        if (tid < 6) M[tid] = 0.0;
        if (tid == 0) { rec->ok = 0; rec->inliers = 0; rec->best_iter = -1; rec->iters_run = niters; rec->valid = valid; rec->refined = 0; rec->sq_error = 0.0; }
        return;
    }
    const AffModel m = aff_model(src, dst, a.triples + ((size_t)b * a.max_iters + best) * 3, n);
    const double t2 = a.t2;
    auto inlier = [&](int k) { return aff_err(m.m, src[2 * k], src[2 * k + 1], dst[2 * k], dst[2 * k + 1]) <= t2; };
    for (int k = tid; k < n; k += AFF_THREADS) inl[k] = inlier(k) ? 1 : 0;
    double R[6];
    for (int j = 0; j < 6; j++) R[j] = m.m[j];
    int refined = 0;
    if (a.refine) {
        aff_sums<4>(term, acc, n, [&](int k, double* t) {
            const bool in = inlier(k);
            t[0] = in ? src[2 * k] : 0.0; t[1] = in ? src[2 * k + 1] : 0.0; t[2] = in ? dst[2 * k] : 0.0; t[3] = in ? dst[2 * k + 1] : 0.0;
        });
        const double gd = (double)g;
        const double mx = acc[0] / gd, my = acc[1] / gd, mX = acc[2] / gd, mY = acc[3] / gd;
        aff_sums<7>(term, acc, n, [&](int k, double* t) {
            const bool in = inlier(k);
            const double u = src[2 * k] - mx, v = src[2 * k + 1] - my, P = dst[2 * k] - mX, Q = dst[2 * k + 1] - mY;
            t[0] = in ? u * u : 0.0; t[1] = in ? u * v : 0.0; t[2] = in ? v * v : 0.0; t[3] = in ? u * P : 0.0; t[4] = in ? v * P : 0.0;
            t[5] = in ? u * Q : 0.0; t[6] = in ? v * Q : 0.0;
        });
        const double Suu = acc[0], Suv = acc[1], Svv = acc[2], SuP = acc[3], SvP = acc[4], SuQ = acc[5], SvQ = acc[6];
        const double D = Suu * Svv - Suv * Suv, T = Suu + Svv;
        const double r00 = (SuP * Svv - SvP * Suv) / D, r01 = (Suu * SvP - Suv * SuP) / D, r02 = (mX - r00 * mx) - r01 * my;
        const double r10 = (SuQ * Svv - SvQ * Suv) / D, r11 = (Suu * SvQ - Suv * SuQ) / D, r12 = (mY - r10 * mx) - r11 * my;
        if (D > MAV_AFFINE_RANK_RATIO * (T * T) && aff_finite(r00) && aff_finite(r01) && aff_finite(r02) && aff_finite(r10) && aff_finite(r11) &&
            aff_finite(r12)) {
            R[0] = r00; R[1] = r01; R[2] = r02; R[3] = r10; R[4] = r11; R[5] = r12;
            refined = 1;
        }
    }
    aff_sums<1>(term, acc, n, [&](int k, double* t) {
        t[0] = inlier(k) ? aff_err(R, src[2 * k], src[2 * k + 1], dst[2 * k], dst[2 * k + 1]) : 0.0;
    });
    if (tid < 6) M[tid] = R[tid];
    if (tid == 0) {
        rec->ok = 1; rec->inliers = g; rec->best_iter = best; rec->iters_run = niters; rec->valid = valid; rec->refined = refined; rec->sq_error = acc[0];
    }
}

void launch_affine_score(hipStream_t st, const AffCall& a)
{
    const int per = (a.max_iters + AFF_WAVES * AFF_HYP_PER_WAVE - 1) / (AFF_WAVES * AFF_HYP_PER_WAVE);
    const int cap = AFF_GRID_CAP / a.B < 1 ? 1 : AFF_GRID_CAP / a.B;
    hipLaunchKernelGGL(k_affine_score, dim3(per < cap ? per : cap, a.B), dim3(AFF_THREADS), 0, st, a);
}
void launch_affine_choose(hipStream_t st, const AffCall& a) { hipLaunchKernelGGL(k_affine_choose, dim3(a.B), dim3(64), 0, st, a); }
void launch_affine_finish(hipStream_t st, const AffCall& a) { hipLaunchKernelGGL(k_affine_finish, dim3(a.B), dim3(AFF_THREADS), 0, st, a); }

// Global-motion subtraction (Detector.get_transformation_matrix / flow_vec_subtract, detector.py:119-202): the pair gather, the
// homography fit and the two full-frame passes.  Compiled with -ffp-contract=off: tests/global_motion_ref.py restates every
// operation of this file in numpy in the same order, and the tests compare bytes.
#include <float.h>

#include "mavflow_internal.h"

// ---- pair gather (detector.py:126-128) ---------------------------------------------------------------------------------------
// src[i] = double(coords[i]), dst[i] = double(coords[i]) + double(flow[y_i, x_i]): float64 + float32 is exact in float64.
__global__ __launch_bounds__(256) void k_pair_gather(const float* __restrict__ flow, const int32_t* __restrict__ coords, int n, int W, int H,
                                                     double* __restrict__ src, double* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    int x = coords[2 * i], y = coords[2 * i + 1];
    const double fx = (double)x, fy = (double)y;
    x = x < 0 ? 0 : (x >= W ? W - 1 : x);                 // (the host refuses coordinates outside the frame; never read out of bounds)
    y = y < 0 ? 0 : (y >= H ? H - 1 : y);
    const float2 f = *(const float2*)(flow + ((size_t)b * W * H + (size_t)y * W + x) * 2);
    const size_t o = ((size_t)b * n + i) * 2;
    src[o] = fx; src[o + 1] = fy;
    dst[o] = fx + (double)f.x; dst[o + 1] = fy + (double)f.y;
}
void launch_pair_gather(hipStream_t st, const float* flow, const int32_t* coords, int n, int B, int W, int H, double* src, double* dst)
{
    hipLaunchKernelGGL(k_pair_gather, dim3((n + 255) / 256, B), dim3(256), 0, st, flow, coords, n, W, H, src, dst);
}

// ---- homography fit ----------------------------------------------------------------------------------------------------------
// One workgroup per batch item.  Sums over the points run in plain index order with one accumulator per matrix entry (a thread
// per entry); the per-point terms they add are computed by all threads into `work` (global memory: n is not bounded by the LDS).
// The 9x9 / 8x8 eigen-decompositions run on wave 0 alone, a rotation's element updates spread over lanes 0 .. n - 1 (jacobi_eigen); the
// other waves wait at the next workgroup barrier.  Every loop has a fixed bound.
#define FIT_THREADS 256
#define JACOBI_SWEEPS 30
#define LM_ITERATIONS 10
#define RANK_RATIO 1e-12

// Wave-scope ordering point between LDS writes of some lanes and LDS reads of others.  One wavefront issues its LDS instructions in
// order, so what is needed is that the compiler neither moves an access across this point nor keeps an LDS value in a register over it.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Cyclic Jacobi on the symmetric n x n matrix A (row stride 9): eigenvalues on the diagonal, eigenvectors as columns of V.  Called by
// every lane of ONE wavefront (lane = 0 .. 63), A and V in LDS.  Every lane evaluates the off-diagonal sum and a rotation's apq, theta,
// t, c, s from the same LDS values (broadcast reads), so every decision is wave-uniform; lane k < n then carries the element updates:
// row k of the column update and row k of V (independent of each other), and, after an ordering point, column k of the row update,
// which reads what the column update wrote.  Every expression is the serial loop's: tests/global_motion_ref.py, same bytes.
__device__ static void jacobi_eigen(double* A, double* V, int n, int lane)
{
    if (lane < n)
        for (int j = 0; j < n; j++) V[lane * 9 + j] = lane == j ? 1.0 : 0.0;
    wave_sync();
    for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
        double off = 0.0;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) off = off + fabs(A[p * 9 + q]);
        if (!(off > 0.0)) break;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * 9 + q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq), app = A[p * 9 + p], aqq = A[q * 9 + q];
                if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    wave_sync();                                       // (every lane has read apq, app, aqq)
                    if (lane == 0) { A[p * 9 + q] = 0.0; A[q * 9 + p] = 0.0; }
                    wave_sync();
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                double t = isfinite(theta) ? 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)) : 0.0;
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                wave_sync();                                           // (every lane has read apq, app, aqq)
                if (lane < n) {
                    const int k = lane;
                    const double akp = A[k * 9 + p], akq = A[k * 9 + q], vkp = V[k * 9 + p], vkq = V[k * 9 + q];
                    A[k * 9 + p] = c * akp - s * akq; A[k * 9 + q] = s * akp + c * akq;
                    V[k * 9 + p] = c * vkp - s * vkq; V[k * 9 + q] = s * vkp + c * vkq;
                }
                wave_sync();
                if (lane < n) {
                    const int k = lane;
                    const double apk = A[p * 9 + k], aqk = A[q * 9 + k];
                    A[p * 9 + k] = c * apk - s * aqk; A[q * 9 + k] = s * apk + c * aqk;
                }
                wave_sync();
            }
    }
}
// entry e of the upper triangle of an m x m matrix in row-major order -> (j, k), j <= k
__device__ __forceinline__ void upper_entry(int e, int m, int* j, int* k)
{
    int r = 0;
    while (e >= m - r) { e -= m - r; r++; }
    *j = r; *k = r + e;
}
// element j of the DLT rows of a point with normalised source (X, Y) and destination (x, y)
__device__ __forceinline__ double dlt_lx(int j, double X, double Y, double x)
{
    switch (j) { case 0: return X; case 1: return Y; case 2: return 1.0; case 6: return -x * X; case 7: return -x * Y; case 8: return -x; default: return 0.0; }
}
__device__ __forceinline__ double dlt_ly(int j, double X, double Y, double y)
{
    switch (j) { case 3: return X; case 4: return Y; case 5: return 1.0; case 6: return -y * X; case 7: return -y * Y; case 8: return -y; default: return 0.0; }
}
// Element j of the Jacobian rows from a point's stored terms P = a, b, ww, -a xi, -b xi, -a yi, -b yi: which of the seven arrays it is
// (lm_jx_term / lm_jy_term, -1: the element is 0), and its value.  The array is chosen once per matrix entry, outside the sum over the
// points, so that the lanes of a wavefront -- one entry each -- issue the same loads side by side instead of one switch case after the
// other; the value is the one the switch returned.
__device__ __forceinline__ int lm_jx_term(int j) { return j < 3 ? j : j == 6 ? 3 : j == 7 ? 4 : -1; }
__device__ __forceinline__ int lm_jy_term(int j) { return j >= 3 && j < 6 ? j - 3 : j == 6 ? 5 : j == 7 ? 6 : -1; }
__device__ __forceinline__ double lm_term(const double* P, size_t n, int a, int i)
{
    const double v = P[(size_t)(a < 0 ? 0 : a) * n + i];
    return a < 0 ? 0.0 : v;
}
// projection of (X, Y) by h (8 parameters, h[8] = 1): ww, xi, yi
__device__ __forceinline__ void lm_project(const double* h, double X, double Y, double* ww, double* xi, double* yi)
{
    const double Wd = (h[6] * X + h[7] * Y) + 1.0;
    *ww = fabs(Wd) > DBL_EPSILON ? 1.0 / Wd : 0.0;
    *xi = ((h[0] * X + h[1] * Y) + h[2]) * *ww;
    *yi = ((h[3] * X + h[4] * Y) + h[5]) * *ww;
}

// sum of term(0) .. term(n - 1) in index order with one accumulator.  The terms of 16 consecutive points are fetched before they are
// added, so that the loads of a block are in flight together; the order of the additions -- and so every bit of the sum -- is that
// of the plain loop.  (Measured: the fit's time did not change with it; where the time was and is: DESIGN.md 4d.)
template <typename F>
__device__ __forceinline__ double seq_sum(int n, F term)
{
    double acc = 0.0;
    for (int i0 = 0; i0 < n; i0 += 16) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; u++) t[u] = i0 + u < n ? term(i0 + u) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++)
            if (i0 + u < n) acc = i0 + u == 0 ? t[u] : acc + t[u];
    }
    return acc;
}

// work: 9 * n doubles per item
__global__ __launch_bounds__(FIT_THREADS) void k_homography_fit(const double* __restrict__ src_all, const double* __restrict__ dst_all, int n,
                                                               double* __restrict__ work_all, double* __restrict__ H_out, int* __restrict__ ok_out)
{
    __shared__ double A[81], V[81], cen[4], scl[4], h[8], hn[8], grad[8];
    __shared__ double S_cur, lambda;
    __shared__ int state;                              // 1: fitting, 0: failed, 2: refinement finished
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* src = src_all + (size_t)b * n * 2;
    const double* dst = dst_all + (size_t)b * n * 2;
    double* work = work_all + (size_t)b * n * 9;
    const size_t N = (size_t)n;
    const double fn = (double)n;

    // normalisation: centroids, then per-axis scale n / sum |v - centroid|
    if (tid < 4) {
        const double* v = (tid < 2 ? src : dst) + (tid & 1);
        const double c = seq_sum(n, [&](int i) { return v[2 * i]; }) / fn;
        cen[tid] = c;
        scl[tid] = seq_sum(n, [&](int i) { return fabs(v[2 * i] - c); });
    }
    if (tid == 0) state = 1;
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 4; k++) {
            if (!(scl[k] > DBL_EPSILON) || !isfinite(scl[k])) state = 0;
        }
        if (state)
            for (int k = 0; k < 4; k++) scl[k] = fn / scl[k];
    }
    __syncthreads();
    if (state) {                                       // (uniform: state is read after a barrier)
        for (int i = tid; i < n; i += FIT_THREADS) {
            work[i] = (src[2 * i] - cen[0]) * scl[0];
            work[N + i] = (src[2 * i + 1] - cen[1]) * scl[1];
            work[2 * N + i] = (dst[2 * i] - cen[2]) * scl[2];
            work[3 * N + i] = (dst[2 * i + 1] - cen[3]) * scl[3];
        }
    }
    __syncthreads();
    if (state && tid < 45) {
        int j, k;
        upper_entry(tid, 9, &j, &k);
        const double acc = seq_sum(n, [&](int i) {
            const double X = work[i], Y = work[N + i], x = work[2 * N + i], y = work[3 * N + i];
            return dlt_lx(j, X, Y, x) * dlt_lx(k, X, Y, x) + dlt_ly(j, X, Y, y) * dlt_ly(k, X, Y, y);
        });
        A[j * 9 + k] = acc; A[k * 9 + j] = acc;
    }
    __syncthreads();
    if (state && tid < 64) jacobi_eigen(A, V, 9, tid); // wave 0, no workgroup barrier inside: the other waves wait at the next one
    if (state && tid == 0) {
        int kmin = 0;
        double wmax = fabs(A[0]);
        for (int k = 1; k < 9; k++) {
            if (A[k * 9 + k] < A[kmin * 9 + kmin]) kmin = k;
            if (fabs(A[k * 9 + k]) > wmax) wmax = fabs(A[k * 9 + k]);
        }
        bool have = false;
        double second = 0.0;
        for (int k = 0; k < 9; k++)
            if (k != kmin && (!have || A[k * 9 + k] < second)) { second = A[k * 9 + k]; have = true; }
        if (!(second > RANK_RATIO * wmax)) state = 0;
        else {
            // H = inv(T_dst) H0 T_src
            const double id[3][3] = {{1.0 / scl[2], 0.0, cen[2]}, {0.0, 1.0 / scl[3], cen[3]}, {0.0, 0.0, 1.0}};
            const double ts[3][3] = {{scl[0], 0.0, -cen[0] * scl[0]}, {0.0, scl[1], -cen[1] * scl[1]}, {0.0, 0.0, 1.0}};
            double T[3][3], Hm[3][3];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    T[i][j] = (id[i][0] * V[(0 + j) * 9 + kmin] + id[i][1] * V[(3 + j) * 9 + kmin]) + id[i][2] * V[(6 + j) * 9 + kmin];
            bool fin = true;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    Hm[i][j] = (T[i][0] * ts[0][j] + T[i][1] * ts[1][j]) + T[i][2] * ts[2][j];
                    fin = fin && isfinite(Hm[i][j]);
                }
            if (!fin || Hm[2][2] == 0.0) state = 0;
            else {
                const double inv = 1.0 / Hm[2][2];
                for (int i = 0; i < 8; i++) {
                    h[i] = Hm[i / 3][i % 3] * inv;
                    if (!isfinite(h[i])) state = 0;
                }
                if (!isfinite(Hm[2][2] * inv)) state = 0;
                lambda = 1e-3;
            }
        }
    }
    __syncthreads();

    // refinement: squared error at h, then at most LM_ITERATIONS damped steps
    if (state == 1) {
        for (int i = tid; i < n; i += FIT_THREADS) {
            double ww, xi, yi;
            lm_project(h, src[2 * i], src[2 * i + 1], &ww, &xi, &yi);
            const double rx = xi - dst[2 * i], ry = yi - dst[2 * i + 1];
            work[i] = rx * rx + ry * ry;
        }
    }
    __syncthreads();
    if (state == 1 && tid == 0) S_cur = seq_sum(n, [&](int i) { return work[i]; });
    __syncthreads();
    for (int it = 0; it < LM_ITERATIONS; it++) {
        if (state == 1 && tid == 0 && !(S_cur > 0.0)) state = 2;
        __syncthreads();
        const bool run = state == 1;                   // uniform
        if (run) {
            for (int i = tid; i < n; i += FIT_THREADS) {
                const double X = src[2 * i], Y = src[2 * i + 1];
                double ww, xi, yi;
                lm_project(h, X, Y, &ww, &xi, &yi);
                const double a = X * ww, bb = Y * ww;
                work[i] = a; work[N + i] = bb; work[2 * N + i] = ww;
                work[3 * N + i] = -a * xi; work[4 * N + i] = -bb * xi;
                work[5 * N + i] = -a * yi; work[6 * N + i] = -bb * yi;
                work[7 * N + i] = xi - dst[2 * i]; work[8 * N + i] = yi - dst[2 * i + 1];
            }
        }
        __syncthreads();
        if (run && tid < 36) {
            int j, k;
            upper_entry(tid, 8, &j, &k);
            const int xj = lm_jx_term(j), xk = lm_jx_term(k), yj = lm_jy_term(j), yk = lm_jy_term(k);
            const double acc = seq_sum(n, [&](int i) {
                return lm_term(work, N, xj, i) * lm_term(work, N, xk, i) + lm_term(work, N, yj, i) * lm_term(work, N, yk, i);
            });
            A[j * 9 + k] = acc; A[k * 9 + j] = acc;
        } else if (run && tid >= 64 && tid < 72) {      // (a second wave: the gradient)
            const int j = tid - 64;
            const int xj = lm_jx_term(j), yj = lm_jy_term(j);
            grad[j] = seq_sum(n, [&](int i) { return lm_term(work, N, xj, i) * work[7 * N + i] + lm_term(work, N, yj, i) * work[8 * N + i]; });
        }
        __syncthreads();
        if (run && tid < 64) {                         // wave 0, as above
            if (tid < 8) A[tid * 9 + tid] = A[tid * 9 + tid] + lambda * A[tid * 9 + tid];
            wave_sync();
            jacobi_eigen(A, V, 8, tid);
        }
        if (run && tid == 0) {
            double wmax = 0.0;
            for (int k = 0; k < 8; k++)
                if (fabs(A[k * 9 + k]) > wmax) wmax = fabs(A[k * 9 + k]);
            double d[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < 8; k++) {
                const double w = A[k * 9 + k];
                if (!(fabs(w) > DBL_EPSILON * wmax)) continue;
                double dot = 0.0;
                for (int j = 0; j < 8; j++) dot = dot + V[j * 9 + k] * grad[j];
                const double coef = dot / w;
                for (int j = 0; j < 8; j++) d[j] = d[j] + V[j * 9 + k] * coef;
            }
            for (int j = 0; j < 8; j++) hn[j] = h[j] - d[j];
        }
        __syncthreads();
        if (run) {
            for (int i = tid; i < n; i += FIT_THREADS) {
                double ww, xi, yi;
                lm_project(hn, src[2 * i], src[2 * i + 1], &ww, &xi, &yi);
                const double rx = xi - dst[2 * i], ry = yi - dst[2 * i + 1];
                work[i] = rx * rx + ry * ry;
            }
        }
        __syncthreads();
        if (run && tid == 0) {
            const double acc = seq_sum(n, [&](int i) { return work[i]; });
            if (acc < S_cur) {
                for (int j = 0; j < 8; j++) h[j] = hn[j];
                S_cur = acc;
                lambda = lambda / 10.0;
            } else lambda = lambda * 10.0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        bool good = state != 0;
        for (int j = 0; j < 8 && good; j++) good = isfinite(h[j]);
        for (int j = 0; j < 8; j++) H_out[9 * b + j] = good ? h[j] : 0.0;
        H_out[9 * b + 8] = good ? 1.0 : 0.0;
        ok_out[b] = good ? 1 : 0;
    }
}
size_t homography_work_doubles(int n) { return (size_t)n * 9; }
void launch_homography_fit(hipStream_t st, const double* src, const double* dst, int n, int B, double* work, double* H, int* ok)
{
    hipLaunchKernelGGL(k_homography_fit, dim3(B), dim3(FIT_THREADS), 0, st, src, dst, n, work, H, ok);
}

// ---- the full-frame passes (detector.py:164-185, im_helpers.py:188-199) ------------------------------------------------------
// global_motion in double in the reference's order, rounded to float32; warped = global_motion - flow and its magnitude in float32.
struct MotionPx { float g0, g1, w0, w1, mag; };
__device__ __forceinline__ MotionPx motion_px(const double* M, int x, int y, float u, float v)
{
    const double dx = (double)x, dy = (double)y;
    MotionPx p;
    p.g0 = (float)(((M[0] * dx + M[1] * dy) + M[2]) - dx);
    p.g1 = (float)(((M[3] * dx + M[4] * dy) + M[5]) - dy);
    p.w0 = p.g0 - u;
    p.w1 = p.g1 - v;
    p.mag = sqrtf(p.w0 * p.w0 + p.w1 * p.w1);
    return p;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other > k ? other : k;
    }
    return k;
}
// Pass A: two pixels per thread (16 bytes of flow).  key[b] (zeroed by the caller) = max of (float bits of mag << 32) | ~pixel index:
// the largest magnitude, the first pixel among equals.  warped / mag / gm: optional outputs.
__global__ __launch_bounds__(256) void k_motion_pass_a(const float* __restrict__ flow, const double* __restrict__ M_all, int m_stride, int W, int H,
                                                       float* __restrict__ warped, float* __restrict__ mag, float* __restrict__ gm,
                                                       unsigned long long* __restrict__ key)
{
    const int b = blockIdx.y;
    const size_t n0 = (size_t)W * H, base = (size_t)b * n0;
    const float* f = flow + base * 2;
    double M[6];
    for (int i = 0; i < 6; i++) M[i] = M_all[(size_t)b * m_stride + i];
    const bool vec = ((uintptr_t)f & 15) == 0 && (!warped || ((uintptr_t)(warped + base * 2) & 15) == 0) &&
                     (!gm || ((uintptr_t)(gm + base * 2) & 15) == 0) && (!mag || ((uintptr_t)(mag + base) & 7) == 0);     // uniform per image
    const size_t pairs = (n0 + 1) / 2;
    unsigned long long best = 0ull;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (size_t)gridDim.x * 256) {
        const size_t p0 = 2 * q;
        const bool two = p0 + 1 < n0;
        float4 in;
        if (vec && two) in = *(const float4*)(f + p0 * 2);
        else {
            const float2 a = *(const float2*)(f + p0 * 2);
            const float2 c = two ? *(const float2*)(f + p0 * 2 + 2) : make_float2(0.f, 0.f);
            in = make_float4(a.x, a.y, c.x, c.y);
        }
        const int y0 = (int)(p0 / W), x0 = (int)(p0 - (size_t)y0 * W);
        const int x1 = x0 + 1 < W ? x0 + 1 : 0, y1 = x0 + 1 < W ? y0 : y0 + 1;
        const MotionPx a = motion_px(M, x0, y0, in.x, in.y);
        const MotionPx c = motion_px(M, x1, y1, in.z, in.w);
        unsigned long long k = ((unsigned long long)__float_as_uint(a.mag) << 32) | (unsigned)~(unsigned)p0;
        best = k > best ? k : best;
        if (two) {
            k = ((unsigned long long)__float_as_uint(c.mag) << 32) | (unsigned)~(unsigned)(p0 + 1);
            best = k > best ? k : best;
        }
        if (vec && two) {
            if (warped) *(float4*)(warped + (base + p0) * 2) = make_float4(a.w0, a.w1, c.w0, c.w1);
            if (gm) *(float4*)(gm + (base + p0) * 2) = make_float4(a.g0, a.g1, c.g0, c.g1);
            if (mag) *(float2*)(mag + base + p0) = make_float2(a.mag, c.mag);
        } else {
            if (warped) { *(float2*)(warped + (base + p0) * 2) = make_float2(a.w0, a.w1); if (two) *(float2*)(warped + (base + p0 + 1) * 2) = make_float2(c.w0, c.w1); }
            if (gm) { *(float2*)(gm + (base + p0) * 2) = make_float2(a.g0, a.g1); if (two) *(float2*)(gm + (base + p0 + 1) * 2) = make_float2(c.g0, c.g1); }
            if (mag) { mag[base + p0] = a.mag; if (two) mag[base + p0 + 1] = c.mag; }
        }
    }
    if (key) {
        best = wave_max_u64(best);
        if ((threadIdx.x & 63) == 0 && best) atomicMax(&key[b], best);
    }
}
// Pass B: four pixels per thread; the magnitude is recomputed (same bytes as pass A's), normalised with the image's maximum from key[b]
// in float32 -- (|mag| * 255) / max, round half to even -- and stored as u8.  A maximum of 0 gives an all-zero image.
__global__ __launch_bounds__(256) void k_motion_pass_b(const float* __restrict__ flow, const double* __restrict__ M_all, int m_stride, int W, int H,
                                                       const unsigned long long* __restrict__ key, uint8_t* __restrict__ gray)
{
    const int b = blockIdx.y;
    const size_t n0 = (size_t)W * H, base = (size_t)b * n0;
    const float* f = flow + base * 2;
    uint8_t* g = gray + base;
    double M[6];
    for (int i = 0; i < 6; i++) M[i] = M_all[(size_t)b * m_stride + i];
    const float mx = __uint_as_float((unsigned)(key[b] >> 32));
    const bool vec = ((uintptr_t)f & 15) == 0 && ((uintptr_t)g & 3) == 0;
    const size_t quads = (n0 + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
        const size_t p0 = 4 * q;
        const int cnt = n0 - p0 >= 4 ? 4 : (int)(n0 - p0);
        float in[8];
        if (vec && cnt == 4) {
            const float4 a = *(const float4*)(f + p0 * 2), c = *(const float4*)(f + p0 * 2 + 4);
            in[0] = a.x; in[1] = a.y; in[2] = a.z; in[3] = a.w; in[4] = c.x; in[5] = c.y; in[6] = c.z; in[7] = c.w;
        } else {
            for (int i = 0; i < 4; i++) {
                const float2 a = i < cnt ? *(const float2*)(f + (p0 + i) * 2) : make_float2(0.f, 0.f);
                in[2 * i] = a.x; in[2 * i + 1] = a.y;
            }
        }
        int y = (int)(p0 / W), x = (int)(p0 - (size_t)y * W);
        uint8_t o[4];
        for (int i = 0; i < 4; i++) {
            const MotionPx p = motion_px(M, x, y, in[2 * i], in[2 * i + 1]);
            o[i] = mx > 0.0f ? (uint8_t)rintf((fabsf(p.mag) * 255.0f) / mx) : (uint8_t)0;
            if (++x == W) { x = 0; y++; }
        }
        if (vec && cnt == 4) *(uchar4*)(g + p0) = make_uchar4(o[0], o[1], o[2], o[3]);
        else
            for (int i = 0; i < cnt; i++) g[p0 + i] = o[i];
    }
}
static int motion_blocks(size_t items)
{
    const size_t need = (items + 255) / 256;
    return (int)(need < 2048 ? (need ? need : 1) : 2048);
}
void launch_motion_pass_a(hipStream_t st, const float* flow, const double* M, int m_stride, int B, int W, int H, float* warped, float* mag,
                          float* gm, unsigned long long* key)
{
    hipLaunchKernelGGL(k_motion_pass_a, dim3(motion_blocks(((size_t)W * H + 1) / 2), B), dim3(256), 0, st, flow, M, m_stride, W, H, warped, mag,
                       gm, key);
}
void launch_motion_pass_b(hipStream_t st, const float* flow, const double* M, int m_stride, int B, int W, int H, const unsigned long long* key,
                          uint8_t* gray)
{
    hipLaunchKernelGGL(k_motion_pass_b, dim3(motion_blocks(((size_t)W * H + 3) / 4), B), dim3(256), 0, st, flow, M, m_stride, W, H, key, gray);
}

// ---- glue between the passes and the window search ---------------------------------------------------------------------------
// analyze_pyramid's record -> the window optimize_window starts from: (x, y, 64, 64), or the zero rectangle when no window scored
__global__ void k_motion_window(const int64_t* __restrict__ pyr, int B, int32_t* __restrict__ win)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool any = pyr[6 * b] != 0;
    win[4 * b] = any ? (int32_t)pyr[6 * b + 1] : 0;
    win[4 * b + 1] = any ? (int32_t)pyr[6 * b + 2] : 0;
    win[4 * b + 2] = any ? 64 : 0;
    win[4 * b + 3] = any ? 64 : 0;
}
// the per-item record: opt_score / opt_win null = no optimisation (the window search's own window, score 0); ok null = every item valid
__global__ void k_motion_pack(const unsigned long long* __restrict__ key, const int64_t* __restrict__ pyr, const int32_t* __restrict__ win,
                              const int64_t* __restrict__ opt_score, const int32_t* __restrict__ opt_win, const int* __restrict__ ok, int B,
                              int W, mav_motion_result* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    mav_motion_result r;
    const unsigned long long k = key[b];
    const unsigned idx = ~(unsigned)(k & 0xFFFFFFFFull);
    r.max_mag = __uint_as_float((unsigned)(k >> 32));
    r.max_row = (int32_t)(idx / (unsigned)W);
    r.max_col = (int32_t)(idx % (unsigned)W);
    r.reserved = 0;
    for (int i = 0; i < 6; i++) r.window[i] = pyr[6 * b + i];
    r.opt_score = opt_score ? opt_score[b] : 0;
    for (int i = 0; i < 4; i++) r.opt_window[i] = opt_win ? opt_win[4 * b + i] : win[4 * b + i];
    if (ok && !ok[b]) {
        r.max_mag = 0.f; r.max_row = r.max_col = 0;
        for (int i = 0; i < 6; i++) r.window[i] = 0;
        r.opt_score = 0;
        for (int i = 0; i < 4; i++) r.opt_window[i] = 0;
    }
    out[b] = r;
}
void launch_motion_window(hipStream_t st, const int64_t* pyr, int B, int32_t* win)
{
    hipLaunchKernelGGL(k_motion_window, dim3((B + 63) / 64), dim3(64), 0, st, pyr, B, win);
}
void launch_motion_pack(hipStream_t st, const unsigned long long* key, const int64_t* pyr, const int32_t* win, const int64_t* opt_score,
                        const int32_t* opt_win, const int* ok, int B, int W, mav_motion_result* out)
{
    hipLaunchKernelGGL(k_motion_pack, dim3((B + 63) / 64), dim3(64), 0, st, key, pyr, win, opt_score, opt_win, ok, B, W, out);
}

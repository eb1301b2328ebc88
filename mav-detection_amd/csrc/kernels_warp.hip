// Image warps (include/mavflow_warp.h): cv2.remap / warpAffine / warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0, restated from
// OpenCV 4.x; Farneback.warp_flow with the map generated in the kernel; Detector.warp_method with subtraction, magnitude and argmax as an
// epilogue.  ONE sampling body (warp_sample), instantiated over a coordinate policy (Coord*) and a pixel format.  Compiled with
// -ffp-contract=off: tests/warp_ref.py restates every operation of this file in numpy in the same order, and the tests compare bytes.
//
// Shape of the pass: a memory-bound gather.  One destination pixel, all channels, per thread; consecutive lanes are consecutive pixels of
// a row, so map reads and destination writes coalesce and the four taps of neighbouring lanes fall into the same cache lines for every
// warp that is locally smooth; blockIdx.y is the image.  Taps are loaded branch-free from clamped positions and zeroed by predicate.
// The matrix policies invert their matrix once per workgroup (thread 0, into LDS).  No floating-point atomics.
#include <limits.h>

#include "mavflow_internal.h"
#include "../../include/mavflow_warp.h"

#define WARP_WG 256     // threads of a workgroup
// Most workgroups per image of a launch; the rest of the frame is reached by the grid-stride loop.  Measured (profiles/warp/caps.txt:
// A/B builds with -DWARP_CAP through tools/warp_probe.py --lib): 1024, 2048 and 4096 lie within 1 % of each other in the geometric
// mean over all routes; a quarter turn at batch 16 gains 7 - 19 % without a cap, a smooth warp loses 2 - 7 % there.
#ifndef WARP_CAP
#define WARP_CAP 2048
#endif
// warp_method's cap: every workgroup ends in one atomic on its image's key, so fewer, longer workgroups (measured in the same builds:
// 512 is the fastest or within 10 % of it at every size; 8192 costs 3.5 - 4.8x)
#ifndef WARP_METHOD_CAP
#define WARP_METHOD_CAP 512
#endif

__device__ __forceinline__ float wcanon(float v) { return v != v ? __int_as_float(0x7FC00000) : v; }

// ---- pixel formats -------------------------------------------------------------------------------------------------------------------
template <int F> struct WarpFmt;
template <> struct WarpFmt<MAV_WARP_U8C1> { typedef uint8_t T; enum { C = 1 }; };
template <> struct WarpFmt<MAV_WARP_U8C3> { typedef uint8_t T; enum { C = 3 }; };
template <> struct WarpFmt<MAV_WARP_F32C1> { typedef float T; enum { C = 1 }; };
template <> struct WarpFmt<MAV_WARP_F32C2> { typedef float T; enum { C = 2 }; };

// ---- the one sampling body: SAMPLING of the header, steps 1 - 4 ----------------------------------------------------------------------
// src: one image.  (qx, qy): the position in 1/32 pixel; !fits: wholly outside.  out: the C channels of the element.
template <int F>
__device__ __forceinline__ void warp_sample(const typename WarpFmt<F>::T* __restrict__ src, int W, int H, bool fits, int qx, int qy,
                                            typename WarpFmt<F>::T* out)
{
    typedef typename WarpFmt<F>::T T;
    enum { C = WarpFmt<F>::C };
    int sx = qx >> 5, sy = qy >> 5;                                                           // arithmetic shifts
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
    sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
    const int ax = qx & 31, ay = qy & 31;
    const bool inside = fits && !(sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0);
    const bool xa = sx >= 0, xb = sx + 1 < W, ya = sy >= 0, yb = sy + 1 < H;                  // (sx < W, sx + 1 >= 0 where `inside`)
    const int cxa = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx), cxb = sx + 1 < 0 ? 0 : (sx + 1 > W - 1 ? W - 1 : sx + 1);
    const int cya = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy), cyb = sy + 1 < 0 ? 0 : (sy + 1 > H - 1 ? H - 1 : sy + 1);
    const size_t ra = (size_t)cya * W, rb = (size_t)cyb * W;
    const size_t ia = (ra + cxa) * C, ib = (ra + cxb) * C, ic = (rb + cxa) * C, id = (rb + cxb) * C;     // always in range
    const bool va = inside && ya && xa, vb = inside && ya && xb, vc = inside && yb && xa, vd = inside && yb && xb;
    T a[C], b[C], c[C], d[C];
    if (F == MAV_WARP_F32C2 && ((uintptr_t)src & 7) == 0) {                                   // the pair as one access where the pointer allows it
        const float2 pa = *(const float2*)(src + ia), pb = *(const float2*)(src + ib), pc = *(const float2*)(src + ic), pd = *(const float2*)(src + id);
        a[0] = pa.x; a[C - 1] = pa.y; b[0] = pb.x; b[C - 1] = pb.y; c[0] = pc.x; c[C - 1] = pc.y; d[0] = pd.x; d[C - 1] = pd.y;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) { a[k] = src[ia + k]; b[k] = src[ib + k]; c[k] = src[ic + k]; d[k] = src[id + k]; }
    }
    if (sizeof(T) == 4) {
        const float fx = (float)ax * 0.03125f, fy = (float)ay * 0.03125f;
        const float gx = 1.0f - fx, gy = 1.0f - fy;
        const float w00 = gy * gx, w01 = gy * fx, w10 = fy * gx, w11 = fy * fx;              // multiples of 1/1024
#pragma unroll
        for (int k = 0; k < C; k++) {
            const float t00 = va ? (float)a[k] : 0.0f, t01 = vb ? (float)b[k] : 0.0f, t10 = vc ? (float)c[k] : 0.0f, t11 = vd ? (float)d[k] : 0.0f;
            out[k] = (T)wcanon(((t00 * w00 + t01 * w01) + t10 * w10) + t11 * w11);           // wholly outside: every tap is 0 and the sum +0.0
        }
    } else {
        const int w00 = 32 * (32 - ay) * (32 - ax), w01 = 32 * (32 - ay) * ax, w10 = 32 * ay * (32 - ax), w11 = 32 * ay * ax;     // sum 32768
#pragma unroll
        for (int k = 0; k < C; k++) {
            const int t00 = va ? (int)a[k] : 0, t01 = vb ? (int)b[k] : 0, t10 = vc ? (int)c[k] : 0, t11 = vd ? (int)d[k] : 0;
            out[k] = (T)((t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + 16384) >> 15);
        }
    }
}

// ---- coordinate policies: COORDINATES of the header ------------------------------------------------------------------------------------
// What a launch works on, all device pointers.  a, b: the policy's operands (map_xy | map_x, map_y | flow | M).
struct WarpArgs {
    const void* src; void* dst; const void* a; const void* b;
    int W, H, flags;
    float* diff; float* mag; unsigned long long* key;     // warp_method alone
};
// A policy: LDS doubles it needs, setup() by thread 0 of the workgroup for image `img`, at() per destination pixel -> fits.
__device__ __forceinline__ bool q_from_map(float mx, float my, int& qx, int& qy)
{
    const float px = mx * 32.0f, py = my * 32.0f;
    // NaN, infinite or past int32: wholly outside (every comparison with a NaN is false)
    const bool fits = px >= -2147483648.0f && px < 2147483648.0f && py >= -2147483648.0f && py < 2147483648.0f;
    qx = (int)rintf(fits ? px : 0.0f);                                                        // round half to even
    qy = (int)rintf(fits ? py : 0.0f);
    return fits;
}
struct CoordMap {           // mav_remap: map_xy (H, W, 2)
    enum { LDS = 1 };
    const float* m; bool vec;
    __device__ void setup(const WarpArgs&, size_t, double*) const {}
    __device__ void bind(const WarpArgs& k, size_t img, const double*) { m = (const float*)k.a + img * k.W * k.H * 2; vec = ((uintptr_t)m & 7) == 0; }
    __device__ bool at(int, int, size_t p, int& qx, int& qy) const
    {
        float2 v;
        if (vec) v = *(const float2*)(m + 2 * p);
        else { v.x = m[2 * p]; v.y = m[2 * p + 1]; }
        return q_from_map(v.x, v.y, qx, qy);
    }
};
struct CoordPlanes {        // mav_remap_planes: map_x, map_y (H, W)
    enum { LDS = 1 };
    const float *mx, *my;
    __device__ void setup(const WarpArgs&, size_t, double*) const {}
    __device__ void bind(const WarpArgs& k, size_t img, const double*) { mx = (const float*)k.a + img * k.W * k.H; my = (const float*)k.b + img * k.W * k.H; }
    __device__ bool at(int, int, size_t p, int& qx, int& qy) const { return q_from_map(mx[p], my[p], qx, qy); }
};
struct CoordFlow {          // mav_warp_flow: grid - flow, generated here
    enum { LDS = 1 };
    const float* f; bool vec;
    __device__ void setup(const WarpArgs&, size_t, double*) const {}
    __device__ void bind(const WarpArgs& k, size_t img, const double*) { f = (const float*)k.a + img * k.W * k.H * 2; vec = ((uintptr_t)f & 7) == 0; }
    __device__ bool at(int x, int y, size_t p, int& qx, int& qy) const
    {
        float2 v;
        if (vec) v = *(const float2*)(f + 2 * p);
        else { v.x = f[2 * p]; v.y = f[2 * p + 1]; }
        return q_from_map((float)x + (-v.x), (float)y + (-v.y), qx, qy);
    }
};
// rint, half to even, saturated to int32; a NaN gives INT_MIN
__device__ __forceinline__ int sat_rint(double v)
{
    if (v != v) return INT_MIN;
    if (v >= 2147483647.0) return INT_MAX;
    if (v <= -2147483648.0) return INT_MIN;
    return (int)rint(v);
}
__device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
struct CoordAffine {        // mav_warp_affine: M (2, 3) double
    enum { LDS = 6 };
    const double* m;
    __device__ void setup(const WarpArgs& k, size_t img, double* lds) const
    {
        const double* M = (const double*)k.a + img * 6;
        double M0 = M[0], M1 = M[1], M2 = M[2], M3 = M[3], M4 = M[4], M5 = M[5];
        if (!(k.flags & MAV_WARP_INVERSE_MAP)) {
            double D = M0 * M4 - M1 * M3;
            D = D != 0 ? 1.0 / D : 0.0;
            const double A11 = M4 * D, A22 = M0 * D;
            M0 = A11; M1 = M1 * (-D); M3 = M3 * (-D); M4 = A22;
            const double b1 = (-M0) * M2 - M1 * M5, b2 = (-M3) * M2 - M4 * M5;
            M2 = b1; M5 = b2;
        }
        lds[0] = M0; lds[1] = M1; lds[2] = M2; lds[3] = M3; lds[4] = M4; lds[5] = M5;
    }
    __device__ void bind(const WarpArgs&, size_t, const double* lds) { m = lds; }
    __device__ bool at(int x, int y, size_t, int& qx, int& qy) const
    {
        const double dx = (double)x, dy = (double)y;
        const int X0 = wrap_add(sat_rint((m[1] * dy + m[2]) * 1024.0), 16), Y0 = wrap_add(sat_rint((m[4] * dy + m[5]) * 1024.0), 16);
        qx = wrap_add(X0, sat_rint((m[0] * dx) * 1024.0)) >> 5;
        qy = wrap_add(Y0, sat_rint((m[3] * dx) * 1024.0)) >> 5;
        return true;
    }
};
struct CoordPerspective {   // mav_warp_perspective: M (3, 3) double
    enum { LDS = 9 };
    const double* m;
    __device__ void setup(const WarpArgs& k, size_t img, double* lds) const
    {
        const double* M = (const double*)k.a + img * 9;
        if (k.flags & MAV_WARP_INVERSE_MAP) {
            for (int i = 0; i < 9; i++) lds[i] = M[i];
            return;
        }
        const double M0 = M[0], M1 = M[1], M2 = M[2], M3 = M[3], M4 = M[4], M5 = M[5], M6 = M[6], M7 = M[7], M8 = M[8];
        double d = (M0 * (M4 * M8 - M5 * M7) - M1 * (M3 * M8 - M5 * M6)) + M2 * (M3 * M7 - M4 * M6);
        d = d != 0 ? 1.0 / d : 0.0;
        lds[0] = (M4 * M8 - M5 * M7) * d; lds[1] = (M2 * M7 - M1 * M8) * d; lds[2] = (M1 * M5 - M2 * M4) * d;
        lds[3] = (M5 * M6 - M3 * M8) * d; lds[4] = (M0 * M8 - M2 * M6) * d; lds[5] = (M2 * M3 - M0 * M5) * d;
        lds[6] = (M3 * M7 - M4 * M6) * d; lds[7] = (M1 * M6 - M0 * M7) * d; lds[8] = (M0 * M4 - M1 * M3) * d;
    }
    __device__ void bind(const WarpArgs&, size_t, const double* lds) { m = lds; }
    __device__ bool at(int x, int y, size_t, int& qx, int& qy) const
    {
        const double dx = (double)x, dy = (double)y;
        double Wd = (m[6] * dx + m[7] * dy) + m[8];
        Wd = Wd != 0 ? 32.0 / Wd : 0.0;
        double fX = ((m[0] * dx + m[1] * dy) + m[2]) * Wd, fY = ((m[3] * dx + m[4] * dy) + m[5]) * Wd;
        const bool fits = fX == fX && fY == fY;
        fX = fX < -2147483648.0 ? -2147483648.0 : (fX > 2147483647.0 ? 2147483647.0 : fX);
        fY = fY < -2147483648.0 ? -2147483648.0 : (fY > 2147483647.0 ? 2147483647.0 : fY);
        qx = (int)rint(fits ? fX : 0.0);
        qy = (int)rint(fits ? fY : 0.0);
        return fits;
    }
};

// ---- the warp of a batch ---------------------------------------------------------------------------------------------------------------
template <typename P, int F>
__global__ __launch_bounds__(WARP_WG) void k_warp(const WarpArgs k)
{
    typedef typename WarpFmt<F>::T T;
    enum { C = WarpFmt<F>::C };
    __shared__ double lds[P::LDS];
    const size_t img = blockIdx.y, n0 = (size_t)k.W * k.H;
    P pol;
    if (threadIdx.x == 0) pol.setup(k, img, lds);
    __syncthreads();
    pol.bind(k, img, lds);
    const T* src = (const T*)k.src + img * n0 * C;
    T* dst = (T*)k.dst + img * n0 * C;
    const bool vec = F == MAV_WARP_F32C2 && ((uintptr_t)dst & 7) == 0;
    for (size_t p = (size_t)blockIdx.x * WARP_WG + threadIdx.x; p < n0; p += (size_t)gridDim.x * WARP_WG) {
        const int y = (int)((unsigned)p / (unsigned)k.W), x = (int)((unsigned)p - (unsigned)y * (unsigned)k.W);
        int qx, qy;
        const bool fits = pol.at(x, y, p, qx, qy);
        T o[C];
        warp_sample<F>(src, k.W, k.H, fits, qx, qy, o);
        if (vec) *(float2*)(dst + p * C) = make_float2((float)o[0], (float)o[C - 1]);
        else {
#pragma unroll
            for (int c = 0; c < C; c++) dst[p * C + c] = o[c];
        }
    }
}

// ---- Detector.warp_method: the matrix policies on F32C2 with subtraction, magnitude and argmax as the epilogue ------------------------
__device__ __forceinline__ unsigned long long warp_wave_max(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    return v;
}
// While a call runs, an image's record holds its key: (float bits of mag << 32) | ~pixel index -- the largest magnitude, the first pixel
// among equals (a magnitude is >= +0.0 or the quiet NaN, whose bits rank above every number's).  k_warp_key_init clears it, the warp
// raises it, k_warp_key_finish writes the record over it.
__global__ void k_warp_key_init(unsigned long long* key, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { key[2 * b] = 0ull; key[2 * b + 1] = 0ull; }
}
__global__ void k_warp_key_finish(unsigned long long* key, int B, int W)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long v = key[2 * b];
    const unsigned p = ~(unsigned)(v & 0xFFFFFFFFull);
    const unsigned row = p / (unsigned)W, col = p - row * (unsigned)W;
    key[2 * b] = (v >> 32) | ((unsigned long long)row << 32);          // max_mag, row
    key[2 * b + 1] = (unsigned long long)col;                          // col, pad = 0
}
template <typename P>
__global__ __launch_bounds__(WARP_WG) void k_warp_method(const WarpArgs k)
{
    __shared__ double lds[P::LDS];
    const size_t img = blockIdx.y, n0 = (size_t)k.W * k.H;
    P pol;
    if (threadIdx.x == 0) pol.setup(k, img, lds);
    __syncthreads();
    pol.bind(k, img, lds);
    const float* flow = (const float*)k.src + img * n0 * 2;
    float* diff = k.diff ? k.diff + img * n0 * 2 : nullptr;
    float* mag = k.mag ? k.mag + img * n0 : nullptr;
    const bool vin = ((uintptr_t)flow & 7) == 0, vout = ((uintptr_t)diff & 7) == 0;
    unsigned long long best = 0ull;
    for (size_t p = (size_t)blockIdx.x * WARP_WG + threadIdx.x; p < n0; p += (size_t)gridDim.x * WARP_WG) {
        const int y = (int)((unsigned)p / (unsigned)k.W), x = (int)((unsigned)p - (unsigned)y * (unsigned)k.W);
        int qx, qy;
        const bool fits = pol.at(x, y, p, qx, qy);
        float s[2];
        warp_sample<MAV_WARP_F32C2>(flow, k.W, k.H, fits, qx, qy, s);
        float2 f;
        if (vin) f = *(const float2*)(flow + 2 * p);
        else { f.x = flow[2 * p]; f.y = flow[2 * p + 1]; }
        // flow_uv[mask] = flow_uv_stable[mask], element-wise, then flow_uv - flow_uv_stable
        const float d0 = wcanon((s[0] == 0.0f ? s[0] : f.x) - s[0]), d1 = wcanon((s[1] == 0.0f ? s[1] : f.y) - s[1]);
        const float m = wcanon(sqrtf(d0 * d0 + d1 * d1));
        if (diff) {
            if (vout) *(float2*)(diff + 2 * p) = make_float2(d0, d1);
            else { diff[2 * p] = d0; diff[2 * p + 1] = d1; }
        }
        if (mag) mag[p] = m;
        const unsigned long long key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)~(unsigned)p;
        best = key > best ? key : best;
    }
    // one atomic per workgroup: the waves' maxima meet in LDS first (same-address atomics serialise in L2; measured, tools/warp_probe.py)
    __shared__ unsigned long long wave_best[WARP_WG / 64];
    best = warp_wave_max(best);
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WARP_WG / 64; w++) best = wave_best[w] > best ? wave_best[w] : best;
        if (best) atomicMax(&k.key[2 * img], best);
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------------------
static dim3 warp_grid(int W, int H, int B, size_t cap = WARP_CAP)
{
    const size_t need = ((size_t)W * H + WARP_WG - 1) / WARP_WG;
    return dim3((unsigned)(need < cap ? (need ? need : 1) : cap), (unsigned)B);
}
template <typename P>
static void launch_policy(hipStream_t st, int format, int B, const WarpArgs& k)
{
    const dim3 grid = warp_grid(k.W, k.H, B), block(WARP_WG);
    switch (format) {
    case MAV_WARP_U8C1: hipLaunchKernelGGL((k_warp<P, MAV_WARP_U8C1>), grid, block, 0, st, k); break;
    case MAV_WARP_U8C3: hipLaunchKernelGGL((k_warp<P, MAV_WARP_U8C3>), grid, block, 0, st, k); break;
    case MAV_WARP_F32C1: hipLaunchKernelGGL((k_warp<P, MAV_WARP_F32C1>), grid, block, 0, st, k); break;
    case MAV_WARP_F32C2: hipLaunchKernelGGL((k_warp<P, MAV_WARP_F32C2>), grid, block, 0, st, k); break;
    }
}
void launch_warp(hipStream_t st, int policy, int format, const void* src, const void* a, const void* b, int flags, int W, int H, int B, void* dst)
{
    WarpArgs k = {};
    k.src = src; k.dst = dst; k.a = a; k.b = b; k.W = W; k.H = H; k.flags = flags;
    switch (policy) {
    case WARP_POLICY_MAP: launch_policy<CoordMap>(st, format, B, k); break;
    case WARP_POLICY_PLANES: launch_policy<CoordPlanes>(st, format, B, k); break;
    case WARP_POLICY_FLOW: launch_policy<CoordFlow>(st, format, B, k); break;
    case WARP_POLICY_AFFINE: launch_policy<CoordAffine>(st, format, B, k); break;
    case WARP_POLICY_PERSPECTIVE: launch_policy<CoordPerspective>(st, format, B, k); break;
    }
}
void launch_warp_method(hipStream_t st, int policy, const float* flow, const double* M, int W, int H, int B, float* diff, float* mag, void* records)
{
    WarpArgs k = {};
    k.src = flow; k.a = M; k.W = W; k.H = H; k.flags = 0; k.diff = diff; k.mag = mag; k.key = (unsigned long long*)records;
    const dim3 one((B + 63) / 64), lanes(64);
    hipLaunchKernelGGL(k_warp_key_init, one, lanes, 0, st, k.key, B);
    if (policy == WARP_POLICY_AFFINE) hipLaunchKernelGGL(k_warp_method<CoordAffine>, warp_grid(W, H, B, WARP_METHOD_CAP), dim3(WARP_WG), 0, st, k);
    else hipLaunchKernelGGL(k_warp_method<CoordPerspective>, warp_grid(W, H, B, WARP_METHOD_CAP), dim3(WARP_WG), 0, st, k);
    hipLaunchKernelGGL(k_warp_key_finish, one, lanes, 0, st, k.key, B, W);
}

// Flow history (Detector.get_history, detector.py:365-388): cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) of a 2-channel field, restated
// from OpenCV 4.x, and the trajectory every pixel takes through the ring's fields by chained remaps -- one kernel, nothing intermediate
// written.  Compiled with -ffp-contract=off: tests/history_ref.py restates every operation of this file in numpy in the same order, and
// the tests compare bytes.
#include <type_traits>

#include "mavflow_internal.h"

#define HIST_WG 256     // threads of a workgroup of every kernel here
// Pixels per thread and grid cap of the trajectory kernel, measured (DESIGN.md section 4g has the table; A/B builds override them
// for tools/history_probe.py --lib): one chain per thread is the fastest form at both frame sizes, occupancy alone hides the gathers.
#ifndef HIST_PX
#define HIST_PX 1       // pixels a thread of the trajectory kernel owns, HIST_WG apart (lane-contiguous loads): independent chains
#endif
#ifndef HIST_CAP
#define HIST_CAP 4096   // most workgroups of a launch; the rest of the frame is reached by the grid-stride loop
#endif

template <typename T> struct Pair2;
template <> struct Pair2<float> { typedef float2 type; };
template <> struct Pair2<double> { typedef double2 type; };

static int history_blocks(size_t items)
{
    const size_t need = (items + HIST_WG - 1) / HIST_WG;
    return (int)(need < HIST_CAP ? (need ? need : 1) : HIST_CAP);
}

// A NaN leaves as THE quiet NaN: which payload and sign an invalid operation or a NaN operand produces differs between this GPU and
// the host that runs the numpy restatement, whether a value is a NaN does not.
__device__ __forceinline__ double canon(double v) { return v != v ? __longlong_as_double(0x7FF8000000000000LL) : v; }
__device__ __forceinline__ float canon(float v) { return v != v ? __int_as_float(0x7FC00000) : v; }

// One output element of remap(src, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0) for a W x H field of (u, v) pairs: the five steps
// of include/mavflow.h (mav_stage_remap_linear).  Branch-free: the four taps are always loaded, from clamped (in-range) positions, and
// a tap that is out of range enters the sum as 0.0 -- so that the two chains of a thread keep their loads in flight side by side.
// All four products are always formed: an in-range NaN tap under a zero weight gives NaN, as cv2's interior path does.
template <typename T>
__device__ __forceinline__ void remap_linear_px(const typename Pair2<T>::type* __restrict__ src, int W, int H, float mx, float my, double& o0,
                                                double& o1)
{
    const float px = mx * 32.0f, py = my * 32.0f;
    // NaN, infinite or past int32: wholly outside (every comparison with a NaN is false)
    const bool fits = px >= -2147483648.0f && px < 2147483648.0f && py >= -2147483648.0f && py < 2147483648.0f;
    const int qx = (int)rintf(fits ? px : 0.0f), qy = (int)rintf(fits ? py : 0.0f);          // round half to even
    int sx = qx >> 5, sy = qy >> 5;                                                           // arithmetic shifts
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
    sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
    const float fx = (float)(qx & 31) * 0.03125f, fy = (float)(qy & 31) * 0.03125f;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const double w00 = (double)(gy * gx), w01 = (double)(gy * fx), w10 = (double)(fy * gx), w11 = (double)(fy * fx);   // multiples of 1/1024
    const bool inside = fits && !(sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0);
    const bool xa = sx >= 0, xb = sx + 1 < W, ya = sy >= 0, yb = sy + 1 < H;                  // (sx < W, sx + 1 >= 0 where `inside`)
    const int cxa = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx), cxb = sx + 1 < 0 ? 0 : (sx + 1 > W - 1 ? W - 1 : sx + 1);
    const int cya = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy), cyb = sy + 1 < 0 ? 0 : (sy + 1 > H - 1 ? H - 1 : sy + 1);
    const size_t ra = (size_t)cya * W, rb = (size_t)cyb * W;
    const typename Pair2<T>::type a = src[ra + cxa], b = src[ra + cxb], c = src[rb + cxa], d = src[rb + cxb];
    const bool va = inside && ya && xa, vb = inside && ya && xb, vc = inside && yb && xa, vd = inside && yb && xb;
    const double a0 = va ? (double)a.x : 0.0, b0 = vb ? (double)b.x : 0.0, c0 = vc ? (double)c.x : 0.0, d0 = vd ? (double)d.x : 0.0;
    const double a1 = va ? (double)a.y : 0.0, b1 = vb ? (double)b.y : 0.0, c1 = vc ? (double)c.y : 0.0, d1 = vd ? (double)d.y : 0.0;
    o0 = ((a0 * w00 + b0 * w01) + c0 * w10) + d0 * w11;         // wholly outside: every tap is 0.0 and the sum is +0.0
    o1 = ((a1 * w00 + b1 * w01) + c1 * w10) + d1 * w11;
}

// ---- one remap of a whole field (mav_stage_remap_linear: the stage-level pin) ------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(HIST_WG) void k_remap_linear(const T* __restrict__ src, const float* __restrict__ map_x, const float* __restrict__ map_y,
                                                          int W, int H, double* __restrict__ out)
{
    const size_t n0 = (size_t)W * H;
    for (size_t p = (size_t)blockIdx.x * HIST_WG + threadIdx.x; p < n0; p += (size_t)gridDim.x * HIST_WG) {
        double u, v;
        remap_linear_px<T>((const typename Pair2<T>::type*)src, W, H, map_x[p], map_y[p], u, v);
        out[2 * p] = canon(u);
        out[2 * p + 1] = canon(v);
    }
}
void launch_remap_linear(hipStream_t st, const void* src, bool f64, const float* map_x, const float* map_y, int W, int H, double* out)
{
    const dim3 grid(history_blocks((size_t)W * H)), block(HIST_WG);
    if (f64) hipLaunchKernelGGL(k_remap_linear<double>, grid, block, 0, st, (const double*)src, map_x, map_y, W, H, out);
    else hipLaunchKernelGGL(k_remap_linear<float>, grid, block, 0, st, (const float*)src, map_x, map_y, W, H, out);
}

// ---- the ring write: a caller's field -> a slot, copied or widened -----------------------------------------------------------------
// One pixel (two elements) per thread and iteration; the caller's pointer is aligned to its element only, so the pair is loaded as one
// access where the pointer allows it and as two otherwise.  The slot is the library's own memory: always aligned to a pair.
template <typename S, typename D>
__global__ __launch_bounds__(HIST_WG) void k_history_put(const S* __restrict__ src, D* __restrict__ dst, size_t n0)
{
    const bool vec = ((uintptr_t)src & (2 * sizeof(S) - 1)) == 0;
    for (size_t p = (size_t)blockIdx.x * HIST_WG + threadIdx.x; p < n0; p += (size_t)gridDim.x * HIST_WG) {
        typename Pair2<S>::type s;
        if (vec) s = ((const typename Pair2<S>::type*)src)[p];
        else { s.x = src[2 * p]; s.y = src[2 * p + 1]; }
        typename Pair2<D>::type d;
        d.x = (D)s.x; d.y = (D)s.y;
        ((typename Pair2<D>::type*)dst)[p] = d;
    }
}
void launch_history_put(hipStream_t st, const void* src, bool src_f64, void* slot, bool ring_f64, int W, int H)
{
    const size_t n0 = (size_t)W * H;
    const dim3 grid(history_blocks(n0)), block(HIST_WG);
    if (src_f64) hipLaunchKernelGGL((k_history_put<double, double>), grid, block, 0, st, (const double*)src, (double*)slot, n0);      // (the host refuses float64 into a float32 ring)
    else if (ring_f64) hipLaunchKernelGGL((k_history_put<float, double>), grid, block, 0, st, (const float*)src, (double*)slot, n0);
    else hipLaunchKernelGGL((k_history_put<float, float>), grid, block, 0, st, (const float*)src, (float*)slot, n0);
}

// ---- the trajectories --------------------------------------------------------------------------------------------------------------
// Every pixel (y, x) starts at r = y, c = x (double) and, for each slot of the list in turn, adds the field's value at its float32
// position: (u, v) = remap(ring[slot], (float)c, (float)r); r += u, c += v -- the reference's channel order (lookup_map[..., 0] is the
// row and receives the flow's x component) -- or, with XY, r += v, c += u.  A pixel's chain is a sequence of dependent gathers; a thread
// walks HIST_PX chains side by side (one, as measured) and the latency is hidden by occupancy.  No LDS: neighbouring trajectories stay
// neighbours, a wave's taps of one step fall into a few cache lines.  Out: float64 (r - y, c - x), or, with F32, float32
// (c - x, r - y) rounded once each -- the (u, v) layout of the detection stage.
template <typename T, bool XY, bool F32>
__global__ __launch_bounds__(HIST_WG) void k_history_trace(const T* __restrict__ ring, HistSlots slots, int W, int H, void* __restrict__ out)
{
    typedef typename Pair2<T>::type P;
    typedef typename std::conditional<F32, float, double>::type E;
    typedef typename Pair2<E>::type O;
    const size_t n0 = (size_t)W * H, chunk = (size_t)HIST_WG * HIST_PX;
    const bool vec = ((uintptr_t)out & (sizeof(O) - 1)) == 0;
    for (size_t base = (size_t)blockIdx.x * chunk + threadIdx.x; base < n0; base += (size_t)gridDim.x * chunk) {
        size_t p[HIST_PX];
        double y[HIST_PX], x[HIST_PX], r[HIST_PX], c[HIST_PX];
#pragma unroll
        for (int i = 0; i < HIST_PX; i++) {
            p[i] = base + (size_t)i * HIST_WG < n0 ? base + (size_t)i * HIST_WG : n0 - 1;      // past the frame's end: the last pixel again, not stored
            const size_t yi = p[i] / (size_t)W;
            r[i] = y[i] = (double)yi;
            c[i] = x[i] = (double)(p[i] - yi * W);
        }
        for (int k = 0; k < slots.n; k++) {
            const unsigned slot = (slots.w[k >> 2] >> ((k & 3) * 8)) & 255u;
            const P* f = (const P*)ring + (size_t)slot * n0;
            double u[HIST_PX], v[HIST_PX];
#pragma unroll
            for (int i = 0; i < HIST_PX; i++) remap_linear_px<T>(f, W, H, (float)c[i], (float)r[i], u[i], v[i]);
#pragma unroll
            for (int i = 0; i < HIST_PX; i++) {
                r[i] = r[i] + (XY ? v[i] : u[i]);
                c[i] = c[i] + (XY ? u[i] : v[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < HIST_PX; i++) {
            if (base + (size_t)i * HIST_WG >= n0) break;
            const double dr = r[i] - y[i], dc = c[i] - x[i];
            O o;
            if (F32) { o.x = canon((float)dc); o.y = canon((float)dr); }
            else { o.x = canon(dr); o.y = canon(dc); }
            if (vec) ((O*)out)[p[i]] = o;
            else { ((E*)out)[2 * p[i]] = o.x; ((E*)out)[2 * p[i] + 1] = o.y; }
        }
    }
}
template <typename T>
static void launch_trace_t(hipStream_t st, const T* ring, const HistSlots& slots, int W, int H, bool xy, bool f32, void* out)
{
    const dim3 grid(history_blocks(((size_t)W * H + HIST_PX - 1) / HIST_PX)), block(HIST_WG);        // (a workgroup takes HIST_WG * HIST_PX pixels per step)
    if (xy && f32) hipLaunchKernelGGL((k_history_trace<T, true, true>), grid, block, 0, st, ring, slots, W, H, out);
    else if (xy) hipLaunchKernelGGL((k_history_trace<T, true, false>), grid, block, 0, st, ring, slots, W, H, out);
    else if (f32) hipLaunchKernelGGL((k_history_trace<T, false, true>), grid, block, 0, st, ring, slots, W, H, out);
    else hipLaunchKernelGGL((k_history_trace<T, false, false>), grid, block, 0, st, ring, slots, W, H, out);
}
void launch_history_trace(hipStream_t st, const void* ring, bool ring_f64, const HistSlots& slots, int W, int H, bool axes_xy, bool out_f32, void* out)
{
    if (ring_f64) launch_trace_t<double>(st, (const double*)ring, slots, W, H, axes_xy, out_f32, out);
    else launch_trace_t<float>(st, (const float*)ring, slots, W, H, axes_xy, out_f32, out);
}

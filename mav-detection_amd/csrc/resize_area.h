// cv2.resize(INTER_AREA), non-integer ratio: computeResizeAreaTab + resizeArea_<T, float> (resize.cpp), one destination element at a time.
// Shared by kernels_window.hip (the pyramid of analyze_pyramid, the initial flow of OPTFLOW_USE_INITIAL_FLOW) and kernels_resize.hip
// (include/mavflow_resize.h); both are compiled with -ffp-contract=off: the sums accumulate in float in OpenCV's tap order.
#ifndef MAVFLOW_RESIZE_AREA_H
#define MAVFLOW_RESIZE_AREA_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

// One destination index d of one axis covers source cells [d*scale, d*scale + scale): an optional partial first cell
// (s1 - 1, weight wf), whole cells s1 .. s2-1 (weight wm each) and an optional partial last cell (s2, weight wl).
struct AreaSpan { int s1, s2; float wf, wm, wl; bool first, last; };
__device__ __forceinline__ AreaSpan area_span(int d, double scale, int ssize)
{
    AreaSpan a;
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)ssize - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < ssize - 1 ? s2 : ssize - 1;
    s1 = s1 < s2 ? s1 : s2;
    a.s1 = s1; a.s2 = s2;
    a.first = (double)s1 - f1 > 1e-3;
    a.last = f2 - (double)s2 > 1e-3;
    a.wf = (float)(((double)s1 - f1) / cell);
    a.wm = (float)(1.0 / cell);
    a.wl = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
    return a;
}
// channel c of one source row of CN interleaved channels (resizeArea_ keeps one float accumulator per channel: the same sum per channel)
template <int CN, typename T>
__device__ __forceinline__ float area_row(const T* __restrict__ S, const AreaSpan& x, int c = 0)
{
    float buf = 0.f;                                   // buf[dx] += S[si] * alpha, in tab order
    if (x.first) buf = buf + (float)S[(size_t)(x.s1 - 1) * CN + c] * x.wf;
    for (int sx = x.s1; sx < x.s2; sx++) buf = buf + (float)S[(size_t)sx * CN + c] * x.wm;
    if (x.last) buf = buf + (float)S[(size_t)x.s2 * CN + c] * x.wl;
    return buf;
}
// rows in tab order: sum[dx] += beta * buf[dx]; S = channel plane origin, row pitch sw * CN elements
template <int CN, typename T>
__device__ __forceinline__ float area_general(const T* __restrict__ S, int sw, const AreaSpan& x, const AreaSpan& y, int c = 0)
{
    const size_t pitch = (size_t)sw * CN;
    float sum = 0.f;
    if (y.first) sum = sum + y.wf * area_row<CN>(S + (size_t)(y.s1 - 1) * pitch, x, c);
    for (int sy = y.s1; sy < y.s2; sy++) sum = sum + y.wm * area_row<CN>(S + (size_t)sy * pitch, x, c);
    if (y.last) sum = sum + y.wl * area_row<CN>(S + (size_t)y.s2 * pitch, x, c);
    return sum;
}
// the float sum of the fast form (both ratios whole numbers ix, iy): resizeAreaFast_<float, float>'s scalar loop -- the iy x ix block in
// ofs order (rows, then columns), grouped four at a time as the unrolled loop adds them (sum += ((a + b) + c) + d), times 1.f / area.
// B: the block's first element of channel c; CN interleaved channels, row pitch sw * CN elements.
template <int CN>
__device__ __forceinline__ float area_fast_f32(const float* __restrict__ B, int sw, int ix, int iy)
{
    const int area = ix * iy;
    const float inv = 1.f / (float)area;
    auto at = [&](int k) { return B[((size_t)(k / ix) * sw + (k % ix)) * CN]; };
    float sum = 0.f;
    int k = 0;
    for (; k <= area - 4; k += 4) sum = sum + (((at(k) + at(k + 1)) + at(k + 2)) + at(k + 3));
    for (; k < area; k++) sum = sum + at(k);
    return sum * inv;
}
#endif

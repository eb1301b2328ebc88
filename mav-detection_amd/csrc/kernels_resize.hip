// Image resize (include/mavflow_resize.h, whose text is the definition): cv2.resize with INTER_NEAREST, INTER_LINEAR and INTER_AREA
// (shrinking) on the four pixel formats of the warps, and the sky mask of a prediction (resize + key) in one pass.
// gfx950, wave64.  Compiled with -ffp-contract=off: every float32 product and sum is rounded on its own, in the header's order.
//
// One body, k_resize<format, form, vector stores, sky>: a workgroup of 256 covers 4 destination rows x 64 threads, blockIdx.z is the
// image.  A thread owns PX consecutive destination pixels of one row (4; 2 for F32C2) and keeps them in registers; with VEC they leave
// as one dword (U8C1, the sky mask), three dwords (U8C3) or 16 bytes (F32C1, F32C2), which needs dw % PX == 0 and an aligned dst --
// otherwise the scalar form stores element by element and covers the ragged tail.  The per-axis table values (s and a of LINEAR, the
// span of AREA) are computed in registers from d and the double scale: no table in memory, nothing allocated.  A memory-bound pass:
// neighbouring lanes' taps fall into the same cache lines, the source is read through the caches, no LDS.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mavflow_internal.h"
#include "resize_area.h"
#include "../../include/mavflow_resize.h"

template <int FMT> struct RsFmt;
template <> struct RsFmt<MAV_WARP_U8C1>  { typedef uint8_t T; enum { CN = 1, PX = 4 }; };
template <> struct RsFmt<MAV_WARP_U8C3>  { typedef uint8_t T; enum { CN = 3, PX = 4 }; };
template <> struct RsFmt<MAV_WARP_F32C1> { typedef float T;   enum { CN = 1, PX = 4 }; };
template <> struct RsFmt<MAV_WARP_F32C2> { typedef float T;   enum { CN = 2, PX = 2 }; };

// what one launch works on: src (B, sh, sw, CN), dst (B, dh, dw, CN) or the sky mask (B, dh, dw) uint8
struct RsCall { const void* src; void* dst; int sw, sh, dw, dh; double scale_x, scale_y; int ix, iy, key0, key1; };

// an element as the 32 bits a register keeps: a byte's value, a float's bits (a copy moves a NaN's payload)
__device__ __forceinline__ uint32_t rs_raw(const uint8_t* p) { return *p; }
__device__ __forceinline__ uint32_t rs_raw(const float* p) { return *(const uint32_t*)p; }
__device__ __forceinline__ uint32_t rs_f32(float v) { return v != v ? 0x7FC00000u : __float_as_uint(v); }
__device__ __forceinline__ uint32_t rs_u8(float sum)            // saturate_cast<uchar>(float): round half to even, clamp
{
    const float r = rintf(sum);
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// LINEAR's table of one axis
struct LinTab { int s; float a; bool one; };
__device__ __forceinline__ LinTab lin_tab(int d, double scale, int ssize)
{
    LinTab t;
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    float a = f - (float)s;
    if (s < 0) { s = 0; a = 0.f; }
    t.one = s >= ssize - 1;
    if (t.one) { s = ssize - 1; a = 0.f; }
    t.s = s; t.a = a;
    return t;
}
__device__ __forceinline__ int lin_coef(float c)                // round_half_even(c * 2048.f), saturated to int16
{
    const float r = rintf(c * 2048.f);
    return (int)(r > 32767.f ? 32767.f : (r < -32768.f ? -32768.f : r));
}
__device__ __forceinline__ int nearest_index(int d, double scale, int ssize)
{
    const int s = (int)floor((double)d * scale);
    return s < ssize - 1 ? s : ssize - 1;
}

template <int FMT, int FORM, bool VEC, bool SKY>
__global__ __launch_bounds__(256) void k_resize(const RsCall k)
{
    typedef typename RsFmt<FMT>::T T;
    constexpr int CN = RsFmt<FMT>::CN, PX = RsFmt<FMT>::PX, CU = SKY ? 2 : CN;      // the sky key reads channels 0 and 1 alone
    constexpr bool F32 = sizeof(T) == 4;
    const int dx0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * PX, dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx0 >= k.dw || dy >= k.dh) return;
    const size_t pitch = (size_t)k.sw * CN;
    const T* __restrict__ S = (const T*)k.src + (size_t)blockIdx.z * k.sh * pitch;
    uint32_t v[PX * CN];
#pragma unroll
    for (int i = 0; i < PX * CN; i++) v[i] = 0;

    // what the row decides, once for the thread's pixels
    const T *row0 = S, *row1 = S;
    float b = 0.f;
    int b0 = 0, b1 = 0;
    AreaSpan ys = {};
    if constexpr (FORM == RS_COPY) row0 = S + (size_t)dy * pitch;
    if constexpr (FORM == RS_NEAREST) row0 = S + (size_t)nearest_index(dy, k.scale_y, k.sh) * pitch;
    if constexpr (FORM == RS_LINEAR) {
        const LinTab y = lin_tab(dy, k.scale_y, k.sh);
        row0 = S + (size_t)y.s * pitch;
        row1 = S + (size_t)(y.s + 1 < k.sh ? y.s + 1 : k.sh - 1) * pitch;
        b = y.a;
        b0 = lin_coef(1.f - b); b1 = lin_coef(b);
    }
    if constexpr (FORM == RS_AREA_2X2) { row0 = S + (size_t)(2 * dy) * pitch; row1 = row0 + pitch; }
    if constexpr (FORM == RS_AREA_FAST) row0 = S + (size_t)dy * k.iy * pitch;
    if constexpr (FORM == RS_AREA_GENERAL) ys = area_span(dy, k.scale_y, k.sh);

#pragma unroll
    for (int p = 0; p < PX; p++) {
        const int dx = dx0 + p;
        if (VEC || dx < k.dw) {
            if constexpr (FORM == RS_COPY || FORM == RS_NEAREST) {
                const int sx = FORM == RS_COPY ? dx : nearest_index(dx, k.scale_x, k.sw);
#pragma unroll
                for (int c = 0; c < CU; c++) v[p * CN + c] = rs_raw(row0 + (size_t)sx * CN + c);
            } else if constexpr (FORM == RS_LINEAR) {
                const LinTab x = lin_tab(dx, k.scale_x, k.sw);
                const T *p0 = row0 + (size_t)x.s * CN, *p1 = row1 + (size_t)x.s * CN;
                if constexpr (F32) {
                    const float a = x.a;
#pragma unroll
                    for (int c = 0; c < CU; c++) {
                        float h0, h1;
                        if (x.one) { h0 = p0[c] * 1.f; h1 = p1[c] * 1.f; }
                        else { h0 = p0[c] * (1.f - a) + p0[CN + c] * a; h1 = p1[c] * (1.f - a) + p1[CN + c] * a; }
                        v[p * CN + c] = rs_f32(h0 * (1.f - b) + h1 * b);
                    }
                } else {
                    const int a0 = lin_coef(1.f - x.a), a1 = lin_coef(x.a);
#pragma unroll
                    for (int c = 0; c < CU; c++) {
                        int h0, h1;
                        if (x.one) { h0 = (int)p0[c] * 2048; h1 = (int)p1[c] * 2048; }
                        else { h0 = (int)p0[c] * a0 + (int)p0[CN + c] * a1; h1 = (int)p1[c] * a0 + (int)p1[CN + c] * a1; }
                        // clamp(q >> 2, 0, 255) == clamp(q, 0, 1023) >> 2.  Written in the second way on purpose: in the first the
                        // compiler packs two results with v_ashr_pk_u8_i32 and takes the upper half of its destination for zero,
                        // which the MI355X does not write (measured: stale bytes in the third dword of a U8C3 group).
                        const int q = ((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2;
                        v[p * CN + c] = (uint32_t)(q < 0 ? 0 : (q > 1023 ? 1023 : q)) >> 2;
                    }
                }
            } else if constexpr (FORM == RS_AREA_2X2) {          // uint8 alone: rounds a half UP
                const T *p0 = row0 + (size_t)(2 * dx) * CN, *p1 = row1 + (size_t)(2 * dx) * CN;
#pragma unroll
                for (int c = 0; c < CU; c++) v[p * CN + c] = ((uint32_t)p0[c] + p0[CN + c] + p1[c] + p1[CN + c] + 2u) >> 2;
            } else if constexpr (FORM == RS_AREA_FAST) {
                const T* B = row0 + (size_t)dx * k.ix * CN;
#pragma unroll
                for (int c = 0; c < CU; c++) {
                    if constexpr (F32) {
                        v[p * CN + c] = rs_f32(area_fast_f32<CN>((const float*)B + c, k.sw, k.ix, k.iy));
                    } else {
                        int sum = 0;
                        for (int r = 0; r < k.iy; r++)
                            for (int q = 0; q < k.ix; q++) sum += (int)B[(size_t)r * pitch + (size_t)q * CN + c];
                        v[p * CN + c] = rs_u8((float)sum * (1.f / (float)(k.ix * k.iy)));
                    }
                }
            } else {
                const AreaSpan xs = area_span(dx, k.scale_x, k.sw);
#pragma unroll
                for (int c = 0; c < CU; c++) {
                    const float sum = area_general<CN>(S, k.sw, xs, ys, c);
                    v[p * CN + c] = F32 ? rs_f32(sum) : rs_u8(sum);
                }
            }
        }
    }

    // the thread's pixels leave
    const size_t at = ((size_t)blockIdx.z * k.dh + dy) * k.dw + dx0;             // in pixels
    if constexpr (SKY) {
        uint32_t m[PX];
#pragma unroll
        for (int p = 0; p < PX; p++) m[p] = (v[p * CN] == (uint32_t)k.key0 && v[p * CN + 1] == (uint32_t)k.key1) ? 1u : 0u;
        uint8_t* D = (uint8_t*)k.dst + at;
        if constexpr (VEC) *(uint32_t*)D = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        else {
#pragma unroll
            for (int p = 0; p < PX; p++) if (dx0 + p < k.dw) D[p] = (uint8_t)m[p];
        }
    } else if constexpr (VEC) {
        if constexpr (F32) {
            *(uint4*)((uint32_t*)k.dst + at * CN) = make_uint4(v[0], v[1], v[2], v[3]);       // PX * CN == 4
        } else {
            uint32_t* D = (uint32_t*)((uint8_t*)k.dst + at * CN);
#pragma unroll
            for (int j = 0; j < CN; j++) D[j] = v[4 * j] | (v[4 * j + 1] << 8) | (v[4 * j + 2] << 16) | (v[4 * j + 3] << 24);
        }
    } else {
#pragma unroll
        for (int p = 0; p < PX; p++) {
            if (dx0 + p < k.dw) {
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    if constexpr (F32) ((uint32_t*)k.dst)[(at + p) * CN + c] = v[p * CN + c];
                    else ((uint8_t*)k.dst)[(at + p) * CN + c] = (uint8_t)v[p * CN + c];
                }
            }
        }
    }
}

template <int FMT, bool SKY>
static void launch_fmt(hipStream_t st, int form, bool vec, int B, const RsCall& k)
{
    constexpr int PX = RsFmt<FMT>::PX;
    const dim3 grid(((k.dw + PX - 1) / PX + 63) / 64, (k.dh + 3) / 4, B), block(256);
#define RS_GO(FORM)                                                                                  \
    do {                                                                                             \
        if (vec) hipLaunchKernelGGL((k_resize<FMT, FORM, true, SKY>), grid, block, 0, st, k);        \
        else hipLaunchKernelGGL((k_resize<FMT, FORM, false, SKY>), grid, block, 0, st, k);           \
    } while (0)
    constexpr bool u8 = sizeof(typename RsFmt<FMT>::T) == 1;
    if (form == RS_COPY) RS_GO(RS_COPY);
    else if (form == RS_LINEAR) RS_GO(RS_LINEAR);
    else if (form == RS_AREA_2X2) { if constexpr (u8) RS_GO(RS_AREA_2X2); }
    else if constexpr (!SKY) {
        if (form == RS_NEAREST) RS_GO(RS_NEAREST);
        else if (form == RS_AREA_FAST) RS_GO(RS_AREA_FAST);
        else RS_GO(RS_AREA_GENERAL);
    }
#undef RS_GO
}

// cv::resize's dispatch, in the header's order
int resize_form(int format, int sw, int sh, int dw, int dh, int interpolation, int* ix, int* iy)
{
    const double scale_x = (double)sw / dw, scale_y = (double)sh / dh;
    *ix = (int)nearbyint(scale_x); *iy = (int)nearbyint(scale_y);
    if (dw == sw && dh == sh) return RS_COPY;
    if (interpolation == MAV_INTER_LINEAR && fabs(scale_x - 2.0) < DBL_EPSILON && fabs(scale_y - 2.0) < DBL_EPSILON) interpolation = MAV_INTER_AREA;
    if (interpolation == MAV_INTER_NEAREST) return RS_NEAREST;
    if (interpolation == MAV_INTER_LINEAR) return RS_LINEAR;
    if (!(fabs(scale_x - *ix) < DBL_EPSILON && fabs(scale_y - *iy) < DBL_EPSILON)) return RS_AREA_GENERAL;
    const bool u8 = format == MAV_WARP_U8C1 || format == MAV_WARP_U8C3;
    return u8 && *ix == 2 && *iy == 2 ? RS_AREA_2X2 : RS_AREA_FAST;
}
// the vector-store form: the destination's rows all begin on the store's boundary
bool resize_vector_stores(int format, int dw, const void* dst, bool sky)
{
    if (sky || format == MAV_WARP_U8C1 || format == MAV_WARP_U8C3) return dw % 4 == 0 && (uintptr_t)dst % 4 == 0;
    return dw % (format == MAV_WARP_F32C2 ? 2 : 4) == 0 && (uintptr_t)dst % 16 == 0;
}

void launch_resize(hipStream_t st, int format, const void* src, int sw, int sh, int dw, int dh, int interpolation, int B, void* dst)
{
    RsCall k = {src, dst, sw, sh, dw, dh, (double)sw / dw, (double)sh / dh, 1, 1, 0, 0};
    const int form = resize_form(format, sw, sh, dw, dh, interpolation, &k.ix, &k.iy);
    const bool vec = resize_vector_stores(format, dw, dst, false);
    switch (format) {
    case MAV_WARP_U8C1: launch_fmt<MAV_WARP_U8C1, false>(st, form, vec, B, k); break;
    case MAV_WARP_U8C3: launch_fmt<MAV_WARP_U8C3, false>(st, form, vec, B, k); break;
    case MAV_WARP_F32C1: launch_fmt<MAV_WARP_F32C1, false>(st, form, vec, B, k); break;
    default: launch_fmt<MAV_WARP_F32C2, false>(st, form, vec, B, k); break;
    }
}

void launch_sky_mask(hipStream_t st, const uint8_t* pred_bgr, int sw, int sh, int dw, int dh, int key0, int key1, int B, uint8_t* sky)
{
    RsCall k = {pred_bgr, sky, sw, sh, dw, dh, (double)sw / dw, (double)sh / dh, 1, 1, key0, key1};
    const int form = resize_form(MAV_WARP_U8C3, sw, sh, dw, dh, MAV_INTER_LINEAR, &k.ix, &k.iy);
    launch_fmt<MAV_WARP_U8C3, true>(st, form, resize_vector_stores(MAV_WARP_U8C3, dw, sky, true), B, k);
}

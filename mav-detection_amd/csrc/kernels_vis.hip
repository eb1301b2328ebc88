// Flow pictures (include/mavflow_vis.h, whose text is the definition): the HSV picture of a flow field in the two forms the reference's
// Farneback class has (process(), draw_hsv), cv2.cvtColor's COLOR_HSV2BGR and COLOR_BGR2HSV on uint8 x 3, and draw_flow's line field.
// gfx950, wave64.  Compiled with -ffp-contract=off: every float32 product and sum is rounded on its own; float32 '/' and sqrtf are the
// correctly rounded ones (the toolchain's default, which the build leaves on), so everything but atan2f is IEEE arithmetic in a fixed
// order and equals numpy's bits.
//
// The pixel passes work FLAT over the B * H * W pixels of a call: no mode depends on a pixel's position, only (MAV_HSV_PROCESS) on its
// image's minimum and maximum.  One thread owns a GROUP of 16 consecutive pixels -- 8 x 16 bytes of flow in, 3 x 16 bytes of picture out --
// where the caller's pointers are aligned to 16 (vis_form: the FAST form); the N % 16 pixels behind the last group, and every pixel of a
// call whose pointers are not aligned (the BYTES form), are taken one per thread with byte stores, by further threads of the same launch.
// A group may straddle two images (n0 % 16 != 0): the image is tracked per pixel.
//
// MAV_HSV_PROCESS is three launches: k_hsv_record_init sets the caller's record block, k_flow_minmax reduces each image's magnitude bits
// into it (wave shuffle, then LDS, then one atomicMin / atomicMax per workgroup; a workgroup whose pixels lie in two images falls back to
// per-thread atomics), k_flow_hsv renders and counts.  The record block IS the scratch: the context holds no memory for these calls.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mavflow_internal.h"
#include "../../include/mavflow_vis.h"

#define VIS_WG 256
#define VIS_GROUP 16

static_assert(sizeof(mav_hsv_record) == 16, "mav_hsv_record");

// np.float32(np.pi), np.float32(2 * np.pi), np.float32(180 / np.pi / 2), np.float32(6.0 / 180.0)
#define VIS_PI 3.14159274101257324f
#define VIS_2PI 6.28318548202514648f
static constexpr float VIS_HALF_DEG = (float)(180.0 / 3.14159265358979323846 / 2.0);
static constexpr float VIS_H6 = (float)(6.0 / 180.0);

// ---- COLOR_HSV2BGR on one uint8 triple: mavflow.farneback.hsv_to_bgr, operation for operation.  Returns b | g << 8 | r << 16. ------------
__device__ __forceinline__ uint32_t vis_u8(float x)                    // clip(rint(x * 255.0), 0, 255)
{
    const float r = rintf(x * 255.0f);
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}
__device__ __forceinline__ uint32_t vis_hsv2bgr(uint32_t h8, uint32_t s8, uint32_t v8)
{
    const float h = (float)h8 * VIS_H6;
    const float s = (float)s8 / 255.0f, v = (float)v8 / 255.0f;
    const float sec = floorf(h), f = h - sec;
    const int sector = (int)sec % 6;                                    // h8 <= 255: sec in 0 .. 8
    const float t1 = v * (1.f - s), t2 = v * (1.f - s * f), t3 = v * (1.f - s * (1.f - f));
    float b, g, r;
    switch (sector) {
    case 0: b = t1; g = t3; r = v; break;
    case 1: b = t1; g = v; r = t2; break;
    case 2: b = t3; g = v; r = t1; break;
    case 3: b = v; g = t2; r = t1; break;
    case 4: b = v; g = t1; r = t3; break;
    default: b = t2; g = t1; r = v; break;
    }
    return vis_u8(b) | (vis_u8(g) << 8) | (vis_u8(r) << 16);
}

// ---- COLOR_BGR2HSV on one uint8 triple: OpenCV's integer path (hsv_shift = 12, hue range 180).  The tables are built by the host
// compiler in double: sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)), entry 0 = 0.  No quotient is a tie
// (2 * 255 * 4096 / i and 2 * 30 * 4096 / i are never odd integers for i <= 255), so floor(x + 0.5) is rint.
struct VisDivTables {
    int sdiv[256], hdiv[256];
    constexpr VisDivTables() : sdiv(), hdiv()
    {
        for (int i = 1; i < 256; i++) {
            sdiv[i] = (int)((double)(255 << 12) / (double)i + 0.5);
            hdiv[i] = (int)((double)(180 << 12) / (6.0 * (double)i) + 0.5);
        }
    }
};
__device__ const VisDivTables VIS_DIV = VisDivTables();

// c = b | g << 8 | r << 16 -> h | s << 8 | v << 16; sdiv, hdiv: the tables (in LDS)
__device__ __forceinline__ uint32_t vis_bgr2hsv(uint32_t c, const int* sdiv, const int* hdiv)
{
    const int b = c & 255, g = (c >> 8) & 255, r = (c >> 16) & 255;
    const int v = max(b, max(g, r)), d = v - min(b, min(g, r));
    const int s = (d * sdiv[v] + 2048) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
    h = (h * hdiv[d] + 2048) >> 12;                                   // arithmetic shift
    if (h < 0) h += 180;
    return (uint32_t)h | ((uint32_t)s << 8) | ((uint32_t)v << 16);
}

// ---- the flat pixel space of a call ------------------------------------------------------------------------------------------------------
// N pixels in all, n0 per image; threads 0 .. G - 1 own a group of 16, threads G .. G + (N - 16 G) - 1 one pixel each
struct VisSpan { uint32_t N, n0, G; };
__device__ __forceinline__ uint32_t vis_threads(const VisSpan& s) { return s.G + (s.N - VIS_GROUP * s.G); }
__device__ __forceinline__ uint32_t vis_first_px(const VisSpan& s, uint32_t t) { return t < s.G ? t * VIS_GROUP : s.G * VIS_GROUP + (t - s.G); }
// all pixels of this workgroup's threads lie in one image (the same answer in every thread)
__device__ __forceinline__ bool vis_wg_one_image(const VisSpan& s)
{
    const uint32_t t0 = blockIdx.x * VIS_WG, T = vis_threads(s);
    const uint32_t tl = (t0 + VIS_WG < T ? t0 + VIS_WG : T) - 1;
    const uint32_t last = tl < s.G ? tl * VIS_GROUP + VIS_GROUP - 1 : s.G * VIS_GROUP + (tl - s.G);
    return vis_first_px(s, t0) / s.n0 == last / s.n0;
}
static unsigned vis_grid(uint32_t N, uint32_t G)
{
    const uint64_t T = (uint64_t)G + (N - (uint64_t)VIS_GROUP * G);
    return (unsigned)((T + VIS_WG - 1) / VIS_WG);
}

__device__ __forceinline__ uint32_t vis_wave_min(uint32_t v) { for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o)); return v; }
__device__ __forceinline__ uint32_t vis_wave_max(uint32_t v) { for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o)); return v; }
__device__ __forceinline__ uint32_t vis_wave_sum(uint32_t v) { for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o); return v; }

// 16 pixels of flow, 16-byte loads (FAST), or one pixel, 4-byte loads
__device__ __forceinline__ void vis_load_group(const float* flow, uint32_t p0, float2* f)
{
    const float4* q = (const float4*)(flow + 2 * (size_t)p0);
#pragma unroll
    for (int i = 0; i < VIS_GROUP / 2; i++) {
        const float4 a = q[i];
        f[2 * i] = make_float2(a.x, a.y);
        f[2 * i + 1] = make_float2(a.z, a.w);
    }
}
__device__ __forceinline__ float2 vis_load_px(const float* flow, uint32_t p) { return make_float2(flow[2 * (size_t)p], flow[2 * (size_t)p + 1]); }
// four packed pixels (24 bits each) -> the three words they fill
__device__ __forceinline__ void vis_pack4(const uint32_t* c, uint32_t* w)
{
    w[0] = c[0] | (c[1] << 24);
    w[1] = (c[1] >> 8) | (c[2] << 16);
    w[2] = (c[2] >> 16) | (c[3] << 8);
}
__device__ __forceinline__ void vis_unpack4(const uint32_t* w, uint32_t* c)
{
    c[0] = w[0] & 0xFFFFFFu;
    c[1] = ((w[0] >> 24) | (w[1] << 8)) & 0xFFFFFFu;
    c[2] = ((w[1] >> 16) | (w[2] << 16)) & 0xFFFFFFu;
    c[3] = w[2] >> 8;
}
__device__ __forceinline__ void vis_store_group(uint8_t* img, uint32_t p0, const uint32_t* c)
{
    uint4* q = (uint4*)(img + 3 * (size_t)p0);
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 4; i++) vis_pack4(c + 4 * i, w + 3 * i);
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
__device__ __forceinline__ void vis_store_px(uint8_t* img, uint32_t p, uint32_t c)
{
    uint8_t* q = img + 3 * (size_t)p;
    q[0] = (uint8_t)c; q[1] = (uint8_t)(c >> 8); q[2] = (uint8_t)(c >> 16);
}

// ---- MAV_HSV_PROCESS, first pass: each image's minimum and maximum of the magnitude's bits ------------------------------------------------
__global__ void k_hsv_record_init(mav_hsv_record* rec, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t* w = (uint32_t*)(rec + b);
    w[0] = 0xFFFFFFFFu;          // mag_min's bits: above every magnitude's
    w[1] = 0u;                   // mag_max's bits
    w[2] = 0u;                   // nonzero
    w[3] = 1u;                   // invalid until a workgroup counts a non-zero value
}
__device__ __forceinline__ uint32_t vis_mag_bits(float2 f) { return __float_as_uint(sqrtf(f.x * f.x + f.y * f.y)); }
__device__ __forceinline__ void vis_minmax_flush(mav_hsv_record* rec, uint32_t img, uint32_t lo, uint32_t hi)
{
    atomicMin((uint32_t*)&rec[img].mag_min, lo);
    atomicMax((uint32_t*)&rec[img].mag_max, hi);
}
__global__ __launch_bounds__(VIS_WG) void k_flow_minmax(const float* __restrict__ flow, mav_hsv_record* rec, const VisSpan s)
{
    __shared__ uint32_t wlo[VIS_WG / 64], whi[VIS_WG / 64];
    const uint32_t t = blockIdx.x * VIS_WG + threadIdx.x;
    const bool live = t < vis_threads(s), one = vis_wg_one_image(s);
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, img = 0;
    if (live) {
        const uint32_t p0 = vis_first_px(s, t);
        img = p0 / s.n0;
        uint32_t next = (img + 1) * s.n0;
        if (t < s.G) {
            float2 f[VIS_GROUP];
            vis_load_group(flow, p0, f);
#pragma unroll
            for (int i = 0; i < VIS_GROUP; i++) {
                if (p0 + i >= next) {                                   // (only where n0 % 16 != 0)
                    vis_minmax_flush(rec, img, lo, hi);
                    lo = 0xFFFFFFFFu; hi = 0u;
                    while (p0 + i >= next) { img++; next += s.n0; }
                }
                const uint32_t m = vis_mag_bits(f[i]);
                lo = min(lo, m); hi = max(hi, m);
            }
        } else {
            lo = hi = vis_mag_bits(vis_load_px(flow, p0));
        }
    }
    if (!one) {
        if (live) vis_minmax_flush(rec, img, lo, hi);
        return;
    }
    lo = vis_wave_min(lo); hi = vis_wave_max(hi);
    if ((threadIdx.x & 63) == 0) { wlo[threadIdx.x >> 6] = lo; whi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {                                             // thread 0 of a launched workgroup is live
#pragma unroll
        for (int w = 1; w < VIS_WG / 64; w++) { lo = min(lo, wlo[w]); hi = max(hi, whi[w]); }
        vis_minmax_flush(rec, img, lo, hi);
    }
}

// ---- the picture ------------------------------------------------------------------------------------------------------------------------
// What MAV_HSV_PROCESS knows of the image in hand
struct VisImage {
    float lo, scale;
    __device__ __forceinline__ void bind(const mav_hsv_record* rec, uint32_t img)
    {
        const float l = rec[img].mag_min, h = rec[img].mag_max;
        const double d = (double)h - (double)l;
        lo = l;
        scale = d <= DBL_EPSILON ? 0.f : (float)(255.0 / d);          // the IEEE double quotient, rounded once: numpy's bits
    }
};
// One pixel's HSV, h | s << 8 | v << 16; nz: MAV_HSV_PROCESS's value before the repaint was not 0
template <int MODE>
__device__ __forceinline__ uint32_t vis_flow_hsv(float2 f, const VisImage& im, uint32_t& nz)
{
    const float mag = sqrtf(f.x * f.x + f.y * f.y);
    float ang = atan2f(f.y, f.x);
    int h, v;
    if constexpr (MODE == MAV_HSV_PROCESS) {
        if (ang < 0.f) ang = ang + VIS_2PI;
        h = (int)(((ang * 180.0f) / VIS_PI) / 2.0f) & 255;
        const float norm = (mag - im.lo) * im.scale;
        v = (int)(norm * 2.0f) & 255;
        nz = v != 0;
        if (v == 0) { h = 127; v = 255; }
    } else {
        ang = ang + VIS_PI;
        h = (int)(ang * VIS_HALF_DEG) & 255;
        const float m4 = mag * 4.0f;
        v = (int)(m4 < 255.0f ? m4 : 255.0f) & 255;
        nz = 0;
    }
    return (uint32_t)h | (255u << 8) | ((uint32_t)v << 16);
}
template <int MODE, bool HSV>
__global__ __launch_bounds__(VIS_WG) void k_flow_hsv(const float* __restrict__ flow, uint8_t* __restrict__ bgr, uint8_t* __restrict__ hsv,
                                                      mav_hsv_record* rec, const VisSpan s)
{
    __shared__ uint32_t wcnt[VIS_WG / 64];
    constexpr bool PROCESS = MODE == MAV_HSV_PROCESS;
    const uint32_t t = blockIdx.x * VIS_WG + threadIdx.x;
    const bool live = t < vis_threads(s);
    uint32_t cnt = 0, img = 0;
    if (live) {
        const uint32_t p0 = vis_first_px(s, t);
        VisImage im = {0.f, 0.f};
        uint32_t next = s.N;
        if constexpr (PROCESS) {
            img = p0 / s.n0;
            next = (img + 1) * s.n0;
            im.bind(rec, img);
        }
        if (t < s.G) {
            float2 f[VIS_GROUP];
            uint32_t c[VIS_GROUP], q[VIS_GROUP];
            vis_load_group(flow, p0, f);
#pragma unroll
            for (int i = 0; i < VIS_GROUP; i++) {
                if (PROCESS && p0 + i >= next) {                        // (only where n0 % 16 != 0)
                    if (cnt) { atomicAdd(&rec[img].nonzero, (int)cnt); rec[img].invalid = 0; }
                    cnt = 0;
                    while (p0 + i >= next) { img++; next += s.n0; }
                    im.bind(rec, img);
                }
                uint32_t nz;
                q[i] = vis_flow_hsv<MODE>(f[i], im, nz);
                cnt += nz;
                c[i] = vis_hsv2bgr(q[i] & 255, 255, q[i] >> 16);
            }
            vis_store_group(bgr, p0, c);
            if constexpr (HSV) vis_store_group(hsv, p0, q);
        } else {
            uint32_t nz;
            const uint32_t q = vis_flow_hsv<MODE>(vis_load_px(flow, p0), im, nz);
            cnt = nz;
            vis_store_px(bgr, p0, vis_hsv2bgr(q & 255, 255, q >> 16));
            if constexpr (HSV) vis_store_px(hsv, p0, q);
        }
    }
    if constexpr (PROCESS) {
        if (!vis_wg_one_image(s)) {
            if (cnt) { atomicAdd(&rec[img].nonzero, (int)cnt); rec[img].invalid = 0; }
            return;
        }
        cnt = vis_wave_sum(cnt);
        if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 1; w < VIS_WG / 64; w++) cnt += wcnt[w];
            if (cnt) { atomicAdd(&rec[img].nonzero, (int)cnt); rec[img].invalid = 0; }
        }
    }
}

// ---- cvtColor on uint8 x 3 -----------------------------------------------------------------------------------------------------------------
// CODE: MAV_COLOR_HSV2BGR, MAV_COLOR_BGR2HSV, MAV_COLOR_BGR2RADIAL (im_helpers.get_flow_radial: BGR2HSV, S = V = 255, HSV2BGR)
template <int CODE>
__device__ __forceinline__ uint32_t vis_cvt_px(uint32_t c, const int* sdiv, const int* hdiv)
{
    if constexpr (CODE == MAV_COLOR_HSV2BGR) return vis_hsv2bgr(c & 255, (c >> 8) & 255, c >> 16);
    else if constexpr (CODE == MAV_COLOR_BGR2HSV) return vis_bgr2hsv(c, sdiv, hdiv);
    else return vis_hsv2bgr(vis_bgr2hsv(c, sdiv, hdiv) & 255, 255, 255);
}
template <int CODE>
__global__ __launch_bounds__(VIS_WG) void k_cvt_color(const uint8_t* src, uint8_t* dst, const VisSpan s)
{
    __shared__ int sdiv[256], hdiv[256];
    if constexpr (CODE != MAV_COLOR_HSV2BGR) {
        sdiv[threadIdx.x] = VIS_DIV.sdiv[threadIdx.x];
        hdiv[threadIdx.x] = VIS_DIV.hdiv[threadIdx.x];
        __syncthreads();
    }
    const uint32_t t = blockIdx.x * VIS_WG + threadIdx.x;
    if (t >= vis_threads(s)) return;
    const uint32_t p0 = vis_first_px(s, t);
    if (t < s.G) {
        const uint4* q = (const uint4*)(src + 3 * (size_t)p0);
        uint32_t w[12], c[VIS_GROUP];
#pragma unroll
        for (int i = 0; i < 3; i++) { const uint4 a = q[i]; w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w; }
#pragma unroll
        for (int i = 0; i < 4; i++) vis_unpack4(w + 3 * i, c + 4 * i);
#pragma unroll
        for (int i = 0; i < VIS_GROUP; i++) c[i] = vis_cvt_px<CODE>(c[i], sdiv, hdiv);
        vis_store_group(dst, p0, c);
    } else {
        const uint8_t* q = src + 3 * (size_t)p0;
        vis_store_px(dst, p0, vis_cvt_px<CODE>((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), sdiv, hdiv));
    }
}
static_assert(VIS_WG == 256, "k_cvt_color fills its 256-entry tables one entry per thread");

// ---- draw_flow: one thread per grid point ------------------------------------------------------------------------------------------------
struct VisDraw { uint8_t* img; const float* flow; int W, H, step, nx, ny, B; float threshold; uint32_t colour; };
__device__ __forceinline__ void vis_put(const VisDraw& k, uint8_t* img, long long x, long long y)
{
    if (x < 0 || y < 0 || x >= k.W || y >= k.H) return;              // clip_line keeps a line inside; the circle's arms are clipped here
    vis_store_px(img, (uint32_t)y * (uint32_t)k.W + (uint32_t)x, k.colour);
}
// cv::clipLine on int64 points; false: nothing of the segment is inside
__device__ __forceinline__ bool vis_clip_line(long long W, long long H, long long& x1, long long& y1, long long& x2, long long& y2)
{
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}
__device__ __forceinline__ long long vis_end_point(int x, float fx)   // (x + fx + 0.5).astype(int32) of a float64 sum, clamped to +-2^30 first
{
    double e = (double)x + (double)fx + 0.5;
    e = fmin(fmax(e, -1073741824.0), 1073741824.0);
    return (long long)e;                                                // toward zero
}
__global__ __launch_bounds__(VIS_WG) void k_draw_flow(const VisDraw k)
{
    const uint32_t t = blockIdx.x * VIS_WG + threadIdx.x, per = (uint32_t)k.nx * k.ny;
    if (t >= per * (uint32_t)k.B) return;
    const uint32_t b = t / per, g = t - b * per, gy = g / (uint32_t)k.nx, gx = g - gy * (uint32_t)k.nx;
    const int x = k.step / 2 + (int)gx * k.step, y = k.step / 2 + (int)gy * k.step;      // < W, < H by the launch's nx, ny
    const size_t n0 = (size_t)k.W * k.H;
    const float2 f = vis_load_px(k.flow + 2 * n0 * b, (uint32_t)y * (uint32_t)k.W + (uint32_t)x);
    if (!(sqrtf(f.x * f.x + f.y * f.y) > k.threshold)) return;
    uint8_t* img = k.img + 3 * n0 * b;
    long long x1 = x, y1 = y, x2 = vis_end_point(x, f.x), y2 = vis_end_point(y, f.y);
    if (vis_clip_line(k.W, k.H, x1, y1, x2, y2)) {
        // LineIterator, 8-connected, left to right: the major axis advances every step, the minor one where err < 0
        long long dx = x2 - x1, dy = y2 - y1;
        if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
        const long long sy = dy < 0 ? -1 : 1;
        if (dy < 0) dy = -dy;
        const bool steep = dy > dx;
        const long long major = steep ? dy : dx, minor = steep ? dx : dy;
        long long err = major - 2 * minor, px = x1, py = y1;
        for (long long i = 0; i <= major; i++) {
            vis_put(k, img, px, py);
            const bool diag = err < 0;
            err += -2 * minor + (diag ? 2 * major : 0);
            if (steep) { py += sy; if (diag) px += 1; }
            else { px += 1; if (diag) py += sy; }
        }
    }
    // cv2.circle(img, (x, y), 1, colour, -1): the centre's row span x - 1 .. x + 1, and one pixel above and below
    vis_put(k, img, x - 1, y); vis_put(k, img, x, y); vis_put(k, img, x + 1, y);
    vis_put(k, img, x, y - 1); vis_put(k, img, x, y + 1);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
int vis_form(int W, int H, int batch, const void* flow, const void* bgr, const void* hsv)
{
    if (W < 1 || H < 1 || batch < 1) return -1;
    const uint64_t N = (uint64_t)W * H * batch;
    if (N < VIS_GROUP) return MAV_VIS_FORM_BYTES;
    const uintptr_t all = (uintptr_t)flow | (uintptr_t)bgr | (uintptr_t)hsv;       // a NULL pointer constrains nothing
    return all % 16 ? MAV_VIS_FORM_BYTES : MAV_VIS_FORM_FAST;
}
static VisSpan vis_span(int W, int H, int B, int form)
{
    const uint32_t N = (uint32_t)((size_t)W * H * B);
    return VisSpan{N, (uint32_t)((size_t)W * H), form == MAV_VIS_FORM_FAST ? N / VIS_GROUP : 0u};
}
hipError_t launch_flow_hsv(hipStream_t st, const float* flow, int W, int H, int B, int mode, uint8_t* bgr, uint8_t* hsv, void* records)
{
    mav_hsv_record* rec = (mav_hsv_record*)records;
    const VisSpan s = vis_span(W, H, B, vis_form(W, H, B, flow, bgr, hsv));
    const dim3 grid(vis_grid(s.N, s.G)), block(VIS_WG);
    if (mode == MAV_HSV_PROCESS) {
        hipLaunchKernelGGL(k_hsv_record_init, dim3((B + 63) / 64), dim3(64), 0, st, rec, B);
        hipLaunchKernelGGL(k_flow_minmax, grid, block, 0, st, flow, rec, s);
        if (hsv) hipLaunchKernelGGL((k_flow_hsv<MAV_HSV_PROCESS, true>), grid, block, 0, st, flow, bgr, hsv, rec, s);
        else hipLaunchKernelGGL((k_flow_hsv<MAV_HSV_PROCESS, false>), grid, block, 0, st, flow, bgr, hsv, rec, s);
    } else {
        const hipError_t e = hipMemsetAsync(rec, 0, sizeof(mav_hsv_record) * (size_t)B, st);
        if (e != hipSuccess) return e;                                  // nothing is launched on records that were not zeroed
        if (hsv) hipLaunchKernelGGL((k_flow_hsv<MAV_HSV_DRAW, true>), grid, block, 0, st, flow, bgr, hsv, rec, s);
        else hipLaunchKernelGGL((k_flow_hsv<MAV_HSV_DRAW, false>), grid, block, 0, st, flow, bgr, hsv, rec, s);
    }
    return hipSuccess;
}
void launch_cvt_color(hipStream_t st, const uint8_t* src, int code, int W, int H, int B, uint8_t* dst)
{
    const VisSpan s = vis_span(W, H, B, vis_form(W, H, B, nullptr, dst, src));
    const dim3 grid(vis_grid(s.N, s.G)), block(VIS_WG);
    switch (code) {
    case MAV_COLOR_HSV2BGR: hipLaunchKernelGGL(k_cvt_color<MAV_COLOR_HSV2BGR>, grid, block, 0, st, src, dst, s); break;
    case MAV_COLOR_BGR2HSV: hipLaunchKernelGGL(k_cvt_color<MAV_COLOR_BGR2HSV>, grid, block, 0, st, src, dst, s); break;
    case MAV_COLOR_BGR2RADIAL: hipLaunchKernelGGL(k_cvt_color<MAV_COLOR_BGR2RADIAL>, grid, block, 0, st, src, dst, s); break;
    }
}
void vis_draw_grid(int W, int H, int step, int* nx, int* ny)
{
    const long long first = step / 2;
    *nx = first < W ? (int)((W - first + step - 1) / step) : 0;
    *ny = first < H ? (int)((H - first + step - 1) / step) : 0;
}
void launch_draw_flow(hipStream_t st, uint8_t* img, const float* flow, int W, int H, int B, int step, float threshold, const uint8_t* colour)
{
    VisDraw k = {img, flow, W, H, step, 0, 0, B, threshold, (uint32_t)colour[0] | ((uint32_t)colour[1] << 8) | ((uint32_t)colour[2] << 16)};
    vis_draw_grid(W, H, step, &k.nx, &k.ny);
    const uint64_t T = (uint64_t)k.nx * k.ny * B;
    if (!T) return;
    hipLaunchKernelGGL(k_draw_flow, dim3((unsigned)((T + VIS_WG - 1) / VIS_WG)), dim3(VIS_WG), 0, st, k);
}

// PNG decode on the device (include/mavflow_png_decode.h): zlib streams in, frames out.  gfx950; integer arithmetic only.
//
// Three launches per call, one workgroup per image in each:
//   k_png_inflate   ONE WAVEFRONT per stream (a workgroup is one wave of 64).  The symbol loop of inflate_core.h runs on values every
//                   lane holds alike (readfirstlane keeps them on the scalar side); the stream is read through a 1 KB window in LDS
//                   that the 64 lanes fill together; the code tables (3.6 KB of LDS) are filled by lane-strided loops.  Tokens are
//                   queued one per lane, IN REGISTERS; a full queue (64 tokens), a stored block and the end of the stream resolve it:
//                   a prefix sum of the lengths across the wave gives every token its position, all literals are written at once,
//                   and the matches follow in order, each copied by the 64 lanes (byte i of a match comes from
//                   out[p - distance + i % distance], which lies below p and is therefore written already).
//   k_png_adler     256 threads per image: a slice's (sum, weighted sum) each, exact integers modulo 65521, combined in slice order.
//   k_png_unfilter  one wave per image: 64 rows at a time, lane l one pixel behind lane l - 1, so that the pixel above and the pixel
//                   above-left arrive by __shfl_up from the lane of the row above and the pixel to the left is the lane's own last
//                   result.  The output conversion is fused into the store.  Bands of 64 rows go in order; a band's last row is
//                   written back over its filtered bytes in the scratch, where lane 0 of the next band reads it.
//
// STORE-TO-LOAD ORDER.  A lane reads bytes another lane of the same wave stored (a match's source, a band's last row, the LDS window
// and tables).  The workgroup IS the wave, so __syncthreads() is a barrier every lane reaches in uniform control flow, and it orders
// the workgroup's global and LDS stores before the loads behind it (the stores are waited for; all lanes share the CU's L1, which a
// store writes through).  The copy stage does not pay it per match: it tracks the lowest output position written since the last
// barrier, and a match whose source ends at or below that position reads only bytes from before the barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mavflow_internal.h"
#include "inflate_core.h"
#include "../../include/mavflow_png_decode.h"

#define PD_WAVE 64
#define PD_WINDOW 1024                 // stream bytes staged in LDS
#define PD_ADLER_WG 256
#define PD_CHUNK 8                     // pixels a lane loads ahead of the recurrence in the un-filter pass

__device__ inline uint64_t pd_uniform64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// ---- the device policies of inflate_core.h ---------------------------------------------------------------------------------------------
struct PdPar {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return PD_WAVE; }
    __device__ void sync() const { __syncthreads(); }
};
// the stream through a window in LDS: bytes base .. base + PD_WINDOW - 1, zero past the stream's end
struct PdSrc {
    const uint8_t* z;
    uint64_t n;
    uint8_t* win;
    uint64_t base;
    bool loaded;
    __device__ uint32_t word(size_t pos)
    {
        if (!loaded || pos < base || pos + 4 > base + PD_WINDOW) {
            base = pos;
            loaded = true;
            __syncthreads();                                   // the loads of the old window are over
            for (uint32_t i = threadIdx.x; i < PD_WINDOW; i += PD_WAVE) win[i] = base + i < n ? z[base + i] : (uint8_t)0;
            __syncthreads();
        }
        const uint32_t o = (uint32_t)(pos - base);
        return (uint32_t)win[o] | ((uint32_t)win[o + 1] << 8) | ((uint32_t)win[o + 2] << 16) | ((uint32_t)win[o + 3] << 24);
    }
};
// the copy stage: lane k holds token k of the queue
struct PdSink {
    const uint8_t* z;
    uint8_t* raw;
    uint32_t qn = 0;                   // tokens queued
    uint64_t qpos = 0;                 // the output position of token 0
    uint64_t dirty_lo = ~0ull;         // the lowest output position written since the last barrier
    uint32_t tlen = 0, tdist = 0, tbyte = 0;
    __device__ PdSink(const uint8_t* z_, uint8_t* raw_) : z(z_), raw(raw_) {}
    __device__ void push(uint64_t pos, uint32_t len, uint32_t dist, uint32_t byte)
    {
        if (qn == 0) qpos = pos;
        if (threadIdx.x == qn) { tlen = len; tdist = dist; tbyte = byte; }
        if (++qn == PD_WAVE) flush();
    }
    __device__ void literal(uint64_t pos, uint32_t byte) { push(pos, 1, 0, byte); }
    __device__ void match(uint64_t pos, uint32_t len, uint32_t dist) { push(pos, len, dist, 0); }
    __device__ void stored(uint64_t pos, uint64_t at, uint32_t len)
    {
        flush();
        for (uint32_t i = threadIdx.x; i < len; i += PD_WAVE) raw[pos + i] = z[at + i];
        if (pos < dirty_lo) dirty_lo = pos;
    }
    __device__ void finish() { flush(); }
    __device__ void flush()
    {
        if (qn == 0) return;
        const uint32_t lane = threadIdx.x;
        const bool active = lane < qn;
        const uint32_t len = active ? tlen : 0;
        uint32_t incl = len;                                   // inclusive prefix sum of the lengths (at most 64 * 258)
        for (uint32_t d = 1; d < PD_WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const uint32_t off = incl - len;
        const bool is_match = active && tdist != 0;
        if (active && !is_match) raw[qpos + off] = (uint8_t)tbyte;
        unsigned long long matches = __ballot(is_match);
        if (__ballot(active && !is_match) && qpos < dirty_lo) dirty_lo = qpos;
        while (matches) {
            const int t = __ffsll((long long)matches) - 1;
            matches &= matches - 1;
            const uint64_t p = qpos + INF_U32(__shfl(off, t));
            const uint32_t l = INF_U32(__shfl(len, t)), d = INF_U32(__shfl(tdist, t));
            if (p - d + (l < d ? l : d) > dirty_lo) {          // the source reaches into bytes written since the last barrier
                __syncthreads();
                dirty_lo = ~0ull;
            }
            const uint8_t* src = raw + (p - d);
            if (d >= l) {
                for (uint32_t i = lane; i < l; i += PD_WAVE) raw[p + i] = src[i];
            } else {
                for (uint32_t i = lane; i < l; i += PD_WAVE) raw[p + i] = src[i % d];
            }
            if (p < dirty_lo) dirty_lo = p;
        }
        qn = 0;
    }
};

// grid: count workgroups of one wave.  raw: count blocks of raw_stride bytes; status: count records, written in full.
__global__ __launch_bounds__(PD_WAVE) void k_png_inflate(const uint8_t* __restrict__ streams, const uint64_t* __restrict__ index, uint64_t raw_bytes,
                                                         uint64_t raw_stride, uint8_t* raw, mav_png_status* status)
{
    __shared__ InfTables T;
    __shared__ uint8_t win[PD_WINDOW];
    const uint32_t s = blockIdx.x;
    const uint64_t off = pd_uniform64(index[2 * s]), n = pd_uniform64(index[2 * s + 1]);
    PdSrc src{streams + off, n, win, 0, false};
    PdPar par;
    PdSink sink(streams + off, raw + raw_stride * s);
    mav_png_status st;
    inf_run(src, n, raw_bytes, &T, par, sink, &st);
    if (threadIdx.x == 0) status[s] = st;
}

// Adler-32 of every image whose inflate succeeded; a mismatch sets MAV_PNG_E_ADLER.  Per slice of n bytes: s1 = sum b, s2 = sum (n - i) b_i;
// a slice continues (A, B) as A + s1, B + n A + s2, modulo 65521.
__global__ __launch_bounds__(PD_ADLER_WG) void k_png_adler(const uint8_t* __restrict__ raw, uint64_t raw_bytes, uint64_t raw_stride, mav_png_status* status)
{
    __shared__ uint32_t s1[PD_ADLER_WG], s2[PD_ADLER_WG], sn[PD_ADLER_WG];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (status[s].code != 0) return;
    const uint8_t* p = raw + raw_stride * s;
    const uint64_t per = (raw_bytes + PD_ADLER_WG - 1) / PD_ADLER_WG;
    const uint64_t lo = per * t < raw_bytes ? per * t : raw_bytes, hi = lo + per < raw_bytes ? lo + per : raw_bytes;
    uint64_t a = 0, b = 0;
    for (uint64_t i = lo; i < hi;) {
        const uint64_t e = i + 4096 < hi ? i + 4096 : hi;      // 4096 * 255 and its running sums stay far below 2^64
        for (; i < e; i++) { a += p[i]; b += a; }
        a %= 65521u;
        b %= 65521u;
    }
    s1[t] = (uint32_t)a;
    s2[t] = (uint32_t)b;
    sn[t] = (uint32_t)((hi - lo) % 65521u);
    __syncthreads();
    if (t == 0) {
        uint64_t A = 1, B = 0;
        for (int k = 0; k < PD_ADLER_WG; k++) {
            B = (B + (uint64_t)sn[k] * A + s2[k]) % 65521u;
            A = (A + s1[k]) % 65521u;
        }
        const uint32_t adler = (uint32_t)((B << 16) | A);
        status[s].adler_computed = adler;
        if (adler != status[s].adler_stream) status[s].code = MAV_PNG_E_ADLER;
    }
}

// one byte of a pixel: the filtered byte x, the reconstructed bytes left (a), above (b), above-left (c)
__device__ inline uint32_t pd_recon(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;
    else if (ft == 4) {
        const int p = (int)a + (int)b - (int)c, pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x + pred) & 255u;
}

// grid: count workgroups of one wave.  raw: the inflated rows (a band's last row is un-filtered in place); out: zero before the launch,
// written only for an image whose code is 0 and stays 0.
template <int BPP>
__global__ __launch_bounds__(PD_WAVE) void k_png_unfilter(uint8_t* raw_all, uint64_t raw_stride, int W, int H, int format, uint8_t* out_all,
                                                          mav_png_status* status)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (status[s].code != 0) return;
    uint8_t* raw = raw_all + raw_stride * s;
    const uint32_t stride = (uint32_t)W * BPP, pitch = stride + 1;
    bool bad = false;
    for (int r = (int)lane; r < H; r += PD_WAVE) bad |= raw[(size_t)r * pitch] > 4;
    if (__ballot(bad)) {
        if (lane == 0) status[s].code = MAV_PNG_E_FILTER;
        return;
    }
    const int oc = format == MAV_PNG_OUT_SAMPLES ? BPP : format == MAV_PNG_OUT_BGR ? 3 : 1;
    uint8_t* out = out_all + (size_t)W * H * oc * s;
    const int steps = W + PD_WAVE - 1;
    for (int r0 = 0; r0 < H; r0 += PD_WAVE) {
        const int r = r0 + (int)lane;
        const bool row = r < H;
        uint8_t* in = raw + (size_t)(row ? r : 0) * pitch;
        const uint8_t* up = raw + (size_t)(r > 0 && row ? r - 1 : 0) * pitch + 1;     // read by lane 0 of a band behind the first alone
        const uint32_t ft = row ? in[0] : 0;
        const bool write_back = lane == PD_WAVE - 1 && r0 + PD_WAVE < H;
        uint32_t prev = 0, up_left = 0;                        // the lane's last pixel; the pixel above it
        for (int s0 = 0; s0 < steps; s0 += PD_CHUNK) {
            uint32_t cur[PD_CHUNK], above[PD_CHUNK];
#pragma unroll
            for (int k = 0; k < PD_CHUNK; k++) {
                const int x = s0 + k - (int)lane;
                cur[k] = above[k] = 0;
                if (row && x >= 0 && x < W) {
                    for (int j = 0; j < BPP; j++) cur[k] |= (uint32_t)in[1 + (size_t)x * BPP + j] << (8 * j);
                    if (lane == 0 && r0 > 0)
                        for (int j = 0; j < BPP; j++) above[k] |= (uint32_t)up[(size_t)x * BPP + j] << (8 * j);
                }
            }
#pragma unroll
            for (int k = 0; k < PD_CHUNK; k++) {
                const int x = s0 + k - (int)lane;
                uint32_t b = __shfl_up(prev, 1);               // lane l - 1's pixel of the step before: the pixel above this one
                if (lane == 0) b = above[k];
                if (row && x >= 0 && x < W) {
                    const uint32_t a = x > 0 ? prev : 0, c = x > 0 ? up_left : 0;
                    uint32_t px = 0;
                    for (int j = 0; j < BPP; j++)
                        px |= pd_recon(ft, (cur[k] >> (8 * j)) & 255u, (a >> (8 * j)) & 255u, (b >> (8 * j)) & 255u, (c >> (8 * j)) & 255u) << (8 * j);
                    prev = px;
                    up_left = b;
                    const size_t o = (size_t)r * W + x;
                    const uint32_t v0 = px & 255u, v1 = (px >> 8) & 255u, v2 = (px >> 16) & 255u;
                    if (format == MAV_PNG_OUT_SAMPLES) {
                        for (int j = 0; j < BPP; j++) out[o * BPP + j] = (uint8_t)(px >> (8 * j));
                    } else if (format == MAV_PNG_OUT_BGR) {
                        out[o * 3] = (uint8_t)(BPP < 3 ? v0 : v2);
                        out[o * 3 + 1] = (uint8_t)(BPP < 3 ? v0 : v1);
                        out[o * 3 + 2] = (uint8_t)v0;
                    } else {
                        out[o] = BPP < 3 ? (uint8_t)v0 : bgr2gray_px(v2, v1, v0);
                    }
                    if (write_back)
                        for (int j = 0; j < BPP; j++) in[1 + (size_t)x * BPP + j] = (uint8_t)(px >> (8 * j));
                }
            }
        }
        __syncthreads();                                       // the band's last row is in the scratch before the next band's lane 0 reads it
    }
}

// ---- host side: the entry points of include/mavflow_png_decode.h -----------------------------------------------------------------------
#define PCHK(call) do { const int rc_ = (call); if (rc_ != MAV_OK) return rc_; } while (0)

static uint64_t pd_raw_bytes(int W, int H, int channels) { return (uint64_t)H * (1 + (uint64_t)W * channels); }
static uint64_t pd_raw_stride(int W, int H, int channels) { return (pd_raw_bytes(W, H, channels) + 15) & ~(uint64_t)15; }
static bool pd_shape_ok(int W, int H, int channels, int count)
{
    return W >= 1 && H >= 1 && channels >= 1 && channels <= 4 && count >= 1 && count <= MAV_PNG_DECODE_MAX_COUNT &&
           pd_raw_bytes(W, H, channels) <= 0x7FFFFFFFull;
}
static int pd_out_channels(int channels, int out_format)
{
    return out_format == MAV_PNG_OUT_SAMPLES ? channels : out_format == MAV_PNG_OUT_BGR ? 3 : 1;
}
extern "C" size_t mav_png_decode_scratch_bytes(int W, int H, int channels, int count)
{
    return pd_shape_ok(W, H, channels, count) ? (size_t)(pd_raw_stride(W, H, channels) * (uint64_t)count) : 0;
}
extern "C" int mav_png_inflate_host(const uint8_t* z, size_t n, uint8_t* raw, size_t raw_bytes, mav_png_status* status)
{
    if (!status || (!z && n) || (!raw && raw_bytes)) return ctx_fail(MAV_ERR_ARG, "mav_png_inflate_host: NULL argument");
    inf_inflate_host(z, n, raw, raw_bytes, status);
    return MAV_OK;
}
static int pd_checked(mav_ctx* c, const void* streams, const void* index, int count, int W, int H, int channels, int out_format, const void* out,
                      const void* status, const char* fn)
{
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!streams || !index || !out || !status) return ctx_fail(MAV_ERR_ARG, "%s: NULL %s", fn, !streams ? "streams" : !index ? "index" : !out ? "out" : "status");
    if (count < 1 || count > MAV_PNG_DECODE_MAX_COUNT) return ctx_fail(MAV_ERR_ARG, "%s: count %d outside [1, %d]", fn, count, MAV_PNG_DECODE_MAX_COUNT);
    if (channels < 1 || channels > 4) return ctx_fail(MAV_ERR_ARG, "%s: channels %d outside [1, 4]", fn, channels);
    if (out_format != MAV_PNG_OUT_SAMPLES && out_format != MAV_PNG_OUT_BGR && out_format != MAV_PNG_OUT_GRAY)
        return ctx_fail(MAV_ERR_ARG, "%s: out_format %d is none of MAV_PNG_OUT_*", fn, out_format);
    if (!pd_shape_ok(W, H, channels, count))
        return ctx_fail(MAV_ERR_ARG, "%s: an image of %d x %d x %d is empty or inflates to more than 2^31 - 1 bytes", fn, W, H, channels);
    return MAV_OK;
}
// the launches of one call
static int pd_launch(mav_ctx* c, const CtxView& v, const uint8_t* streams, const uint64_t* index, int count, int W, int H, int channels, int out_format,
                     uint8_t* out, mav_png_status* status, void* scratch, const char* fn)
{
    const uint64_t raw_bytes = pd_raw_bytes(W, H, channels), raw_stride = pd_raw_stride(W, H, channels);
    const size_t out_bytes = (size_t)W * H * pd_out_channels(channels, out_format) * count;
    MiscScope ps(c);
    const hipError_t e = hipMemsetAsync(out, 0, out_bytes, v.stream);
    if (e != hipSuccess) return ctx_fail(MAV_ERR_HIP, "%s: clearing the output failed: %s", fn, hipGetErrorString(e));
    uint8_t* raw = (uint8_t*)scratch;
    hipLaunchKernelGGL(k_png_inflate, dim3(count), dim3(PD_WAVE), 0, v.stream, streams, index, raw_bytes, raw_stride, raw, status);
    hipLaunchKernelGGL(k_png_adler, dim3(count), dim3(PD_ADLER_WG), 0, v.stream, raw, raw_bytes, raw_stride, status);
    switch (channels) {
    case 1: hipLaunchKernelGGL(k_png_unfilter<1>, dim3(count), dim3(PD_WAVE), 0, v.stream, raw, raw_stride, W, H, out_format, out, status); break;
    case 2: hipLaunchKernelGGL(k_png_unfilter<2>, dim3(count), dim3(PD_WAVE), 0, v.stream, raw, raw_stride, W, H, out_format, out, status); break;
    case 3: hipLaunchKernelGGL(k_png_unfilter<3>, dim3(count), dim3(PD_WAVE), 0, v.stream, raw, raw_stride, W, H, out_format, out, status); break;
    default: hipLaunchKernelGGL(k_png_unfilter<4>, dim3(count), dim3(PD_WAVE), 0, v.stream, raw, raw_stride, W, H, out_format, out, status); break;
    }
    return ctx_check_launch("png_decode");
}
extern "C" int mav_png_decode_dev(mav_ctx* c, const uint8_t* streams, const uint64_t* index, int count, int W, int H, int channels, int out_format,
                                  uint8_t* out, mav_png_status* status, void* scratch)
{
    const char* fn = "mav_png_decode_dev";
    PCHK(pd_checked(c, streams, index, count, W, H, channels, out_format, out, status, fn));
    if (!scratch) return ctx_fail(MAV_ERR_ARG, "%s: NULL scratch", fn);
    if ((uintptr_t)index % 8 || (uintptr_t)status % 8 || (uintptr_t)scratch % 16)
        return ctx_fail(MAV_ERR_ARG, "%s: index and status must be aligned to 8, scratch to 16", fn);
    CtxView v;
    PCHK(ctx_enter(c, 1, fn, &v));          // the count is the call's own: not bound by max_batch
    return pd_launch(c, v, streams, index, count, W, H, channels, out_format, out, status, scratch, fn);
}
extern "C" int mav_png_decode(mav_ctx* c, const uint8_t* streams, const uint64_t* index, int count, int W, int H, int channels, int out_format,
                              uint8_t* out, mav_png_status* status)
{
    const char* fn = "mav_png_decode";
    PCHK(pd_checked(c, streams, index, count, W, H, channels, out_format, out, status, fn));
    uint64_t bytes = 0;
    for (int i = 0; i < count; i++) {
        const uint64_t off = index[2 * i], n = index[2 * i + 1];
        if (off > (1ull << 40) || n > (1ull << 40)) return ctx_fail(MAV_ERR_ARG, "%s: stream %d lies at offset %llu with %llu bytes", fn, i,
                                                                     (unsigned long long)off, (unsigned long long)n);
        if (off + n > bytes) bytes = off + n;
    }
    StagedCall h(c, fn);
    CtxView v;
    PCHK(h.begin(1, &v));
    const uint8_t* ds = (const uint8_t*)h.in(streams, (size_t)(bytes ? bytes : 1));
    const uint64_t* di = (const uint64_t*)h.in(index, sizeof(uint64_t) * 2 * (size_t)count);
    uint8_t* dout = (uint8_t*)h.out(out, (size_t)W * H * pd_out_channels(channels, out_format) * count);
    mav_png_status* dst = (mav_png_status*)h.out(status, sizeof(mav_png_status) * (size_t)count);
    void* scratch = h.scratch(mav_png_decode_scratch_bytes(W, H, channels, count));
    PCHK(h.staged());
    PCHK(pd_launch(c, v, ds, di, count, W, H, channels, out_format, dout, dst, scratch, fn));
    return h.finish();
}
static_assert(sizeof(mav_png_status) == 48, "mav_png_status");

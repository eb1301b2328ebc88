// JPEG decode on the device (include/mavflow_jpeg.h): baseline files in, frames out.  gfx950; integer arithmetic only, no inline assembly.
// The decoding source is jpeg_core.h, shared with the host build (mav_jpeg_decode_host) and with tools/jpeg_check.c.
//
// Four launches per call; an image's scratch holds its coefficients, its component planes, a header and its interval table:
//   k_jpeg_intervals  one workgroup of 256 per image.  Thread 0 runs jc_info_ok on the image's info (the verdict UNSUPPORTED keeps every
//                     later launch away from that info) and clears the status record.  The workgroup then scans the entropy bytes for
//                     FF D0..D7 pairs, 2048 bytes a step, and compacts them in order (a prefix sum of the threads' counts) into the
//                     table's rows (byte offset behind the marker, first MCU).  The table is general: a row is where a unit starts.
//   k_jpeg_entropy    ONE WAVEFRONT per (image, interval), as k_png_inflate has one per stream: a workgroup is one wave of 64 and walks
//                     the image's intervals with the grid's stride.  The symbol loop of jpeg_core.h runs on values every lane holds
//                     alike (readfirstlane keeps them on the scalar side); the bytes come through a 1 KB window in LDS that the 64
//                     lanes fill together; the code tables (11 KB of LDS) are filled by lane-strided loops, once per workgroup.  Lane i
//                     holds coefficient i of the block in hand IN A REGISTER, so a block leaves as one 128-byte store and every
//                     coefficient of it is written.  The DC predictor starts at 0 in every interval: nothing crosses intervals.
//   k_jpeg_idct       eight lanes per block, 32 blocks per workgroup: lane j loads row j as one 16-byte load and dequantises it, the
//                     block is transposed through LDS for the column pass (descale 11) and back for the row pass (descale 18), and
//                     lane j stores row j of the 8-bit plane as one 8-byte store.
//   k_jpeg_finish     one thread per four output pixels: upsampling (the row neighbours of h2v2 come from the planes), colour
//                     conversion, crop and the output format, stored as 4-byte words.  A failed image's output is written as zeros
//                     here, so no byte of `out` is written twice and none is left out.  Thread 0 of an image's first workgroup turns
//                     the error word into the status' code and `consumed`.
//
// STORE-TO-LOAD ORDER.  Within a launch only LDS is read back (behind __syncthreads()); everything in global memory that a launch reads
// was written by an earlier launch on the same stream.  The units of an image meet in its status record and error word through
// atomics (sums, a maximum, a minimum), whose results do not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mavflow_internal.h"
#define JC_GRAY_PX(b, g, r) bgr2gray_px((b), (g), (r))
#include "jpeg_core.h"
#include "../../include/mavflow_jpeg.h"

#define JD_WAVE 64
#define JD_WINDOW 1024                 // entropy bytes staged in LDS
#define JD_SCAN_WG 256
#define JD_SCAN_PER 8                  // bytes a thread tests per step of the marker scan
#define JD_IDCT_WG 256                 // 32 blocks of 8 lanes
#define JD_FINISH_WG 256
#define JD_MAX_UNITS_X 256             // workgroups per image in the entropy launch

struct JdCall {
    const uint8_t* files; const uint64_t* index; const mav_jpeg_info* info; int count, W, H, format;
    uint8_t* out; mav_jpeg_status* status; void* scratch;
};
// the call's component count is image 0's; an info that names neither 1 nor 3 is refused by jc_info_ok under either
__host__ __device__ inline int jd_comps(const mav_jpeg_info* info) { return info[0].components == 3 ? 3 : 1; }

__global__ __launch_bounds__(JD_SCAN_WG) void k_jpeg_intervals(JdCall a)
{
    __shared__ int ok_s;
    __shared__ uint32_t wave_sum[JD_SCAN_WG / JD_WAVE];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const int comps = jd_comps(a.info);
    const JcScratch sc = jc_scratch_of(a.scratch, a.W, a.H, comps, s);
    const mav_jpeg_info* I = a.info + s;
    const uint64_t file_off = a.index[2 * s], file_size = a.index[2 * s + 1];
    if (t == 0) {
        const bool ok = jc_info_ok(I, a.W, a.H, comps, file_size);
        ok_s = ok;
        mav_jpeg_status st = {};
        JcGeom g0;
        if (ok) {
            jc_geometry(I, &g0);
            st.intervals = (uint32_t)g0.intervals;
        }
        a.status[s] = st;
        sc.hdr[0] = ok ? JC_NO_ERR : (uint32_t)MAV_JPEG_E_UNSUPPORTED;
        sc.hdr[1] = 0;
        sc.hdr[2] = ok ? 0u : 1u;
        sc.hdr[3] = 0;
        sc.table[0] = sc.table[1] = sc.table[2] = sc.table[3] = 0;
    }
    __syncthreads();
    if (!ok_s) return;
    JcGeom g;
    jc_geometry(I, &g);
    if (!g.ri) return;
    const uint8_t* z = a.files + file_off + I->entropy_offset;
    const uint32_t size = (uint32_t)I->entropy_bytes;
    uint32_t total = 0;
    for (uint32_t base = 0; base < size; base += JD_SCAN_WG * JD_SCAN_PER) {
        const uint32_t i0 = base + t * JD_SCAN_PER;
        uint32_t hits = 0;
        if (i0 < size) {
            uint32_t prev = z[i0];
            for (uint32_t j = 0; j < JD_SCAN_PER; j++) {
                const uint32_t i = i0 + j;
                if (i + 1 >= size) break;
                const uint32_t next = z[i + 1];
                if (jc_is_rst(prev, next)) hits |= 1u << j;
                prev = next;
            }
        }
        const uint32_t mine = (uint32_t)__popc(hits);
        uint32_t incl = mine;
        const uint32_t lane = t % JD_WAVE, wave = t / JD_WAVE;
        for (uint32_t d = 1; d < JD_WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        __syncthreads();                                       // the last step's wave sums have been read
        if (lane == JD_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = total + incl - mine, all = 0;
        for (uint32_t w = 0; w < JD_SCAN_WG / JD_WAVE; w++) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        for (uint32_t j = 0; j < JD_SCAN_PER; j++)
            if (hits & (1u << j)) {
                before++;                                      // marker number `before` opens interval `before`
                if (before < (uint32_t)g.intervals) {
                    uint32_t* row = sc.table + 4 * (size_t)before;
                    row[0] = i0 + j + 2;
                    row[1] = before * (uint32_t)g.ri;
                    row[2] = 0;
                    row[3] = 0;
                }
            }
        total += all;
    }
    if (t == 0) sc.hdr[1] = total;
}

// ---- the device policies of jpeg_core.h ---------------------------------------------------------------------------------------------------
struct JdPar {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return JD_WAVE; }
    __device__ void sync() const { __syncthreads(); }
};
// the entropy segment through a window in LDS: bytes base .. base + JD_WINDOW - 1 (zero behind the segment's end, which nothing asks for)
struct JdSrc {
    const uint8_t* z;
    uint32_t n;
    uint8_t* win;
    uint32_t base;
    bool loaded;
    __device__ uint32_t byte(uint32_t pos)
    {
        if (!loaded || pos < base || pos >= base + JD_WINDOW) {
            base = pos;
            loaded = true;
            __syncthreads();                                   // the loads of the old window are over
            for (uint32_t i = threadIdx.x; i < JD_WINDOW; i += JD_WAVE) win[i] = base + i < n ? z[base + i] : (uint8_t)0;
            __syncthreads();
        }
        return JC_U32(win[pos - base]);
    }
};
// lane i holds coefficient i of the block in hand
struct JdSink {
    int16_t mine;
    __device__ void begin() { mine = 0; }
    __device__ void coef(uint32_t i, int16_t v) { if (threadIdx.x == i) mine = v; }
    __device__ void end(int16_t* dst) { dst[threadIdx.x] = mine; }
};

// grid: (workgroups per image, count), one wave each
__global__ __launch_bounds__(JD_WAVE) void k_jpeg_entropy(JdCall a)
{
    __shared__ JcTables T;
    __shared__ mav_jpeg_info info_s;
    __shared__ uint8_t win[JD_WINDOW];
    const uint32_t s = blockIdx.y;
    const int comps = jd_comps(a.info);
    const JcScratch sc = jc_scratch_of(a.scratch, a.W, a.H, comps, s);
    if (JC_U32(sc.hdr[2])) return;                             // an info nothing may be read through
    {
        const uint32_t* from = (const uint32_t*)(a.info + s);
        uint32_t* to = (uint32_t*)&info_s;
        for (uint32_t i = threadIdx.x; i < sizeof(mav_jpeg_info) / 4; i += JD_WAVE) to[i] = from[i];
    }
    __syncthreads();
    const mav_jpeg_info* I = &info_s;
    JcGeom g;
    jc_geometry(I, &g);
    const uint32_t intervals = JC_U32(g.intervals);
    if (blockIdx.x >= intervals) return;
    JdPar par;
    jc_build_tables(par, I, &T);
    const uint32_t found = JC_U32(sc.hdr[1]), size = JC_U32((uint32_t)I->entropy_bytes);
    const uint64_t at = a.index[2 * s] + I->entropy_offset;
    const uint8_t* z = a.files + (((uint64_t)JC_U32((uint32_t)(at >> 32)) << 32) | JC_U32((uint32_t)at));
    for (uint32_t k = blockIdx.x; k < intervals; k += gridDim.x) {
        JcUnit u;
        uint32_t* row = sc.table + 4 * (size_t)k;
        if (k > found) {
            jc_missing_interval(size, &u);
        } else {
            const uint32_t start = JC_U32(row[0]), first = JC_U32(row[1]), left = (uint32_t)g.mcus - first;
            JdSrc src{z, size, win, 0, false};
            JdSink sink;
            jc_decode_interval(src, size, start, I, g, &T, sink, sc.coef, k, first, g.ri && (uint32_t)g.ri < left ? (uint32_t)g.ri : left,
                               k + 1 == intervals, &u);
        }
        if (threadIdx.x == 0) jc_merge(a.status + s, sc.hdr, row, k, u);
    }
}

// grid: (ceil(blocks of one image at most / 32), count)
__global__ __launch_bounds__(JD_IDCT_WG) void k_jpeg_idct(JdCall a)
{
    __shared__ int32_t ws[JD_IDCT_WG / 8][8][9];
    const uint32_t s = blockIdx.y;
    const int comps = jd_comps(a.info);
    const JcScratch sc = jc_scratch_of(a.scratch, a.W, a.H, comps, s);
    if (sc.hdr[0] != JC_NO_ERR) return;                        // the whole workgroup alike
    const mav_jpeg_info* I = a.info + s;
    JcGeom g;
    jc_geometry(I, &g);
    const uint32_t slot = threadIdx.x / 8, j = threadIdx.x % 8, blk = blockIdx.x * (JD_IDCT_WG / 8) + slot;
    const bool live = blk < jc_total_blocks(g);
    int c = 0;
    if (live && g.comps == 3) c = blk >= g.block0[2] ? 2 : blk >= g.block0[1] ? 1 : 0;
    int32_t v[8];
    if (live) {
        const uint4 raw = *(const uint4*)(sc.coef + (size_t)blk * 64 + j * 8);
        const uint2 q2 = *(const uint2*)(I->quant[I->comp[c].tq] + j * 8);
        const uint32_t cw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[2] = {q2.x, q2.y};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int32_t coef = (int16_t)(cw[k / 2] >> (16 * (k % 2)));
            ws[slot][j][k] = coef * (int32_t)((qw[k / 4] >> (8 * (k % 4))) & 255u);
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = ws[slot][r][j];
        jc_idct_pass(v, 11);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[slot][r][j] = v[r];     // the lane's own column
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = ws[slot][j][k];
        jc_idct_pass(v, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            lo |= (uint32_t)jc_clamp8(v[k] + 128) << (8 * k);
            hi |= (uint32_t)jc_clamp8(v[k + 4] + 128) << (8 * k);
        }
        const uint32_t local = blk - g.block0[c], by = local / (uint32_t)g.bw[c], bx = local % (uint32_t)g.bw[c];
        uint8_t* dst = sc.planes + (size_t)g.block0[c] * 64 + ((size_t)by * 8 + j) * ((size_t)g.bw[c] * 8) + (size_t)bx * 8;
        *(uint2*)dst = make_uint2(lo, hi);
    }
}

// grid: (ceil(ceil(W H / 4) / 256), count)
__global__ __launch_bounds__(JD_FINISH_WG) void k_jpeg_finish(JdCall a)
{
    const uint32_t s = blockIdx.y;
    const int comps = jd_comps(a.info);
    const JcScratch sc = jc_scratch_of(a.scratch, a.W, a.H, comps, s);
    const uint32_t err = sc.hdr[0];
    const int code = jc_verdict_code(err);
    if (blockIdx.x == 0 && threadIdx.x == 0) jc_verdict(a.status + s, err, sc.table, a.status[s].intervals);
    const int oc = jc_out_channels(comps, a.format);
    const size_t pixels = (size_t)a.W * a.H, p0 = ((size_t)blockIdx.x * JD_FINISH_WG + threadIdx.x) * 4;
    if (p0 >= pixels) return;
    const int n = pixels - p0 < 4 ? (int)(pixels - p0) : 4;
    uint8_t px[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!code) {
        JcGeom g;
        jc_geometry(a.info + s, &g);
        for (int i = 0; i < n; i++) jc_pixel(sc.planes, g, a.format, (int)((p0 + i) % (size_t)a.W), (int)((p0 + i) / (size_t)a.W), px + i * oc);
    }
    uint8_t* dst = a.out + (pixels * s + p0) * oc;
    if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
        for (int w = 0; w < oc; w++)
            ((uint32_t*)dst)[w] = (uint32_t)px[4 * w] | ((uint32_t)px[4 * w + 1] << 8) | ((uint32_t)px[4 * w + 2] << 16) | ((uint32_t)px[4 * w + 3] << 24);
    } else {
        for (int i = 0; i < n * oc; i++) dst[i] = px[i];
    }
}

// ---- host side: the entry points of include/mavflow_jpeg.h ------------------------------------------------------------------------------
#define JCHK(call) do { const int rc_ = (call); if (rc_ != MAV_OK) return rc_; } while (0)

extern "C" int mav_jpeg_parse(const uint8_t* file, size_t n, mav_jpeg_info* info)
{
    if (!file || !info) return ctx_fail(MAV_ERR_ARG, "mav_jpeg_parse: NULL %s", !file ? "file" : "info");
    char why[160];
    const int rc = jc_parse(file, n, info, why, sizeof why);
    return rc ? ctx_fail(rc, "mav_jpeg_parse: %s", why) : MAV_OK;
}
extern "C" size_t mav_jpeg_decode_scratch_bytes(int W, int H, int components, int count)
{
    return jc_shape_ok(W, H, components, count) ? (size_t)(jc_image_scratch(W, H, components) * (uint64_t)count) : 0;
}
extern "C" int mav_jpeg_decode_host(const uint8_t* file, size_t n, const mav_jpeg_info* info, int out_format, uint8_t* out, mav_jpeg_status* status)
{
    if (!file || !info || !out || !status)
        return ctx_fail(MAV_ERR_ARG, "mav_jpeg_decode_host: NULL %s", !file ? "file" : !info ? "info" : !out ? "out" : "status");
    if (out_format != MAV_JPEG_OUT_SAMPLES && out_format != MAV_JPEG_OUT_BGR && out_format != MAV_JPEG_OUT_GRAY)
        return ctx_fail(MAV_ERR_ARG, "mav_jpeg_decode_host: out_format %d is none of MAV_JPEG_OUT_*", out_format);
    if (jc_decode_host(file, n, info, out_format, out, status) != 0) return ctx_fail(MAV_ERR_OOM, "mav_jpeg_decode_host: no host memory for the coefficients");
    return MAV_OK;
}
static int jd_checked(mav_ctx* c, const void* files, const void* index, const void* info, int count, int W, int H, int out_format, const void* out,
                      const void* status, const char* fn)
{
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!files || !index || !info || !out || !status)
        return ctx_fail(MAV_ERR_ARG, "%s: NULL %s", fn, !files ? "files" : !index ? "index" : !info ? "info" : !out ? "out" : "status");
    if (count < 1 || count > MAV_JPEG_MAX_COUNT) return ctx_fail(MAV_ERR_ARG, "%s: count %d outside [1, %d]", fn, count, MAV_JPEG_MAX_COUNT);
    if (out_format != MAV_JPEG_OUT_SAMPLES && out_format != MAV_JPEG_OUT_BGR && out_format != MAV_JPEG_OUT_GRAY)
        return ctx_fail(MAV_ERR_ARG, "%s: out_format %d is none of MAV_JPEG_OUT_*", fn, out_format);
    if (!jc_shape_ok(W, H, 1, count)) return ctx_fail(MAV_ERR_ARG, "%s: an image of %d x %d is empty or larger than 65535", fn, W, H);
    return MAV_OK;
}
// the launches of one call
static int jd_launch(mav_ctx* c, const CtxView& v, const JdCall& a, const char* fn)
{
    const uint64_t full = jc_full_blocks(a.W, a.H);
    const unsigned units_x = (unsigned)(full < JD_MAX_UNITS_X ? full : JD_MAX_UNITS_X);
    const unsigned idct_x = (unsigned)((full * 3 + JD_IDCT_WG / 8 - 1) / (JD_IDCT_WG / 8));
    const unsigned finish_x = (unsigned)((((uint64_t)a.W * a.H + 3) / 4 + JD_FINISH_WG - 1) / JD_FINISH_WG);
    { JpegScope ps(c, 0); hipLaunchKernelGGL(k_jpeg_intervals, dim3(a.count), dim3(JD_SCAN_WG), 0, v.stream, a); }
    { JpegScope ps(c, 1); hipLaunchKernelGGL(k_jpeg_entropy, dim3(units_x, a.count), dim3(JD_WAVE), 0, v.stream, a); }
    { JpegScope ps(c, 2); hipLaunchKernelGGL(k_jpeg_idct, dim3(idct_x, a.count), dim3(JD_IDCT_WG), 0, v.stream, a); }
    { JpegScope ps(c, 3); hipLaunchKernelGGL(k_jpeg_finish, dim3(finish_x, a.count), dim3(JD_FINISH_WG), 0, v.stream, a); }
    (void)fn;
    return ctx_check_launch("jpeg_decode");
}
extern "C" int mav_jpeg_decode_dev(mav_ctx* c, const uint8_t* files, const uint64_t* index, const mav_jpeg_info* info, int count, int W, int H,
                                   int out_format, uint8_t* out, mav_jpeg_status* status, void* scratch)
{
    const char* fn = "mav_jpeg_decode_dev";
    JCHK(jd_checked(c, files, index, info, count, W, H, out_format, out, status, fn));
    if (!scratch) return ctx_fail(MAV_ERR_ARG, "%s: NULL scratch", fn);
    if ((uintptr_t)index % 8 || (uintptr_t)info % 8 || (uintptr_t)status % 8 || (uintptr_t)scratch % 16)
        return ctx_fail(MAV_ERR_ARG, "%s: index, info and status must be aligned to 8, scratch to 16", fn);
    CtxView v;
    JCHK(ctx_enter(c, 1, fn, &v));          // the count is the call's own: not bound by max_batch
    const JdCall a{files, index, info, count, W, H, out_format, out, status, scratch};
    return jd_launch(c, v, a, fn);
}
extern "C" int mav_jpeg_decode(mav_ctx* c, const uint8_t* files, const uint64_t* index, const mav_jpeg_info* info, int count, int W, int H,
                               int out_format, uint8_t* out, mav_jpeg_status* status)
{
    const char* fn = "mav_jpeg_decode";
    JCHK(jd_checked(c, files, index, info, count, W, H, out_format, out, status, fn));
    uint64_t bytes = 0;
    for (int i = 0; i < count; i++) {
        const uint64_t off = index[2 * i], n = index[2 * i + 1];
        if (off > (1ull << 40) || n > (1ull << 40)) return ctx_fail(MAV_ERR_ARG, "%s: file %d lies at offset %llu with %llu bytes", fn, i,
                                                                     (unsigned long long)off, (unsigned long long)n);
        if (off + n > bytes) bytes = off + n;
    }
    const int comps = jd_comps(info);
    StagedCall h(c, fn);
    CtxView v;
    JCHK(h.begin(1, &v));
    const uint8_t* df = (const uint8_t*)h.in(files, (size_t)(bytes ? bytes : 1));
    const uint64_t* di = (const uint64_t*)h.in(index, sizeof(uint64_t) * 2 * (size_t)count);
    const mav_jpeg_info* dinfo = (const mav_jpeg_info*)h.in(info, sizeof(mav_jpeg_info) * (size_t)count);
    uint8_t* dout = (uint8_t*)h.out(out, (size_t)W * H * jc_out_channels(comps, out_format) * count);
    mav_jpeg_status* dst = (mav_jpeg_status*)h.out(status, sizeof(mav_jpeg_status) * (size_t)count);
    void* scratch = h.scratch(mav_jpeg_decode_scratch_bytes(W, H, comps, count));
    JCHK(h.staged());
    const JdCall a{df, di, dinfo, count, W, H, out_format, dout, dst, scratch};
    JCHK(jd_launch(c, v, a, fn));
    return h.finish();
}
static_assert(sizeof(mav_jpeg_status) == 40, "mav_jpeg_status");
static_assert(sizeof(mav_jpeg_info) == 2512, "mav_jpeg_info");
static_assert(sizeof(mav_jpeg_huffman) == 272 && sizeof(mav_jpeg_component) == 8, "mav_jpeg_info's parts");

// The validation tail of the reference's loop on the device (include/mavflow_validation.h): MAV pixel count and raster-order list,
// get_simple_bounding_box, validate_sky_segment's counts, the sequential sum of the derotated ground-truth flow over the MAV.
// Compiled with -ffp-contract=off: the threshold products and the derotation are single IEEE operations in the order
// tests/validation_ref.py restates (src/processor.py:343-347, src/im_helpers.py:55-84,244-252, src/datasets/dataset.py:173-175,
// src/detector.py:70-117).
// Four phases, separate launches on the context's stream (the launches order them: no flag between workgroups; k_gts_init sets the
// accumulators before the first):
//   k_gts_max    max(seg), max(depth) as an order-preserving integer key, the NaN flag         -- integer atomics, one per workgroup
//   k_gts_count  per row (one wave each): MAV pixels, box test, depth > thr and the sky's counts  -- 64-bit atomics, one per workgroup
//   k_gts_list   per row: exclusive prefix of the row counts, ballot rank within the row          -- plain stores, disjoint
//   k_gts_finish per image (one workgroup): gather + derotate the listed pixels 1 024 at a time, two threads add them in order; the record
// Only integer atomics: every byte is the same on every run and at every batch position.
#include "mavflow_internal.h"
#include "../../include/mavflow_validation.h"

#include <limits.h>

__global__ void k_gts_init(GtsAcc* __restrict__ acc, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    GtsAcc a;
    a.drone = a.pos = a.tp = a.fp = 0ull;
    a.seg_max = 0; a.depth_key = 0u; a.nan = 0u; a.pad = 0;
    a.box[0] = a.box[1] = INT_MAX; a.box[2] = a.box[3] = -1;
    acc[b] = a;
}

// float -> unsigned, monotone: a < b  <=>  key(a) < key(b) for every pair of non-NaN floats (-0 below +0); no float has key 0
__device__ __forceinline__ unsigned depth_key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float depth_of_key(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// The fraction as given in decimal (include/mavflow_validation.h): the double nearest to the shortest n / 10^d that rounds to f.
__device__ __forceinline__ double fraction_as_given(float f)
{
    const double v = (double)f;
    double p = 1.0;
    for (int d = 1; d <= 9; d++) {
        p = p * 10.0;
        const double q = rint(v * p) / p;
        if ((float)q == f) return q;
    }
    return v;
}
__device__ __forceinline__ float depth_threshold(const mav_gt_stats_params* P, float dmax)
{
    if (P->flags & MAV_GT_STATS_THR_F64) return (float)(fraction_as_given(P->depth_fraction) * (double)dmax);
    return P->depth_fraction * dmax;
}
__device__ __forceinline__ float depth_max_of(const GtsAcc* a)
{
    return a->nan ? __uint_as_float(0x7FC00000u) : depth_of_key(a->depth_key);
}

// Workgroup = 256 threads over 256 consecutive pixels, grid-strided; blockIdx.z = the image.
__global__ __launch_bounds__(256) void k_gts_max(const uint8_t* __restrict__ seg, const float* __restrict__ depth, unsigned npx,
                                                 GtsAcc* __restrict__ acc)
{
    __shared__ int s_seg[4];
    __shared__ unsigned s_key[4], s_nan[4];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint8_t* sg = seg + (size_t)b * npx;
    const float* dp = depth ? depth + (size_t)b * npx : nullptr;
    int m = 0;
    unsigned key = 0u, nan = 0u;
    for (unsigned p = blockIdx.x * 256u + tid; p < npx; p += gridDim.x * 256u) {
        const int s = sg[p];
        m = s > m ? s : m;
        if (dp) {
            const float d = dp[p];
            if (d != d) nan = 1u;
            else { const unsigned k = depth_key(d); key = k > key ? k : key; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int m2 = __shfl_xor(m, o);
        const unsigned k2 = __shfl_xor(key, o);
        nan |= __shfl_xor(nan, o);
        m = m2 > m ? m2 : m;
        key = k2 > key ? k2 : key;
    }
    if (lane == 0) { s_seg[wv] = m; s_key[wv] = key; s_nan[wv] = nan; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) { m = s_seg[w] > m ? s_seg[w] : m; key = s_key[w] > key ? s_key[w] : key; nan |= s_nan[w]; }
        if (m > 0) atomicMax(&acc[b].seg_max, m);
        if (key) atomicMax(&acc[b].depth_key, key);
        if (nan) atomicOr(&acc[b].nan, 1u);
    }
}

// Workgroup = 4 waves, one image row each (row = 4 * blockIdx.x + wave), 64 pixels per step; blockIdx.z = the image.
__global__ __launch_bounds__(256) void k_gts_count(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ sky, const float* __restrict__ depth,
                                                   const mav_gt_stats_params* __restrict__ params, int W, int H, GtsAcc* acc,
                                                   int* __restrict__ rowcnt)
{
    __shared__ unsigned s_cnt[4][4];
    __shared__ int s_box[4][4];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = blockIdx.x * 4 + wv;
    const size_t npx = (size_t)W * H;
    const mav_gt_stats_params* P = params + b;
    const int seg_thr = P->seg_threshold;
    const double box_thr = P->box_fraction * (double)acc[b].seg_max;       // 0.1 * np.max(img): a float64 scalar
    const float thr = depth ? depth_threshold(P, depth_max_of(acc + b)) : 0.f;
    unsigned drone = 0u, pos = 0u, tp = 0u, fp = 0u;
    int x0 = INT_MAX, x1 = -1;
    if (y < H) {
        const uint8_t* sg = seg + (size_t)b * npx + (size_t)y * W;
        const uint8_t* sk = sky ? sky + (size_t)b * npx + (size_t)y * W : nullptr;
        const float* dp = depth ? depth + (size_t)b * npx + (size_t)y * W : nullptr;
        for (int x = lane; x < W; x += 64) {
            const int s = sg[x];
            drone += s > seg_thr;
            if ((double)s > box_thr) { x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; }
            if (dp) {
                const bool gt = dp[x] > thr, k = sk && sk[x] != 0;
                pos += gt; tp += gt && k; fp += !gt && k;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        drone += __shfl_xor(drone, o); pos += __shfl_xor(pos, o); tp += __shfl_xor(tp, o); fp += __shfl_xor(fp, o);
        const int a0 = __shfl_xor(x0, o), a1 = __shfl_xor(x1, o);
        x0 = a0 < x0 ? a0 : x0; x1 = a1 > x1 ? a1 : x1;
    }
    if (lane == 0) {
        if (y < H) rowcnt[(size_t)b * H + y] = (int)drone;
        s_cnt[wv][0] = drone; s_cnt[wv][1] = pos; s_cnt[wv][2] = tp; s_cnt[wv][3] = fp;
        const bool any = x1 >= 0;
        s_box[wv][0] = x0; s_box[wv][1] = any ? y : INT_MAX; s_box[wv][2] = x1; s_box[wv][3] = any ? y : -1;
    }
    __syncthreads();
    if (tid < 4) {
        const unsigned long long v = (unsigned long long)s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        unsigned long long* dst = tid == 0 ? &acc[b].drone : tid == 1 ? &acc[b].pos : tid == 2 ? &acc[b].tp : &acc[b].fp;
        if (v) atomicAdd(dst, v);
    } else if (tid < 8) {
        const int k = tid - 4;
        int v = s_box[0][k];
        for (int w = 1; w < 4; w++) v = k < 2 ? (s_box[w][k] < v ? s_box[w][k] : v) : (s_box[w][k] > v ? s_box[w][k] : v);
        if (k < 2) { if (v != INT_MAX) atomicMin(&acc[b].box[k], v); }
        else if (v >= 0) atomicMax(&acc[b].box[k], v);
    }
}

// The same rows.  A row's first list position is the sum of the counts of the rows above it; within the row a pixel's rank is the number
// of MAV pixels in the lower lanes of its 64-pixel step (ballot + popcount) on top of the steps before.  Positions >= max_pixels are
// not written.  The launch's threads also put -1 into the entries behind the list.
__global__ __launch_bounds__(256) void k_gts_list(const uint8_t* __restrict__ seg, const mav_gt_stats_params* __restrict__ params, int W, int H,
                                                  int max_pixels, const GtsAcc* __restrict__ acc, const int* __restrict__ rowcnt,
                                                  int32_t* __restrict__ list)
{
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = blockIdx.x * 4 + wv;
    const size_t npx = (size_t)W * H;
    int32_t* out = list + (size_t)b * max_pixels;
    const unsigned long long total = acc[b].drone;
    const int listed = total < (unsigned long long)max_pixels ? (int)total : max_pixels;
    for (long long i = (long long)listed + (long long)blockIdx.x * 256 + tid; i < max_pixels; i += (long long)gridDim.x * 256) out[i] = -1;
    if (y >= H) return;
    const int* rc = rowcnt + (size_t)b * H;
    const int mine = rc[y];
    if (mine == 0) return;                                         // (wave-uniform)
    long long above = 0;
    for (int r = lane; r < y; r += 64) above += rc[r];
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
    if (above >= max_pixels) return;
    const int seg_thr = params[b].seg_threshold;
    const uint8_t* sg = seg + (size_t)b * npx + (size_t)y * W;
    long long base = above;
    for (int xb = 0; xb < W && base < max_pixels; xb += 64) {      // (wave-uniform bounds: every lane reaches the ballot)
        const int x = xb + lane;
        const bool mav = x < W && sg[x] > seg_thr;
        const unsigned long long m = __ballot(mav);
        const long long at = base + __popcll(m & ((1ull << lane) - 1ull));
        if (mav && at < max_pixels) out[at] = y * W + x;
        base += __popcll(m);
    }
}

// One workgroup per image: the record, and before it the flow sum.  GTS_SUM_STEP listed pixels at a time are gathered and derotated by
// the threads into LDS (two dependent global loads per step: the index, then the vector -- the step is wide so that their latency is
// paid once per 1 024 pixels); thread 0 then adds the u values, thread 1 the v values, in list order, 64 LDS reads issued together
// in front of each run of 64 adds.
#define GTS_SUM_STEP 1024
__global__ __launch_bounds__(GTS_SUM_STEP) void k_gts_finish(const float* __restrict__ gt_flow, const mav_gt_stats_params* __restrict__ params, int W,
                                                             int H, int max_pixels, int has_depth, const GtsAcc* __restrict__ acc,
                                                             const int32_t* __restrict__ list, mav_gt_stats_record* __restrict__ records)
{
    __shared__ double s_val[2][GTS_SUM_STEP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t npx = (size_t)W * H;
    const mav_gt_stats_params* P = params + b;
    const GtsAcc a = acc[b];
    const bool truncated = a.drone > (unsigned long long)max_pixels;
    const int listed = truncated ? max_pixels : (int)a.drone;
    double sum = 0.0;
    if (gt_flow && list && !truncated && listed > 0) {              // (uniform over the workgroup: every thread reaches the barriers)
        const bool frame0 = (P->flags & MAV_GT_STATS_FRAME0) != 0;
        DerotParams dp;
        dp.o0 = P->omega[0]; dp.o1 = P->omega[1]; dp.o2 = P->omega[2];
        dp.sx = W * P->dt / 2;                                     // w * dt / 2 (detector.py:100-101)
        dp.sy = H * P->dt / 2;
        dp.mode = frame0 ? MAV_PAIR_FRAME0 : MAV_PAIR_DEROTATE;
        const float2* g = (const float2*)gt_flow + (size_t)b * npx;
        const int32_t* idx = list + (size_t)b * max_pixels;
        float sum32 = 0.f;
        for (int k0 = 0; k0 < listed; k0 += GTS_SUM_STEP) {
            const int n = listed - k0 < GTS_SUM_STEP ? listed - k0 : GTS_SUM_STEP;
            if (tid < n) {
                const int p = idx[k0 + tid];
                const int row = p / W, col = p - row * W;
                double u, v;
                derot_apply(g[p], &dp, W, H, row, col, &u, &v);  // FRAME0: the float32 values, promoted exactly
                s_val[0][tid] = u; s_val[1][tid] = v;
            }
            __syncthreads();
            if (tid < 2) {
                const double* val = s_val[tid];
                int k = 0;
                if (frame0) for (; k < n; k++) sum32 = sum32 + (float)val[k];
                else {
                    for (; k + 64 <= n; k += 64) {
#pragma unroll
                        for (int j = 0; j < 64; j++) sum = sum + val[k + j];
                    }
                    for (; k < n; k++) sum = sum + val[k];
                }
            }
            __syncthreads();
        }
        if (frame0) sum = (double)sum32;
    }
    const double s1 = __shfl(sum, 1);                               // (wave 0: thread 1's sum to thread 0)
    if (tid == 0) {
        mav_gt_stats_record r;
        r.drone_pixels = (int64_t)a.drone;
        r.sky[0] = has_depth ? (int64_t)a.pos : 0;
        r.sky[1] = has_depth ? (int64_t)(npx - a.pos) : 0;
        r.sky[2] = (int64_t)a.tp;
        r.sky[3] = (int64_t)a.fp;
        r.flow_sum[0] = sum; r.flow_sum[1] = s1;
        const bool any = a.box[2] >= 0;
        r.box[0] = any ? a.box[0] : -1; r.box[1] = any ? a.box[1] : -1; r.box[2] = a.box[2]; r.box[3] = a.box[3];
        r.seg_max = a.seg_max;
        r.listed = listed;
        r.depth_max = has_depth ? depth_max_of(&a) : 0.f;
        r.flags = (truncated ? MAV_GT_STATS_TRUNCATED : 0u) | (a.nan ? MAV_GT_STATS_DEPTH_NAN : 0u);
        r.pad[0] = r.pad[1] = 0u;
        records[b] = r;
    }
}

size_t gt_stats_scratch_bytes(int B, int H, int max_pixels, bool own_list)
{
    return gts_list_offset(B, H) + (own_list ? sizeof(int32_t) * (size_t)B * max_pixels : 0);
}
void launch_gt_stats_phase(hipStream_t st, int phase, const GtStatsCall& k)
{
    const mav_gt_stats_params* params = (const mav_gt_stats_params*)k.params;
    GtsAcc* acc = (GtsAcc*)k.scratch;
    int* rowcnt = (int*)((char*)k.scratch + gts_rows_offset(k.B));
    int32_t* list = k.indices ? k.indices : k.gt_flow ? (int32_t*)((char*)k.scratch + gts_list_offset(k.B, k.H)) : nullptr;
    const size_t npx = (size_t)k.W * k.H;
    const size_t nblk = (npx + 255) / 256;
    const dim3 rows((unsigned)((k.H + 3) / 4), 1, k.B);
    switch (phase) {
    case GTS_PHASE_MAX:
        hipLaunchKernelGGL(k_gts_init, dim3((k.B + 63) / 64), dim3(64), 0, st, acc, k.B);
        hipLaunchKernelGGL(k_gts_max, dim3((unsigned)(nblk < MAV_GT_STATS_GRID_CAP ? nblk : MAV_GT_STATS_GRID_CAP), 1, k.B), dim3(256), 0, st, k.seg,
                           k.depth, (unsigned)npx, acc);
        break;
    case GTS_PHASE_COUNT:
        hipLaunchKernelGGL(k_gts_count, rows, dim3(256), 0, st, k.seg, k.sky, k.depth, params, k.W, k.H, acc, rowcnt);
        break;
    case GTS_PHASE_LIST:
        if (list) hipLaunchKernelGGL(k_gts_list, rows, dim3(256), 0, st, k.seg, params, k.W, k.H, k.max_pixels, acc, rowcnt, list);
        break;
    case GTS_PHASE_SUM:
        hipLaunchKernelGGL(k_gts_finish, dim3(k.B), dim3(GTS_SUM_STEP), 0, st, k.gt_flow, params, k.W, k.H, k.max_pixels, k.depth ? 1 : 0, acc, list,
                           (mav_gt_stats_record*)k.records);
        break;
    }
}

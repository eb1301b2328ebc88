// Detection kernels for gfx950: derotation, FoE candidates + RANSAC vote, phi + threshold masks + box, and the
// small reductions around them.  Compiled with -ffp-contract=off: every double operation below is written in the
// reference's numpy evaluation order so results are bit-identical to
//   /root/reference/src/detector.py:70-117            (derotate)
//   /root/reference/src/focus_of_expansion.py:32-86   (get_FOE_dense, ransac; utils.py:183-197 line_intersection)
//   /root/reference/src/focus_of_expansion.py:150-184 (get_phi)
//   /root/reference/src/processor.py:333-341          (threshold block)
//   /root/reference/src/im_helpers.py:55-84,244-252   (get_simple_bounding_box, calculate_tpr_fpr)
//   /root/reference/src/detector.py:280-312           (analyze_pyramid, level 0)
// with one documented exception: arccos comes from the device math library, not the host's libm.
#include "mavflow_internal.h"

#include <limits.h>
#include <algorithm>
#include <math.h>

#include <type_traits>

// derot_apply (the derotated flow vector at a pixel, reference operation order) is in mavflow_internal.h: kernels_validation.hip uses it too.
static __device__ __forceinline__ float2 flow_raw(const float* __restrict__ flow, int W, int row, int col)
{
    return *(const float2*)(flow + ((size_t)row * W + col) * 2);
}
static __device__ __forceinline__ double2 flow_raw(const double* __restrict__ flow, int W, int row, int col)
{
    return *(const double2*)(flow + ((size_t)row * W + col) * 2);
}
template <typename FlowT>
static __device__ __forceinline__ void flow_at(const FlowT* __restrict__ flow, const DerotParams* __restrict__ dp, int W, int H,
                                               int row, int col, double* fu, double* fv)
{
    derot_apply(flow_raw(flow, W, row, col), dp, W, H, row, col, fu, fv);
}

__global__ __launch_bounds__(256) void k_derotate(const float* __restrict__ flow, const DerotParams* __restrict__ derot, int W,
                                                  int H, double* __restrict__ out)
{
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t img = (size_t)W * H * 2;
    double u, v;
    flow_at(flow + b * img, derot + b, W, H, y, x, &u, &v);
    *(double2*)(out + b * img + ((size_t)y * W + x) * 2) = make_double2(u, v);
}

void launch_derotate(hipStream_t st, const float* flow, const DerotParams* derot, int B, int W, int H, double* out)
{
    dim3 grid((W + 63) / 64, (H + 3) / 4, B);
    hipLaunchKernelGGL(k_derotate, grid, dim3(256), 0, st, flow, derot, W, H, out);
}

// ------------------------------------------------------------------------------------------------------------
// FoE candidates: one 1024-thread workgroup per pair.  Thread i intersects the flow lines through samples i and
// i+N; surviving rows (x != 0.0) are compacted IN INDEX ORDER (ballot + wave prefix) because RANSAC's tie-break
// is "first candidate wins".
// ------------------------------------------------------------------------------------------------------------
template <typename FlowT>
__global__ __launch_bounds__(1024) void k_foe_candidates(const FlowT* __restrict__ flow, const DerotParams* __restrict__ derot,
                                                         const uint32_t* __restrict__ samples, int W, int H, int N,
                                                         double mag2_thr, float mag2_thr_f32, FoeScratch sc,
                                                         int32_t* __restrict__ box_acc, unsigned long long* __restrict__ max_phi_bits)
{
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t img = (size_t)W * H * 2;
    const FlowT* fl = flow + b * img;
    const DerotParams* dp = derot ? derot + b : nullptr;
    // frame-0 pair (float32 flow handed to numpy as is): only the |flow2| gate runs in float32 there -- `flow + coord` is
    // float32 + uint32 = float64, so the intersections below are the same double arithmetic either way
    const bool f32_gate = std::is_same<FlowT, float>::value && dp && dp->mode == MAV_PAIR_FRAME0;
    const uint32_t* smp = samples + (size_t)b * 4 * N;
    double* cand = sc.cand + (size_t)b * 2 * N;
    if (tid == 0) {
        base_s = 0; sc.best_key[b] = 0ull;
        sc.done[2 * b] = 0u; sc.done[2 * b + 1] = 0u;           // tickets of the vote and of the phi kernel (both run after this one)
        if (box_acc) { box_acc[4 * b] = INT_MAX; box_acc[4 * b + 1] = INT_MAX; box_acc[4 * b + 2] = -1; box_acc[4 * b + 3] = -1; }
        if (max_phi_bits) max_phi_bits[b] = 0ull;
    }
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        double ix = 0.0, iy = 0.0;
        if (i < N) {
            const uint32_t r1 = smp[2 * i], c1 = smp[2 * i + 1];
            const uint32_t r2 = smp[2 * (i + N)], c2 = smp[2 * (i + N) + 1];
            if (r1 < (uint32_t)H && r2 < (uint32_t)H && c1 < (uint32_t)W && c2 < (uint32_t)W) {
                double f1x, f1y, f2x, f2y;
                flow_at(fl, dp, W, H, (int)r1, (int)c1, &f1x, &f1y);
                flow_at(fl, dp, W, H, (int)r2, (int)c2, &f2x, &f2y);
                const double mag2 = f2x * f2x + f2y * f2y;
                bool below = mag2 < mag2_thr;      // == sqrt(mag2) < mag_threshold, see sq_threshold() on the host
                if (f32_gate) {                    // np.linalg.norm of a float32 pair: float32 products, sum and root
                    const float gx = (float)f2x, gy = (float)f2y;
                    const float m2 = gx * gx + gy * gy;
                    below = m2 < mag2_thr_f32;
                }
                if (!below) {
                    const double p1x = (double)c1, p1y = (double)r1, p2x = (double)c2, p2y = (double)r2;
                    const double q1x = f1x + p1x, q1y = f1y + p1y, q2x = f2x + p2x, q2y = f2y + p2y;
                    const double xd0 = p1x - q1x, xd1 = p2x - q2x, yd0 = p1y - q1y, yd1 = p2y - q2y;
                    const double div = xd0 * yd1 - xd1 * yd0;
                    if (!(div == 0.0)) {
                        const double d0 = p1x * q1y - p1y * q1x;
                        const double d1 = p2x * q2y - p2y * q2x;
                        ix = (d0 * xd1 - d1 * xd0) / div;
                        iy = (d0 * yd1 - d1 * yd0) / div;
                        keep = (ix != 0.0);
                    }
                }
            }
        }
        const unsigned long long bal = __ballot(keep);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wv] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int k = 0; k < wv; k++) off += wave_tot[k];
        if (keep) {
            cand[2 * (off + pre)] = ix;
            cand[2 * (off + pre) + 1] = iy;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int k = 0; k < 16; k++) t += wave_tot[k];
            base_s += t;
        }
        __syncthreads();
    }
    if (tid == 0) sc.count[b] = base_s;
}

// RANSAC vote: score_i = #{j : |e_j - e_i| < r} - 1; winner = largest score, lowest index (strict > in the loop).
// One WAVE scores four candidates against all M: its lanes stride over j (one coalesced double2 load feeds the four tests), the
// counts are reduced over the wave.  Grid (ceil(N/16), B).  (Round 2's form -- one THREAD per candidate, 4 workgroups per pair --
// took 23 us for a single pair: a thousand dependent LDS reads per thread.)  The workgroup whose ticket is last reads the winner
// and writes the pair's FoE: no separate finalize launch.  Every workgroup's atomicMax has returned before its ticket is drawn.
__global__ __launch_bounds__(256) void k_ransac(FoeScratch sc, int N, double dist2_thr, double* __restrict__ foe)
{
    __shared__ unsigned long long wkey[4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int M = sc.count[b];
    const double2* cand = (const double2*)(sc.cand + (size_t)b * 2 * N);
    const int i0 = ((int)blockIdx.x * 4 + wv) * 4;
    unsigned long long key = 0ull;
    if (i0 < M) {
        double2 e[4];
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) e[k] = cand[min(i0 + k, M - 1)];
        for (int j = lane; j < M; j += 64) {
            const double2 c = cand[j];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double dx = c.x - e[k].x, dy = c.y - e[k].y;
                const double d2 = dx * dx + dy * dy;
                cnt[k] += (d2 < dist2_thr) ? 1 : 0;  // == (sqrt(d2) < ransac_threshold)
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o);
            const int score = cnt[k] - 1;
            if (i0 + k < M && score > 0) {
                const unsigned long long kk = ((unsigned long long)(unsigned)score << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(i0 + k));
                key = kk > key ? kk : key;
            }
        }
    }
    if (lane == 0) wkey[wv] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < 4; k++) key = wkey[k] > key ? wkey[k] : key;
        unsigned long long seen = 0ull;
        if (key) seen = atomicMax(&sc.best_key[b], key);              // returning form: performed before the ticket below
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(seen) : "memory");
        const unsigned ticket = atomicAdd(&sc.done[2 * b], 1u);
        if (ticket == gridDim.x - 1) {
            const unsigned long long best = __hip_atomic_load(&sc.best_key[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            double x = 0.0, y = 0.0;
            if (best) {
                const unsigned idx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
                x = sc.cand[(size_t)b * 2 * N + 2 * idx];
                y = sc.cand[(size_t)b * 2 * N + 2 * idx + 1];
            }
            foe[2 * b] = x;
            foe[2 * b + 1] = y;
            __hip_atomic_store(&sc.done[2 * b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <typename FlowT>
static void launch_foe_t(hipStream_t st, const FlowT* flow, const DerotParams* derot, const uint32_t* samples, int B, int W,
                         int H, int N, double mag2_thr, float mag2_thr_f32, double dist2_thr, FoeScratch s, double* foe,
                         int32_t* box_acc, unsigned long long* max_phi_bits)
{
    hipLaunchKernelGGL(k_foe_candidates<FlowT>, dim3(B), dim3(1024), 0, st, flow, derot, samples, W, H, N, mag2_thr, mag2_thr_f32, s,
                       box_acc, max_phi_bits);
    hipLaunchKernelGGL(k_ransac, dim3((N + 15) / 16, B), dim3(256), 0, st, s, N, dist2_thr, foe);
}
void launch_foe_f32(hipStream_t st, const float* flow, const DerotParams* derot, const uint32_t* samples, int B, int W, int H,
                    int N, double mag2_thr, float mag2_thr_f32, double dist2_thr, FoeScratch s, double* foe, int32_t* box_acc,
                    unsigned long long* max_phi_bits)
{
    launch_foe_t<float>(st, flow, derot, samples, B, W, H, N, mag2_thr, mag2_thr_f32, dist2_thr, s, foe, box_acc, max_phi_bits);
}
void launch_foe_f64(hipStream_t st, const double* flow, const uint32_t* samples, int B, int W, int H, int N, double mag2_thr,
                    double dist2_thr, FoeScratch s, double* foe, int32_t* box_acc, unsigned long long* max_phi_bits)
{
    launch_foe_t<double>(st, flow, nullptr, samples, B, W, H, N, mag2_thr, 0.f, dist2_thr, s, foe, box_acc, max_phi_bits);
}

// ------------------------------------------------------------------------------------------------------------
// phi + both threshold masks + box extents + max(phi), one pass over the flow.  Workgroup = 4 rows x 256 columns,
// lane-contiguous float2/double2 loads; box extents and max(phi) are reduced per wave, then one atomic per wave.
// ------------------------------------------------------------------------------------------------------------
__global__ void k_box_init(int32_t* box_acc, unsigned long long* max_phi_bits, unsigned* done, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    box_acc[4 * b] = INT_MAX; box_acc[4 * b + 1] = INT_MAX; box_acc[4 * b + 2] = -1; box_acc[4 * b + 3] = -1;
    if (max_phi_bits) max_phi_bits[b] = 0ull;
    if (done) done[2 * b + 1] = 0u;
}
// (the fused chain needs no such launch: k_foe_candidates initialises its pair's accumulators)
void launch_box_init(hipStream_t st, int32_t* box_acc, unsigned long long* max_phi_bits, unsigned* done, int B)
{
    hipLaunchKernelGGL(k_box_init, dim3((B + 63) / 64), dim3(64), 0, st, box_acc, max_phi_bits, done, B);
}

// Box extents of one wave -> the pair's accumulators.  The accumulators only ever grow, so a (possibly stale) read that
// already contains this wave's extents makes the four same-address atomics unnecessary: after the first few waves of a
// pair almost every wave skips them (they were the phi kernel's bottleneck: thousands of atomics on four words).
static __device__ __forceinline__ void wave_box_commit(int x0, int y0, int x1, int y1, int32_t* acc)
{
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o));
    }
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        const int c0 = __hip_atomic_load(&acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c1 = __hip_atomic_load(&acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c2 = __hip_atomic_load(&acc[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c3 = __hip_atomic_load(&acc[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // returning atomics whose results are waited for: when the workgroup draws its ticket (k_phi_mask's tail) they have been performed
        int seen = 0;
        if (x0 < c0) seen |= atomicMin(&acc[0], x0);
        if (y0 < c1) seen |= atomicMin(&acc[1], y0);
        if (x1 > c2) seen |= atomicMax(&acc[2], x1);
        if (y1 > c3) seen |= atomicMax(&acc[3], y1);
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(seen) : "memory");
    }
}

// Screening constants for the single-precision fast path (host-computed, see phi_screen()).
struct PhiScreen {
    int enabled;         // 0: every pixel takes the exact double path
    float tan_fixed;     // tan(fixed_deg), fixed_deg in (0, 80)
    float margin_fixed;  // MAV_SCREEN_TAN_MARGIN * (1 + tan_fixed)
    float fmm2, dmm2;    // fixed_min_mag^2, dyn_min_mag^2
    float dyn_ab, dyn_c; // dyn_a + dyn_b, dyn_c
};
#define MAV_SCREEN_TAN_MAX_DEG 17.0f     // the degree-9 series of tan below is good to 5e-8 relative up to 0.2967 rad
#define MAV_SCREEN_TAN_MARGIN 4e-6f      // decision margin, in units of |flow| * |p - FoE| * (1 + tan T); error bound 1.2e-6

// Exact phi of one pixel (degrees), numpy order of operations (focus_of_expansion.py:163-177).
static __device__ __forceinline__ double phi_exact(double u, double v, double d2x, double d2y, double* fm_out)
{
    const double fm = sqrt(u * u + v * v);
    const double dist = sqrt(d2x * d2x + d2y * d2y);
    const double prod = fm * dist;
    const double norm = (prod > 1e-6 || prod != prod) ? prod : 1e-6;  // np.maximum propagates NaN
    double arg = (u * d2x + v * d2y) / norm;
    *fm_out = fm;
    if (arg != arg) return 0.0;  // angle_diff[isnan] = 0
    arg = arg < -1.0 ? -1.0 : (arg > 1.0 ? 1.0 : arg);
    return acos(arg) * (180.0 / 3.141592653589793238462643383279502884);
}

// Single-precision screen of one pixel of the phi / mask stage.  Returns true when both verdicts are certain (then *fix_out /
// *dyn_out hold them); false sends the pixel to phi_pixel_exact().  For a threshold T below 90 degrees
//     phi > T   <=>   dot <= 0  or  |cross| > tan(T) * dot        (dot = f . d, cross = f x d, d = p - FoE),
// and this form is well conditioned exactly where the thresholds live (a few degrees): in float32 dot and |cross| are each
// within 4.2e-7 S of their exact values (S = |f| |d|), tan(T) within 6.5e-7 relative, so  r = |cross| - tan(T) dot  is within
// 1.2e-6 S (1 + tan T) of its exact value and its sign is the exact path's verdict whenever |r| exceeds the 4e-6 margin: an
// angular band of ~2e-4 degrees, ~1e-5 of the pixels.  (The arccos-argument form of round 1, arg < cos T with a 1e-4 band, is
// ill conditioned at small T -- d arg = sin T dT -- and sent every pixel within ~0.15 degrees of a 2-degree threshold down the
// double path.)  tan(T) of the dynamic threshold T = dyn_a + dyn_b + dyn_c / |f| comes from the degree-9 series, good to 5e-8
// relative up to 17 degrees (every |f| >= 0.5 with the reference's constants); larger dynamic thresholds go to the exact path.
// Magnitude gates: 1e-5 relative around both.  Branch-free, explicit FMAs (this file is built with -ffp-contract=off): the
// kernel is instruction-bound (PMC: 10 % of its cycles waiting on memory), so every instruction here is paid 133 M times a step.
static __device__ __forceinline__ bool phi_pixel_screen(float uf, float vf, float dxf, float dyf, bool notsky, const PhiScreen& scr,
                                                        bool* fix_out, bool* dyn_out)
{
    const float m2 = fmaf(uf, uf, vf * vf), dd = fmaf(dxf, dxf, dyf * dyf);
    const float prod2 = m2 * dd;
    const float dot = fmaf(uf, dxf, vf * dyf);
    const float crs = fabsf(fmaf(uf, dyf, -(vf * dxf)));
    const float S = __builtin_amdgcn_sqrtf(prod2);            // raw v_sqrt_f32 (1 ulp): S only scales the margins
    // norm floor (1e-6), inf / NaN and the two magnitude gates' bands stay on the exact path
    const bool ok = (int)(prod2 > 1e-8f) & (int)(prod2 < 1e30f) & (int)(fabsf(m2 - scr.fmm2) > 1e-5f * scr.fmm2) & (int)(fabsf(m2 - scr.dmm2) > 1e-5f * scr.dmm2);
    const bool act_f = (m2 > scr.fmm2) & notsky, act_d = (m2 > scr.dmm2) & notsky;
    const float rf = fmaf(-scr.tan_fixed, dot, crs);
    const bool ok_f = fabsf(rf) > scr.margin_fixed * S;
    const float T = fmaf(scr.dyn_c, __builtin_amdgcn_rsqf(m2), scr.dyn_ab);      // degrees, >= 0; raw v_rsq_f32 (1 ulp, in the budget)
    const float x = T * 0.017453292519943295f, x2 = x * x;
    const float tT = x * fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, 0.02186948854f, 0.05396825397f), 0.13333333333f), 0.33333333333f), 1.f);
    const float rd = fmaf(-tT, dot, crs);
    const bool ok_d = (T < MAV_SCREEN_TAN_MAX_DEG) & (fabsf(rd) > MAV_SCREEN_TAN_MARGIN * fmaf(S, tT, S));
    *fix_out = act_f & (rf > 0.f);
    *dyn_out = act_d & (rd > 0.f);
    return ok & (!act_f | ok_f) & (!act_d | ok_d);
}

// The exact path of one pixel: double arithmetic in numpy's order (phi_exact) and the literal threshold block.  Out of line on
// purpose: only ~1e-5 of the pixels come here when the screen is on, and sixteen inlined copies of the double sqrt / divide /
// acos sequences made the kernel 69 KB of code -- more than the instruction cache two CUs share.
// (everything by value, result in registers: no stack frame, the kernel needs no scratch memory)
struct PhiVerdict { double ph; unsigned bits; };     // bits: 1 = fixed mask, 2 = dynamic mask
static __device__ __noinline__ PhiVerdict phi_pixel_exact(double u, double v, double d2x, double d2y, int notsky, double fixed_deg,
                                                          double fixed_min_mag, double dyn_min_mag, double dyn_a, double dyn_b,
                                                          double dyn_c)
{
    double fm;
    const double ph = phi_exact(u, v, d2x, d2y, &fm);
    const double t = dyn_b + dyn_c / fm;
    const bool hi = ph > (dyn_a + t);
    const bool lo = ph < (dyn_a - t);
    const bool dyn = (fm > dyn_min_mag) && notsky && (lo || hi);
    const double gated = ((fm > fixed_min_mag) && notsky) ? ph : 0.0;
    return PhiVerdict{ph, (gated > fixed_deg ? 1u : 0u) | (dyn ? 2u : 0u)};
}

// One pixel of a frame-0 pair: get_phi (focus_of_expansion.py:163-177) and the threshold block (processor.py:333-341) as numpy
// evaluates them on a FLOAT32 flow array -- zeros_like keeps diff2 in float32 (the int64 - float64 coordinate difference is
// rounded into it), np.linalg.norm, the products, the quotient and the thresholds (8 / mag, 0.5 + ..., 0.25 + ...) are all
// float32 operations, rad2deg multiplies by 180f / pif.  No contraction (this file is built with -ffp-contract=off).
// arccos: the correctly rounded float32 value (double acos, rounded once).
struct ThrF32 { float fixed_deg, fixed_min_mag, dyn_min_mag, dyn_a, dyn_b, dyn_c; };
static __device__ __noinline__ PhiVerdict phi_pixel_f32(float u, float v, float d2x, float d2y, int notsky, float fixed_deg,
                                                        float fixed_min_mag, float dyn_min_mag, float dyn_a, float dyn_b, float dyn_c)
{
    const ThrF32 t{fixed_deg, fixed_min_mag, dyn_min_mag, dyn_a, dyn_b, dyn_c};
    const float fm = sqrtf(u * u + v * v);
    const float dist = sqrtf(d2x * d2x + d2y * d2y);
    const float prod = fm * dist;
    const float norm = (prod > 1e-6f || prod != prod) ? prod : 1e-6f;      // np.maximum propagates NaN
    float arg = (u * d2x + v * d2y) / norm;
    float ph = 0.f;                                                         // angle_diff[isnan] = 0
    if (arg == arg) {
        arg = arg < -1.f ? -1.f : (arg > 1.f ? 1.f : arg);
        ph = (float)acos((double)arg) * __int_as_float(0x42652EE0);         // 180.0f / 3.14159274f
    }
    const float tt = t.dyn_b + t.dyn_c / fm;
    const bool hi = ph > (t.dyn_a + tt);
    const bool lo = ph < (t.dyn_a - tt);
    const bool dyn = (fm > t.dyn_min_mag) && notsky && (lo || hi);
    const float gated = ((fm > t.fixed_min_mag) && notsky) ? ph : 0.f;
    return PhiVerdict{(double)ph, (gated > t.fixed_deg ? 1u : 0u) | (dyn ? 2u : 0u)};
}

// VEC = 4: one thread = 4 consecutive pixels x 4 rows (W % 4 == 0): float4 / double2 row loads, uchar4 mask stores;
// workgroup = 256 columns x 16 rows.  VEC = 1: any width, one pixel per lane and row, 4 rows per thread.
// ROT = false: the launch carries no per-pair parameters (no rates, no frame-0 pair): pass 1 has no derotation code at all.
template <typename FlowT, int VEC, bool ROT>
__global__ __launch_bounds__(256) void k_phi_mask(const FlowT* __restrict__ flow, const DerotParams* __restrict__ derot,
                                                  const double* __restrict__ foe, const uint8_t* __restrict__ sky, int W, int H,
                                                  mav_thr_params thr, PhiScreen scr, double* __restrict__ phi_out,
                                                  uint8_t* __restrict__ mfix, uint8_t* __restrict__ mdyn,
                                                  int32_t* __restrict__ box_acc, unsigned long long* __restrict__ max_phi_bits,
                                                  unsigned* __restrict__ done, mav_result* __restrict__ results,
                                                  int32_t* __restrict__ box_out)
{
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t npx = (size_t)W * H;
    const FlowT* fl = flow + b * npx * 2;
    const DerotParams* dp = (ROT && derot) ? derot + b : nullptr;
    const bool f32_pair = ROT && std::is_same<FlowT, float>::value && dp && dp->mode == MAV_PAIR_FRAME0;
    const double foex = foe[2 * b], foey = foe[2 * b + 1];
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    double pmax = 0.0;
    const int xb = (blockIdx.x * 64 + lane) * VEC;
    const bool colok = xb < W;                            // lanes past the right edge stay for the wave reductions below
    const int xld = colok ? xb : 0;
    // a workgroup walks every gridDim.y-th block of 16 rows: fewer, longer-lived waves (the launch is wave-launch bound otherwise)
    for (int yblk = blockIdx.y; yblk * 16 < H; yblk += gridDim.y) {
    const int yb = yblk * 16 + wv * 4;
    // Pass 1 (every pixel, compact straight-line code): all flow vectors and sky words of the thread are requested up front, then
    // each pixel is screened in float32; bit 4r + j of fixb / dynb holds its verdicts, of `todo` that it still needs the exact path
    // (inside a guard band, derotated, screen off, or a frame-0 pair).
    decltype(flow_raw(fl, W, 0, 0)) raw[4][VEC];
    uint32_t skw[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int yc = min(yb + r, H - 1);                // rows past the bottom: re-read the last row, never stored
#pragma unroll
        for (int j = 0; j < VEC; j++) raw[r][j] = flow_raw(fl, W, yc, xld + j);
        const size_t oc = b * npx + (size_t)yc * W + xld;
        skw[r] = !sky ? 0u : (VEC == 4 ? *(const uint32_t*)(sky + oc) : (uint32_t)sky[oc]);
    }
    unsigned fixb = 0u, dynb = 0u, todo = 0u;
    const bool screen = scr.enabled && !f32_pair;
    float dxf[VEC], dyf[4];                               // p - FoE: formed in double as the exact path does, then rounded once
#pragma unroll
    for (int j = 0; j < VEC; j++) dxf[j] = (float)((double)(xb + j) - foex);
#pragma unroll
    for (int r = 0; r < 4; r++) dyf[r] = (float)((double)(yb + r) - foey);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (yb + r >= H || !colok) continue;
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const unsigned bit = 1u << (4 * r + j);
            const bool notsky = ((skw[r] >> (8 * j)) & 255u) == 0u;
            bool fix = false, dyn = false, sure = false;
            if (screen) {
                float uf = (float)raw[r][j].x, vf = (float)raw[r][j].y;
                if constexpr (ROT) {                      // derotation (a wave-uniform branch) in double, then the float32 screen
                    double u, v;
                    derot_apply(raw[r][j], dp, W, H, yb + r, xb + j, &u, &v);
                    uf = (float)u; vf = (float)v;
                }
                sure = phi_pixel_screen(uf, vf, dxf[j], dyf[r], notsky, scr, &fix, &dyn);
            }
            const unsigned m = sure ? bit : 0u;           // selects, not branches: this loop is the kernel's whole cost
            fixb |= fix ? m : 0u;
            dynb |= dyn ? m : 0u;
            todo |= bit ^ m;
        }
    }
    // Pass 2 (rare when the screen is on): the exact path, out of line, one pixel at a time; the pixel's inputs are re-read
    // (L1 / L2 hits) instead of being indexed out of registers.
    for (unsigned m = todo; m; m &= m - 1u) {
        const int k = __ffs(m) - 1, r = k >> 2, j = k & 3;
        const int x = xb + j, y = yb + r;
        const size_t o = b * npx + (size_t)y * W + x;
        const int notsky = !sky || sky[o] == 0;
        const auto rv = flow_raw(fl, W, y, x);
        const double d2x = (double)x - foex, d2y = (double)y - foey;
        PhiVerdict pv;
        if (f32_pair)       // diff2 is a float32 array in the reference: the double coordinate difference is rounded into it
            pv = phi_pixel_f32((float)rv.x, (float)rv.y, (float)d2x, (float)d2y, notsky, (float)thr.fixed_deg, (float)thr.fixed_min_mag,
                               (float)thr.dyn_min_mag, (float)thr.dyn_a, (float)thr.dyn_b, (float)thr.dyn_c);
        else {
            double u, v;
            derot_apply(rv, dp, W, H, y, x, &u, &v);
            pv = phi_pixel_exact(u, v, d2x, d2y, notsky, thr.fixed_deg, thr.fixed_min_mag, thr.dyn_min_mag, thr.dyn_a, thr.dyn_b, thr.dyn_c);
        }
        if (phi_out) phi_out[o] = pv.ph;
        pmax = pv.ph > pmax ? pv.ph : pmax;
        if (pv.bits & 1u) fixb |= 1u << k;
        if (pv.bits & 2u) dynb |= 1u << k;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = yb + r;
        if (y >= H || !colok) continue;
        const size_t o = b * npx + (size_t)y * W + xb;
        const unsigned f4 = (fixb >> (4 * r)) & 15u, d4 = (dynb >> (4 * r)) & 15u;
        if (VEC == 4) {
            // bit j -> byte j (0 / 1): spread the nibble over a dword
            if (mfix) *(uint32_t*)(mfix + o) = (f4 & 1u) | ((f4 & 2u) << 7) | ((f4 & 4u) << 14) | ((f4 & 8u) << 21);
            if (mdyn) *(uint32_t*)(mdyn + o) = (d4 & 1u) | ((d4 & 2u) << 7) | ((d4 & 4u) << 14) | ((d4 & 8u) << 21);
        } else {
            if (mfix) mfix[o] = (uint8_t)(f4 & 1u);
            if (mdyn) mdyn[o] = (uint8_t)(d4 & 1u);
        }
        if (f4) {
            bx0 = min(bx0, xb + __ffs(f4) - 1); bx1 = max(bx1, xb + 31 - __clz(f4));
            by0 = min(by0, y); by1 = max(by1, y);
        }
    }
    }   // yblk
    wave_box_commit(bx0, by0, bx1, by1, box_acc + 4 * b);
    if (max_phi_bits) {
        unsigned long long bits = (unsigned long long)__double_as_longlong(pmax);  // phi >= 0: bit order == value order
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(bits, o);
            bits = other > bits ? other : bits;
        }
        if (lane == 0 && bits > __hip_atomic_load(&max_phi_bits[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&max_phi_bits[b], bits);
    }
    // The pair's record (box + FoE; im_helpers.py:55-84 gives -1 for an empty mask) is written by the workgroup that draws the
    // pair's last ticket: every workgroup's box atomics have returned (wave_box_commit waits for them) before its ticket is drawn,
    // and the accumulators are read with agent-scope loads.  No separate finalize launch.
    if (done) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned ticket = atomicAdd(&done[2 * b + 1], 1u);
            if (ticket == gridDim.x * gridDim.y - 1) {
                int x0 = __hip_atomic_load(&box_acc[4 * b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int y0 = __hip_atomic_load(&box_acc[4 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int x1 = __hip_atomic_load(&box_acc[4 * b + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int y1 = __hip_atomic_load(&box_acc[4 * b + 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (x1 < 0) { x0 = y0 = x1 = y1 = -1; }
                if (results) {
                    results[b].box[0] = x0; results[b].box[1] = y0; results[b].box[2] = x1; results[b].box[3] = y1;
                    results[b].foe[0] = foex; results[b].foe[1] = foey;
                }
                if (box_out) { box_out[4 * b] = x0; box_out[4 * b + 1] = y0; box_out[4 * b + 2] = x1; box_out[4 * b + 3] = y1; }
                __hip_atomic_store(&done[2 * b + 1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// The screen is usable when neither phi nor max(phi) is requested and the thresholds are in the regime where
// "lo" (phi < dyn_a - (dyn_b + dyn_c/mag)) can never fire, the fixed threshold lies in (0, 80) degrees and the dynamic one is >= 0.
static PhiScreen phi_screen(const mav_thr_params& t, const double* phi, const unsigned long long* max_phi_bits, bool screen_on)
{
    PhiScreen s{};
    const bool ok = !phi && !max_phi_bits && t.fixed_deg > 0.0 && t.fixed_deg < 80.0 && t.dyn_a - t.dyn_b <= 0.0 &&
                    t.dyn_c >= 0.0 && t.dyn_a + t.dyn_b >= 0.0 && t.fixed_min_mag > 1e-3 && t.dyn_min_mag > 1e-3 &&
                    t.fixed_min_mag < 1e6 && t.dyn_min_mag < 1e6 && t.dyn_c < 1e6 && t.dyn_a + t.dyn_b < 1e3;
    s.enabled = ok && screen_on;
    s.tan_fixed = ok ? (float)tan(t.fixed_deg * 3.141592653589793238462643383279502884 / 180.0) : 0.f;
    s.margin_fixed = MAV_SCREEN_TAN_MARGIN * (1.f + s.tan_fixed);
    s.fmm2 = (float)(t.fixed_min_mag * t.fixed_min_mag);
    s.dmm2 = (float)(t.dyn_min_mag * t.dyn_min_mag);
    s.dyn_ab = (float)(t.dyn_a + t.dyn_b);
    s.dyn_c = (float)t.dyn_c;
    return s;
}

template <typename FlowT>
static void launch_phi_mask_t(hipStream_t st, const FlowT* flow, const DerotParams* derot, const double* foe, const uint8_t* sky,
                              int B, int W, int H, mav_thr_params thr, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                              int32_t* box_acc, unsigned long long* max_phi_bits, const PhiLaunch& pl)
{
    const PhiScreen scr = phi_screen(thr, phi, max_phi_bits, pl.screen);
    const bool vec = W % 4 == 0 && (((uintptr_t)sky | (uintptr_t)mask_fixed | (uintptr_t)mask_dyn) & 3) == 0;
    // Blocks of 16 rows per workgroup: enough that the whole launch stays near 4096 workgroups.  With one block each (34 816
    // workgroups at 1080p x 64 pairs) the kernel is bound by the rate at which waves can be launched, not by its bytes:
    // measured 0.55 ms, against 0.47 / 0.36 / 0.32 / 0.31 ms with 2 / 4 / 8 / 17 blocks per workgroup (option "phi_yloop" overrides).
    const int nby = (H + 15) / 16, gx = vec ? (W / 4 + 63) / 64 : (W + 63) / 64;
    int yloop = pl.yloop;
    if (yloop < 1) {
        const int want = 4096 / (gx * B > 0 ? gx * B : 1);
        yloop = want > 0 ? (nby + want - 1) / want : nby;
    }
    const dim3 grid(gx, (nby + yloop - 1) / yloop, B);
    auto k = vec ? (derot ? k_phi_mask<FlowT, 4, true> : k_phi_mask<FlowT, 4, false>)
                 : (derot ? k_phi_mask<FlowT, 1, true> : k_phi_mask<FlowT, 1, false>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, flow, derot, foe, sky, W, H, thr, scr, phi, mask_fixed, mask_dyn, box_acc, max_phi_bits,
                       (pl.results || pl.box_out) ? pl.done : (unsigned*)nullptr, pl.results, pl.box_out);
}
void launch_phi_mask_f32(hipStream_t st, const float* flow, const DerotParams* derot, const double* foe, const uint8_t* sky,
                         int B, int W, int H, mav_thr_params thr, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn,
                         int32_t* box_acc, unsigned long long* max_phi_bits, const PhiLaunch& pl)
{
    launch_phi_mask_t<float>(st, flow, derot, foe, sky, B, W, H, thr, phi, mask_fixed, mask_dyn, box_acc, max_phi_bits, pl);
}
void launch_phi_mask_f64(hipStream_t st, const double* flow, const double* foe, const uint8_t* sky, int B, int W, int H,
                         mav_thr_params thr, double* phi, uint8_t* mask_fixed, uint8_t* mask_dyn, int32_t* box_acc,
                         unsigned long long* max_phi_bits, const PhiLaunch& pl)
{
    launch_phi_mask_t<double>(st, flow, nullptr, foe, sky, B, W, H, thr, phi, mask_fixed, mask_dyn, box_acc, max_phi_bits, pl);
}

__global__ void k_finalize(const int32_t* __restrict__ box_acc, const double* __restrict__ foe, int B, mav_result* __restrict__ res,
                           int32_t* __restrict__ box_only)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int x0 = box_acc[4 * b], y0 = box_acc[4 * b + 1], x1 = box_acc[4 * b + 2], y1 = box_acc[4 * b + 3];
    if (x1 < 0) { x0 = y0 = x1 = y1 = -1; }
    if (res) {
        res[b].box[0] = x0; res[b].box[1] = y0; res[b].box[2] = x1; res[b].box[3] = y1;
        res[b].foe[0] = foe[2 * b]; res[b].foe[1] = foe[2 * b + 1];
    }
    if (box_only) { box_only[4 * b] = x0; box_only[4 * b + 1] = y0; box_only[4 * b + 2] = x1; box_only[4 * b + 3] = y1; }
}
void launch_box_finalize(hipStream_t st, const int32_t* box_acc, int B, int32_t* box)
{
    hipLaunchKernelGGL(k_finalize, dim3((B + 63) / 64), dim3(64), 0, st, box_acc, (const double*)nullptr, B,
                       (mav_result*)nullptr, box);
}

// ------------------------------------------------------------------------------------------------------------
// get_simple_bounding_box on arbitrary u8 images: pass 1 max, pass 2 extents of (double)v > 0.1*max.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_u8_max(const uint8_t* __restrict__ img, int W, int H, int* __restrict__ maxv)
{
    const int b = blockIdx.z;
    const size_t npx = (size_t)W * H;
    const uint8_t* p = img + b * npx;
    int m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) m = max(m, (int)p[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&maxv[b], m);
}
__global__ __launch_bounds__(256) void k_u8_extents(const uint8_t* __restrict__ img, int W, int H, const int* __restrict__ maxv,
                                                    int32_t* __restrict__ box_acc)
{
    const int b = blockIdx.z;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const double thr = 0.1 * (double)maxv[b];
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    if (y < H)
        for (int x = blockIdx.x * 256 + (threadIdx.x & 63); x < min(W, (int)(blockIdx.x + 1) * 256); x += 64)
            if ((double)img[(size_t)b * W * H + (size_t)y * W + x] > thr) {
                bx0 = min(bx0, x); bx1 = max(bx1, x); by0 = min(by0, y); by1 = max(by1, y);
            }
    wave_box_commit(bx0, by0, bx1, by1, box_acc + 4 * b);
}
void launch_bbox_u8(hipStream_t st, const uint8_t* img, int B, int W, int H, int* maxv, int32_t* box_acc)
{
    hipMemsetAsync(maxv, 0, sizeof(int) * B, st);
    hipLaunchKernelGGL(k_u8_max, dim3(64, 1, B), dim3(256), 0, st, img, W, H, maxv);
    hipLaunchKernelGGL(k_u8_extents, dim3((W + 255) / 256, (H + 3) / 4, B), dim3(256), 0, st, img, W, H, maxv, box_acc);
}

// ------------------------------------------------------------------------------------------------------------
// analyze_pyramid level 0: 64x64 windows, stride 16, score = 3 * sum(u8) (the to_rgb replica has 3 equal channels);
// first window in row-major scan order with the strictly largest score.  One workgroup per window row.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_max(const uint8_t* __restrict__ img, int W, int H, int nwx,
                                                    unsigned long long* __restrict__ key)
{
    extern __shared__ int colsum[];
    const int b = blockIdx.y, wy = blockIdx.x, tid = threadIdx.x;
    const uint8_t* p = img + (size_t)b * W * H + (size_t)wy * 16 * W;
    for (int x = tid; x < W; x += 256) {
        int s = 0;
        for (int r = 0; r < 64; r++) s += p[(size_t)r * W + x];
        colsum[x] = s;
    }
    __syncthreads();
    unsigned long long k = 0ull;
    for (int wx = tid; wx < nwx; wx += 256) {
        int s = 0;
        for (int c = 0; c < 64; c++) s += colsum[wx * 16 + c];
        const unsigned score = 3u * (unsigned)s;
        const unsigned idx = (unsigned)(wy * nwx + wx);
        if (score) {
            const unsigned long long kk = ((unsigned long long)score << 32) | (0xFFFFFFFFu - idx);
            k = kk > k ? kk : k;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other > k ? other : k;
    }
    if ((tid & 63) == 0 && k) atomicMax(&key[b], k);
}
__global__ void k_window_finalize(const unsigned long long* __restrict__ key, int nwx, int B, int64_t* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long k = key[b];
    int64_t score = 0, x = 0, y = 0;
    if (k) {
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
        score = (int64_t)(k >> 32);
        x = (int64_t)(idx % nwx) * 16;
        y = (int64_t)(idx / nwx) * 16;
    }
    out[3 * b] = score; out[3 * b + 1] = x; out[3 * b + 2] = y;
}
void launch_window_max(hipStream_t st, const uint8_t* img, int B, int W, int H, unsigned long long* key, int64_t* out)
{
    hipMemsetAsync(key, 0, sizeof(unsigned long long) * B, st);
    const int nwx = W >= 64 ? (W - 64) / 16 + 1 : 0, nwy = H >= 64 ? (H - 64) / 16 + 1 : 0;
    if (nwx > 0 && nwy > 0)
        hipLaunchKernelGGL(k_window_max, dim3(nwy, B), dim3(256), sizeof(int) * (size_t)W, st, img, W, H, nwx, key);
    hipLaunchKernelGGL(k_window_finalize, dim3((B + 63) / 64), dim3(64), 0, st, key, nwx > 0 ? nwx : 1, B, out);
}

// calculate_tpr_fpr counts for gt (u8) against mask_value * mask: the reference's products in wide integers (no u8 wrap).
// One pass over the ground truth serves one mask or two (the fixed and the dynamic mask of a detection call); gt_stride = 0: one
// ground-truth image for every pair of the batch (a constant segmentation).  16 bytes per thread and load where the images are
// 16-byte addressable, byte by byte otherwise; the counts are integers, so the order of the additions is immaterial.
__device__ __forceinline__ void tpr_fpr_byte(unsigned gv, unsigned m0, unsigned m1, unsigned mask_value, unsigned& pos, unsigned& neg, unsigned& tp0,
                                             unsigned& fp0, unsigned& tp1, unsigned& fp1)
{
    const unsigned v0 = m0 ? mask_value : 0u, v1 = m1 ? mask_value : 0u;
    pos += gv > 127u;
    neg += (255u - gv) > 127u;
    tp0 += (gv * v0) > 127u;
    fp0 += ((255u - gv) * v0) > 127u;
    tp1 += (gv * v1) > 127u;
    fp1 += ((255u - gv) * v1) > 127u;
}
template <bool TWO, bool VEC>
__global__ __launch_bounds__(256) void k_tpr_fpr(const uint8_t* __restrict__ gt, size_t gt_stride, const uint8_t* __restrict__ mask0,
                                                 const uint8_t* __restrict__ mask1, unsigned mask_value, size_t npx,
                                                 unsigned long long* __restrict__ counts0, unsigned long long* __restrict__ counts1)
{
    const int b = blockIdx.y;
    const uint8_t* g = gt + b * gt_stride;
    const uint8_t* m0 = mask0 + b * npx;
    const uint8_t* m1 = TWO ? mask1 + b * npx : m0;
    unsigned pos = 0, neg = 0, tp0 = 0, fp0 = 0, tp1 = 0, fp1 = 0;
    if (VEC) {
        const size_t nv = npx / 16;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
            const uint4 gv = ((const uint4*)g)[i], a = ((const uint4*)m0)[i], c = TWO ? ((const uint4*)m1)[i] : a;
            const unsigned gw[4] = {gv.x, gv.y, gv.z, gv.w}, aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int w = 0; w < 4; w++)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    tpr_fpr_byte((gw[w] >> (8 * k)) & 255u, (aw[w] >> (8 * k)) & 255u, (cw[w] >> (8 * k)) & 255u, mask_value, pos, neg, tp0, fp0, tp1, fp1);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256)
            tpr_fpr_byte(g[i], m0[i], TWO ? m1[i] : 0u, mask_value, pos, neg, tp0, fp0, tp1, fp1);
    }
    for (int o = 32; o > 0; o >>= 1) {
        pos += __shfl_xor(pos, o); neg += __shfl_xor(neg, o); tp0 += __shfl_xor(tp0, o); fp0 += __shfl_xor(fp0, o);
        if (TWO) { tp1 += __shfl_xor(tp1, o); fp1 += __shfl_xor(fp1, o); }
    }
    // one set of atomics per WORKGROUP (round 6): with one per wave a single 1280x720 pair issued 4 096 64-bit atomics onto eight
    // addresses and the kernel took 35 us for 2.8 MB -- all of it the atomics' serialisation
    __shared__ unsigned part[4][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = pos; part[wave][1] = neg; part[wave][2] = tp0; part[wave][3] = fp0; part[wave][4] = tp1; part[wave][5] = fp1;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned long long v = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        const int k = threadIdx.x;                 // 0 pos, 1 neg, 2 tp0, 3 fp0, 4 tp1, 5 fp1
        if (k < 4) atomicAdd(&counts0[4 * b + k], v);
        if (TWO) {
            if (k < 2) atomicAdd(&counts1[4 * b + k], v);
            if (k >= 4) atomicAdd(&counts1[4 * b + k - 2], v);
        }
    }
}
void launch_tpr_fpr2(hipStream_t st, const uint8_t* gt, size_t gt_stride, const uint8_t* mask0, const uint8_t* mask1, unsigned mask_value, int B,
                     int W, int H, unsigned long long* counts0, unsigned long long* counts1)
{
    const size_t npx = (size_t)W * H;
    if (mask1 && counts1 == counts0 + 4 * (size_t)B) {           // the two count blocks follow each other (the fused step, full batch): one fill
        hipMemsetAsync(counts0, 0, sizeof(unsigned long long) * 8 * B, st);
    } else {
        hipMemsetAsync(counts0, 0, sizeof(unsigned long long) * 4 * B, st);
        if (mask1) hipMemsetAsync(counts1, 0, sizeof(unsigned long long) * 4 * B, st);
    }
    const bool vec = npx % 16 == 0 && gt_stride % 16 == 0 && (((uintptr_t)gt | (uintptr_t)mask0 | (uintptr_t)mask1) & 15) == 0;
    const dim3 grid(128, B), blk(256);
    if (mask1) {
        if (vec) hipLaunchKernelGGL((k_tpr_fpr<true, true>), grid, blk, 0, st, gt, gt_stride, mask0, mask1, mask_value, npx, counts0, counts1);
        else hipLaunchKernelGGL((k_tpr_fpr<true, false>), grid, blk, 0, st, gt, gt_stride, mask0, mask1, mask_value, npx, counts0, counts1);
    } else {
        if (vec) hipLaunchKernelGGL((k_tpr_fpr<false, true>), grid, blk, 0, st, gt, gt_stride, mask0, mask1, mask_value, npx, counts0, counts1);
        else hipLaunchKernelGGL((k_tpr_fpr<false, false>), grid, blk, 0, st, gt, gt_stride, mask0, mask1, mask_value, npx, counts0, counts1);
    }
}
void launch_tpr_fpr(hipStream_t st, const uint8_t* gt, const uint8_t* mask, unsigned mask_value, int B, int W, int H,
                    unsigned long long* counts)
{
    launch_tpr_fpr2(st, gt, (size_t)W * H, mask, nullptr, mask_value, B, W, H, counts, nullptr);
}

// ------------------------------------------------------------------------------------------------------------
// Threshold sweep (include/mavflow.h: mav_roc_sweep): the tp / fp counts of the fixed mask for every (angle, magnitude) pair of two
// sorted lists in one pass over flow, sky and ground truth.  The fixed mask  phi * (mag > m) * ~sky > t  is, for t >= 0 and a phi
// that is never NaN,  ~sky && mag > m && phi > t : monotone in both thresholds.  A pixel with ia = #{angles < phi} and
// im = #{mags < mag} (strict, as the mask's comparisons) is set in exactly the cells (i < ia, j < im); the kernel counts it once, in
// the exact bin (ia - 1, im - 1) of a per-workgroup LDS histogram (tp and fp separately: gt >= 1 / gt <= 254 at mask value 255), and
// k_roc_suffix turns the bins into cells.  phi and the magnitude come from derot_apply / phi_exact (float64 pairs) and phi_pixel_f32
// (frame-0 pairs, against the thresholds rounded to float32): the bits of k_phi_mask's exact path.  Sky pixels and pixels below the
// smallest magnitude never reach the arccos; a float64 pair below it skips the square root too (a frame-0 pair always takes sqrtf).  Integer counts: the result does not depend on the order of the additions.
// Workgroup = 1024 consecutive pixels per step (four per thread, 256 apart: every load is lane-contiguous), grid-strided.
// A wave whose set pixels all fall into ONE bin (a strong uniform field: every pixel in the top bin) adds its ballot counts once
// instead of serialising 64 same-address LDS atomics.  FlowT = double: an already derotated float64 field (mav_phi_mask's input).
template <typename FlowT>
__global__ __launch_bounds__(256) void k_roc_sweep(const FlowT* __restrict__ flow, const DerotParams* __restrict__ derot,
                                                   const double* __restrict__ foe, const uint8_t* __restrict__ sky,
                                                   const uint8_t* __restrict__ gt, size_t gt_stride, int W, int H, RocThr thr,
                                                   unsigned long long* __restrict__ table)
{
    __shared__ unsigned hist[MAV_ROC_MAX_ANGLES * MAV_ROC_MAX_MAGS * 2];
    __shared__ unsigned part[4][2];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned npx = (unsigned)W * (unsigned)H;
    const int ka = thr.ka, km = thr.km, cells2 = ka * km * 2;
    for (int i = tid; i < cells2; i += 256) hist[i] = 0u;
    __syncthreads();
    const FlowT* fl = flow + (size_t)b * npx * 2;
    const uint8_t* sk = sky ? sky + (size_t)b * npx : nullptr;
    const uint8_t* g = gt + (size_t)b * gt_stride;
    const DerotParams* dp = derot ? derot + b : nullptr;
    const bool f32_pair = std::is_same<FlowT, float>::value && dp && dp->mode == MAV_PAIR_FRAME0;
    const double foex = foe[2 * b], foey = foe[2 * b + 1];
    unsigned pos = 0u, neg = 0u;
    for (unsigned base = blockIdx.x * 1024u; base < npx; base += gridDim.x * 1024u) {
        decltype(flow_raw(fl, W, 0, 0)) raw[4];
        unsigned skv[4], gv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned p = base + k * 256u + tid;
            const unsigned q = p < npx ? p : npx - 1u;        // past the end: re-read the last pixel, never counted
            raw[k] = flow_raw(fl, (int)npx, 0, (int)q);          // pixel q of the image, as one row
            skv[k] = sk ? sk[q] : 0u;
            gv[k] = g[q];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned p = base + k * 256u + tid;
            const bool valid = p < npx;
            pos += (valid && gv[k] > 127u) ? 1u : 0u;
            neg += (valid && (255u - gv[k]) > 127u) ? 1u : 0u;
            int key = -1;
            if (valid && skv[k] == 0u) {
                const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
                const double d2x = (double)x - foex, d2y = (double)y - foey;
                int ia = 0, im = 0;
                if (f32_pair) {
                    const float u = (float)raw[k].x, v = (float)raw[k].y;
                    const float fm = sqrtf(u * u + v * v);                 // phi_pixel_f32's magnitude
                    for (int j = 0; j < km; j++) im += thr.mag32[j] < fm ? 1 : 0;
                    if (im) {
                        const PhiVerdict pv = phi_pixel_f32(u, v, (float)d2x, (float)d2y, 1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
                        const float ph = (float)pv.ph;                     // the float32 value, widened and back
                        for (int i = 0; i < ka; i++) ia += thr.ang32[i] < ph ? 1 : 0;
                    }
                } else {
                    double u, v;
                    derot_apply(raw[k], dp, W, H, y, x, &u, &v);
                    const double m2 = u * u + v * v;
                    if (!(m2 < thr.mag0_sq_lo)) {                          // below: sqrt(m2) <= mag[0], no gate passes (NaN goes on)
                        double fm = sqrt(m2);
                        for (int j = 0; j < km; j++) im += thr.mag[j] < fm ? 1 : 0;
                        if (im) {
                            const double ph = phi_exact(u, v, d2x, d2y, &fm);
                            for (int i = 0; i < ka; i++) ia += thr.ang[i] < ph ? 1 : 0;
                        }
                    }
                }
                if (ia > 0 && im > 0) key = (ia - 1) * km + (im - 1);
            }
            // every lane of the wave arrives here (the loops above have wave-uniform bounds)
            const bool tp = key >= 0 && gv[k] >= 1u, fp = key >= 0 && gv[k] <= 254u;
            const unsigned long long any = __ballot(key >= 0);
            if (any) {
                const int first = __shfl(key, __ffsll((long long)any) - 1);
                if (__ballot(key >= 0 && key != first) == 0ull) {
                    const unsigned ntp = (unsigned)__popcll(__ballot(tp)), nfp = (unsigned)__popcll(__ballot(fp));
                    if (lane == 0) {
                        if (ntp) atomicAdd(&hist[2 * first], ntp);
                        if (nfp) atomicAdd(&hist[2 * first + 1], nfp);
                    }
                } else {
                    if (tp) atomicAdd(&hist[2 * key], 1u);
                    if (fp) atomicAdd(&hist[2 * key + 1], 1u);
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o); neg += __shfl_xor(neg, o); }
    if (lane == 0) { part[wv][0] = pos; part[wv][1] = neg; }
    __syncthreads();                                                       // ... and every wave's histogram updates
    unsigned long long* tab = table + (size_t)b * MAV_ROC_TABLE_WORDS(ka, km);
    if (tid < 2) {
        const unsigned long long v = (unsigned long long)part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (v) atomicAdd(&tab[tid], v);
    }
    for (int i = tid; i < cells2; i += 256) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&tab[2 + i], (unsigned long long)v);
    }
}
// Exact bins -> cells, in place, one workgroup per pair: cell[i][j] = sum of the bins (a >= i, b >= j), a suffix sum along the
// magnitudes and then along the angles.
__global__ __launch_bounds__(256) void k_roc_suffix(unsigned long long* __restrict__ table, int ka, int km)
{
    __shared__ unsigned long long s[MAV_ROC_MAX_ANGLES * MAV_ROC_MAX_MAGS * 2];
    unsigned long long* t = table + (size_t)blockIdx.x * MAV_ROC_TABLE_WORDS(ka, km) + 2;
    const int tid = threadIdx.x, cells2 = ka * km * 2;
    for (int i = tid; i < cells2; i += 256) s[i] = t[i];
    __syncthreads();
    for (int r = tid; r < ka * 2; r += 256) {
        const int i = r >> 1, k = r & 1;
        unsigned long long acc = 0ull;
        for (int j = km - 1; j >= 0; j--) { acc += s[(i * km + j) * 2 + k]; s[(i * km + j) * 2 + k] = acc; }
    }
    __syncthreads();
    for (int r = tid; r < km * 2; r += 256) {
        const int j = r >> 1, k = r & 1;
        unsigned long long acc = 0ull;
        for (int i = ka - 1; i >= 0; i--) { acc += s[(i * km + j) * 2 + k]; s[(i * km + j) * 2 + k] = acc; }
    }
    __syncthreads();
    for (int i = tid; i < cells2; i += 256) t[i] = s[i];
}
hipError_t launch_roc_sweep(hipStream_t st, const void* flow, bool f64, const DerotParams* derot, const double* foe, const uint8_t* sky,
                      const uint8_t* gt, size_t gt_stride, int B, int W, int H, const RocThr& thr, unsigned long long* table)
{
    const size_t npx = (size_t)W * H;
    const hipError_t e = hipMemsetAsync(table, 0, sizeof(unsigned long long) * MAV_ROC_TABLE_WORDS(thr.ka, thr.km) * B, st);
    if (e != hipSuccess) return e;                           // bins would be added to whatever the table held
    // about 1024 workgroups in all: each flushes its non-zero bins with 64-bit atomics, so fewer, longer-lived workgroups per pair
    const int nblk = (int)((npx + 1023) / 1024), cap = 1024 / B > 0 ? 1024 / B : 1;
    const dim3 grid(nblk < cap ? nblk : cap, 1, B);
    if (f64)
        hipLaunchKernelGGL(k_roc_sweep<double>, grid, dim3(256), 0, st, (const double*)flow, (const DerotParams*)nullptr, foe, sky, gt, gt_stride,
                           W, H, thr, table);
    else
        hipLaunchKernelGGL(k_roc_sweep<float>, grid, dim3(256), 0, st, (const float*)flow, derot, foe, sky, gt, gt_stride, W, H, thr, table);
    hipLaunchKernelGGL(k_roc_suffix, dim3(B), dim3(256), 0, st, table, thr.ka, thr.km);
    return hipSuccess;
}

// cv2.cvtColor(COLOR_BGR2GRAY) on u8 (farneback.py:21,74): fixed point, (B*1868 + G*9617 + R*4899 + 8192) >> 14  (SURVEY A.7).
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t* __restrict__ bgr, size_t n, uint8_t* __restrict__ gray)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint8_t* p = bgr + 3 * i;
        gray[i] = bgr2gray_px(p[0], p[1], p[2]);
    }
}
void launch_bgr2gray(hipStream_t st, const uint8_t* bgr, size_t n, uint8_t* gray)
{
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_bgr2gray, dim3((unsigned)(blocks < 4096 ? (blocks ? blocks : 1) : 4096)), dim3(256), 0, st, bgr, n, gray);
}

// FocusOfExpansion.ransac on caller-supplied estimates (already in s.cand[0..M), s.count[0] = M): vote + pick.
__global__ void k_set_count(FoeScratch sc, int M)
{
    sc.count[0] = M;
    sc.best_key[0] = 0ull;
    sc.done[0] = 0u;
}
void launch_ransac_only(hipStream_t st, FoeScratch s, int M, int N, double dist2_thr, double* foe)
{
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, st, s, M);
    hipLaunchKernelGGL(k_ransac, dim3(((M > 0 ? M : 1) + 15) / 16, 1), dim3(256), 0, st, s, N, dist2_thr, foe);
}

// DerotParams from device-resident omega (B,3) and dt (B, nullable = 1): sx = w*dt/2, sy = h*dt/2 (detector.py:101-102).
__global__ void k_make_derot(const double* __restrict__ omega, const double* __restrict__ dt, const uint8_t* __restrict__ frame0,
                             int B, int W, int H, DerotParams* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double d = dt ? dt[b] : 1.0;
    DerotParams p;
    p.o0 = omega ? omega[3 * b] : 0.0; p.o1 = omega ? omega[3 * b + 1] : 0.0; p.o2 = omega ? omega[3 * b + 2] : 0.0;
    p.sx = (double)W * d / 2;
    p.sy = (double)H * d / 2;
    p.mode = (frame0 && frame0[b]) ? MAV_PAIR_FRAME0 : (omega ? MAV_PAIR_DEROTATE : MAV_PAIR_PROMOTE);
    out[b] = p;
}
void launch_make_derot(hipStream_t st, const double* omega, const double* dt, const uint8_t* frame0, int B, int W, int H,
                       DerotParams* out)
{
    hipLaunchKernelGGL(k_make_derot, dim3((B + 63) / 64), dim3(64), 0, st, omega, dt, frame0, B, W, H, out);
}

// ------------------------------------------------------------------------------------------------------------
// Result images of Processor.run_detection (src/processor.py:364-374 of the reference), (H, W, 3) u8 BGR each:
//   result   im_helpers.to_rgb(255 * estimate_fixed): 255 where the fixed-threshold mask is set, 0 elsewhere (an empty mask goes
//            through 0 / 0 = NaN -> astype(uint8), which is 0 as well)
//   flow     flow_vis.flow_to_color(derotated flow, convert_to_bgr=True)
//   phi      cv2.applyColorMap(to_rgb(phi, max_value=180.0), COLORMAP_JET)
// The render kernel recomputes derotation, mask and phi per pixel with the very device functions k_phi_mask's exact path uses
// (derot_apply, phi_pixel_exact, phi_pixel_f32): no single-precision screen, so mask and phi are the exact ones.  flow_to_color
// normalises by the pair's max |flow|, which k_render_radmax reduces first (max is order independent: the reduction is exact).

// cv2.COLORMAP_JET, BGR.  Entries 0..199 are pinned by the reference's media/colorbar.png (tests/golden/colorbar.png); entries
// 200..255 are NOT pinned by any image the reference wrote: they continue the ramps of OpenCV's Jet (red holds 255 to 223 and falls
// by 4 per entry to 128, green falls by 4 per entry to 0 at 223, blue stays 0) and agree with the mirror image of entries 0..55.
struct JetLut { uint8_t bgr[256][3]; };
__constant__ JetLut c_jet = {{
    {128, 0, 0}, {132, 0, 0}, {136, 0, 0}, {140, 0, 0}, {144, 0, 0}, {148, 0, 0}, {152, 0, 0}, {156, 0, 0},
    {160, 0, 0}, {164, 0, 0}, {168, 0, 0}, {172, 0, 0}, {176, 0, 0}, {180, 0, 0}, {184, 0, 0}, {188, 0, 0},
    {192, 0, 0}, {196, 0, 0}, {200, 0, 0}, {204, 0, 0}, {208, 0, 0}, {212, 0, 0}, {216, 0, 0}, {220, 0, 0},
    {224, 0, 0}, {228, 0, 0}, {232, 0, 0}, {236, 0, 0}, {240, 0, 0}, {244, 0, 0}, {248, 0, 0}, {252, 0, 0},
    {255, 0, 0}, {255, 4, 0}, {255, 8, 0}, {255, 12, 0}, {255, 16, 0}, {255, 20, 0}, {255, 24, 0}, {255, 28, 0},
    {255, 32, 0}, {255, 36, 0}, {255, 40, 0}, {255, 44, 0}, {255, 48, 0}, {255, 52, 0}, {255, 56, 0}, {255, 60, 0},
    {255, 64, 0}, {255, 68, 0}, {255, 72, 0}, {255, 76, 0}, {255, 80, 0}, {255, 84, 0}, {255, 88, 0}, {255, 92, 0},
    {255, 96, 0}, {255, 100, 0}, {255, 104, 0}, {255, 108, 0}, {255, 112, 0}, {255, 116, 0}, {255, 120, 0}, {255, 124, 0},
    {255, 128, 0}, {255, 132, 0}, {255, 136, 0}, {255, 140, 0}, {255, 144, 0}, {255, 148, 0}, {255, 152, 0}, {255, 156, 0},
    {255, 160, 0}, {255, 164, 0}, {255, 168, 0}, {255, 172, 0}, {255, 176, 0}, {255, 180, 0}, {255, 184, 0}, {255, 188, 0},
    {255, 192, 0}, {255, 196, 0}, {255, 200, 0}, {255, 204, 0}, {255, 208, 0}, {255, 212, 0}, {255, 216, 0}, {255, 220, 0},
    {255, 224, 0}, {255, 228, 0}, {255, 232, 0}, {255, 236, 0}, {255, 240, 0}, {255, 244, 0}, {255, 248, 0}, {255, 252, 0},
    {254, 255, 2}, {250, 255, 6}, {246, 255, 10}, {242, 255, 14}, {238, 255, 18}, {234, 255, 22}, {230, 255, 26}, {226, 255, 30},
    {222, 255, 34}, {218, 255, 38}, {214, 255, 42}, {210, 255, 46}, {206, 255, 50}, {202, 255, 54}, {198, 255, 58}, {194, 255, 62},
    {190, 255, 66}, {186, 255, 70}, {182, 255, 74}, {178, 255, 78}, {174, 255, 82}, {170, 255, 86}, {166, 255, 90}, {162, 255, 94},
    {158, 255, 98}, {154, 255, 102}, {150, 255, 106}, {146, 255, 110}, {142, 255, 114}, {138, 255, 118}, {134, 255, 122}, {130, 255, 126},
    {126, 255, 130}, {122, 255, 134}, {118, 255, 138}, {114, 255, 142}, {110, 255, 146}, {106, 255, 150}, {102, 255, 154}, {98, 255, 158},
    {94, 255, 162}, {90, 255, 166}, {86, 255, 170}, {82, 255, 174}, {78, 255, 178}, {74, 255, 182}, {70, 255, 186}, {66, 255, 190},
    {62, 255, 194}, {58, 255, 198}, {54, 255, 202}, {50, 255, 206}, {46, 255, 210}, {42, 255, 214}, {38, 255, 218}, {34, 255, 222},
    {30, 255, 226}, {26, 255, 230}, {22, 255, 234}, {18, 255, 238}, {14, 255, 242}, {10, 255, 246}, {6, 255, 250}, {1, 255, 254},
    {0, 252, 255}, {0, 248, 255}, {0, 244, 255}, {0, 240, 255}, {0, 236, 255}, {0, 232, 255}, {0, 228, 255}, {0, 224, 255},
    {0, 220, 255}, {0, 216, 255}, {0, 212, 255}, {0, 208, 255}, {0, 204, 255}, {0, 200, 255}, {0, 196, 255}, {0, 192, 255},
    {0, 188, 255}, {0, 184, 255}, {0, 180, 255}, {0, 176, 255}, {0, 172, 255}, {0, 168, 255}, {0, 164, 255}, {0, 160, 255},
    {0, 156, 255}, {0, 152, 255}, {0, 148, 255}, {0, 144, 255}, {0, 140, 255}, {0, 136, 255}, {0, 132, 255}, {0, 128, 255},
    {0, 124, 255}, {0, 120, 255}, {0, 116, 255}, {0, 112, 255}, {0, 108, 255}, {0, 104, 255}, {0, 100, 255}, {0, 96, 255},
    {0, 92, 255}, {0, 88, 255}, {0, 84, 255}, {0, 80, 255}, {0, 76, 255}, {0, 72, 255}, {0, 68, 255}, {0, 64, 255},
    {0, 60, 255}, {0, 56, 255}, {0, 52, 255}, {0, 48, 255}, {0, 44, 255}, {0, 40, 255}, {0, 36, 255}, {0, 32, 255},
    {0, 28, 255}, {0, 24, 255}, {0, 20, 255}, {0, 16, 255}, {0, 12, 255}, {0, 8, 255}, {0, 4, 255}, {0, 0, 255},
    {0, 0, 252}, {0, 0, 248}, {0, 0, 244}, {0, 0, 240}, {0, 0, 236}, {0, 0, 232}, {0, 0, 228}, {0, 0, 224},
    {0, 0, 220}, {0, 0, 216}, {0, 0, 212}, {0, 0, 208}, {0, 0, 204}, {0, 0, 200}, {0, 0, 196}, {0, 0, 192},
    {0, 0, 188}, {0, 0, 184}, {0, 0, 180}, {0, 0, 176}, {0, 0, 172}, {0, 0, 168}, {0, 0, 164}, {0, 0, 160},
    {0, 0, 156}, {0, 0, 152}, {0, 0, 148}, {0, 0, 144}, {0, 0, 140}, {0, 0, 136}, {0, 0, 132}, {0, 0, 128},
}};

// flow_vis.make_colorwheel: the 55-entry Middlebury wheel (RY 15, YG 6, GC 4, CB 11, BM 13, MR 6), RGB, entries floor(255 * j / n).
struct Wheel { uint8_t rgb[55][3]; };
static constexpr Wheel make_wheel()
{
    Wheel w{};
    const int n[6] = {15, 6, 4, 11, 13, 6};
    int k = 0;
    for (int s = 0; s < 6; s++)
        for (int j = 0; j < n[s]; j++, k++) {
            const int up = 255 * j / n[s], down = 255 - up;    // floor(255 * j / n): the quotient is exact or not an integer
            int r = 0, g = 0, b = 0;
            switch (s) {
            case 0: r = 255; g = up; break;      // RY
            case 1: r = down; g = 255; break;    // YG
            case 2: g = 255; b = up; break;      // GC
            case 3: g = down; b = 255; break;    // CB
            case 4: b = 255; r = up; break;      // BM
            default: b = down; r = 255; break;   // MR
            }
            w.rgb[k][0] = (uint8_t)r; w.rgb[k][1] = (uint8_t)g; w.rgb[k][2] = (uint8_t)b;
        }
    return w;
}
__constant__ Wheel c_wheel = make_wheel();

// floor(255 * col) -> u8 as numpy's astype(uint8) of a value in [0, 255]; NaN -> 0 (x86-64).  Clamped: never wraps.
static __device__ __forceinline__ unsigned u8_of(double x)
{
    return x >= 1.0 ? (x < 255.0 ? (unsigned)x : 255u) : 0u;
}

// One pixel of flow_uv_to_colors after the normalisation.  fk is the wheel coordinate (a + 1) / 2 * 54 and rad the normalised
// magnitude in the field's own type; from `f = fk - k0` on numpy works in double for both field types (float32 - int32 -> float64).
static __device__ __forceinline__ unsigned wheel_bgr(double fk, double rad)
{
    const int k0 = (fk >= 0.0 && fk < 55.0) ? (int)floor(fk) : 0;   // a is in [-1, 1]: fk in [0, 54]; NaN -> entry 0, in bounds
    const int k1 = k0 + 1 == 55 ? 0 : k0 + 1;
    const double f = fk - (double)k0;
    unsigned out = 0u;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double col0 = (double)c_wheel.rgb[k0][i] / 255.0, col1 = (double)c_wheel.rgb[k1][i] / 255.0;
        double col = (1.0 - f) * col0 + f * col1;
        col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
        out |= u8_of(floor(255.0 * col)) << (8 * (2 - i));           // channel 2 - i: BGR
    }
    return out;
}

// The pair's max |flow| as the reference forms it (flow_to_color: rad = sqrt(u^2 + v^2), rad_max = max(rad)): double for a derotated
// (or promoted) pair, float32 for a frame-0 pair, stored widened.  radmax[b] zeroed by the caller; |flow| >= 0, so bit order is value order.
template <typename FlowT>
__global__ __launch_bounds__(256) void k_render_radmax(const FlowT* __restrict__ flow, const DerotParams* __restrict__ derot, int W, int H,
                                                       unsigned long long* __restrict__ radmax)
{
    const int b = blockIdx.y;
    const size_t npx = (size_t)W * H;
    const FlowT* fl = flow + b * npx * 2;
    const DerotParams* dp = derot ? derot + b : nullptr;
    const bool f32 = std::is_same<FlowT, float>::value && dp && dp->mode == MAV_PAIR_FRAME0;
    double m = 0.0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npx; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        const auto rv = flow_raw(fl, W, y, x);
        double r;
        if (f32) {
            const float u = (float)rv.x, v = (float)rv.y;
            r = (double)sqrtf(u * u + v * v);
        } else {
            double u, v;
            derot_apply(rv, dp, W, H, y, x, &u, &v);
            r = sqrt(u * u + v * v);
        }
        m = r > m ? r : m;
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(m);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(bits, o);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(&radmax[b], bits);
}

// Four consecutive pixels of the batch per thread (the flattened (B, H, W) index): each image gets three dword stores.
template <typename FlowT>
__global__ __launch_bounds__(256) void k_render(const FlowT* __restrict__ flow, const DerotParams* __restrict__ derot,
                                                const double* __restrict__ foe, const uint8_t* __restrict__ sky, int W, int H, int B,
                                                mav_thr_params thr, const unsigned long long* __restrict__ radmax,
                                                uint8_t* __restrict__ o_res, uint8_t* __restrict__ o_flow, uint8_t* __restrict__ o_phi)
{
    const size_t npx = (size_t)W * H, total = npx * B;
    const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= total) return;
    const bool need_phi = o_res || o_phi;
    unsigned px_res[4], px_flow[4], px_phi[4];                 // 0x00BBGGRR-style packed BGR of each pixel (byte 0 = B)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        px_res[j] = px_flow[j] = px_phi[j] = 0u;
        const size_t p = p0 + j;
        if (p >= total) continue;
        const int b = (int)(p / npx);
        const size_t q = p - (size_t)b * npx;
        const int y = (int)(q / W), x = (int)(q - (size_t)y * W);
        const DerotParams* dp = derot ? derot + b : nullptr;
        const bool f32 = std::is_same<FlowT, float>::value && dp && dp->mode == MAV_PAIR_FRAME0;
        const auto rv = flow_raw(flow + b * npx * 2, W, y, x);
        double u = 0.0, v = 0.0;
        if (!f32) derot_apply(rv, dp, W, H, y, x, &u, &v);
        if (need_phi) {
            const int notsky = !sky || sky[p] == 0;
            const double d2x = (double)x - foe[2 * b], d2y = (double)y - foe[2 * b + 1];
            unsigned g;
            PhiVerdict pv;
            if (f32) {
                pv = phi_pixel_f32((float)rv.x, (float)rv.y, (float)d2x, (float)d2y, notsky, (float)thr.fixed_deg, (float)thr.fixed_min_mag,
                                   (float)thr.dyn_min_mag, (float)thr.dyn_a, (float)thr.dyn_b, (float)thr.dyn_c);
                // to_int: np.abs(phi) * 255 / 180.0 in float32 (numpy 2 keeps the Python scalars weak), np.around = half to even
                const float s = fabsf((float)pv.ph) * 255.0f / 180.0f;
                g = u8_of((double)rintf(s));
            } else {
                pv = phi_pixel_exact(u, v, d2x, d2y, notsky, thr.fixed_deg, thr.fixed_min_mag, thr.dyn_min_mag, thr.dyn_a, thr.dyn_b,
                                     thr.dyn_c);
                g = u8_of(rint(fabs(pv.ph) * 255.0 / 180.0));
            }
            px_res[j] = (pv.bits & 1u) ? 0xFFFFFFu : 0u;
            px_phi[j] = (unsigned)c_jet.bgr[g][0] | ((unsigned)c_jet.bgr[g][1] << 8) | ((unsigned)c_jet.bgr[g][2] << 16);
        }
        if (o_flow) {
            const double rmax = __longlong_as_double((long long)radmax[b]);
            if (f32) {
                // flow_to_color on a float32 array: every step up to the wheel coordinate in float32, np.pi rounded to float32
                const float rm = (float)rmax + 1e-5f;
                const float fu = (float)rv.x / rm, fv = (float)rv.y / rm;
                const float rad = sqrtf(fu * fu + fv * fv);
                const float a = (float)atan2(-(double)fv, -(double)fu) / 3.14159274f;
                const float fk = (a + 1.0f) / 2.0f * 54.0f;
                px_flow[j] = wheel_bgr((double)fk, (double)rad);
            } else {
                const double rm = rmax + 1e-5;
                const double nu = u / rm, nv = v / rm;
                const double rad = sqrt(nu * nu + nv * nv);
                const double a = atan2(-nv, -nu) / 3.141592653589793;
                px_flow[j] = wheel_bgr((a + 1.0) / 2.0 * 54.0, rad);
            }
        }
    }
    // 4 pixels x 3 bytes = 3 dwords at byte offset 3 * p0 (a multiple of 12); a partial tail or a misaligned image goes byte by byte
    uint8_t* outs[3] = {o_res, o_flow, o_phi};
    const unsigned* pxs[3] = {px_res, px_flow, px_phi};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint8_t* o = outs[k];
        if (!o) continue;
        const unsigned* px = pxs[k];
        if (p0 + 4 <= total && ((uintptr_t)o & 3) == 0) {
            uint32_t* d = (uint32_t*)(o + 3 * p0);
            d[0] = px[0] | (px[1] << 24);
            d[1] = (px[1] >> 8) | (px[2] << 16);
            d[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
            for (int j = 0; j < 4 && p0 + j < total; j++)
                for (int c = 0; c < 3; c++) o[3 * (p0 + j) + c] = (uint8_t)(px[j] >> (8 * c));
        }
    }
}

template <typename FlowT>
static void launch_render_t(hipStream_t st, const FlowT* flow, const DerotParams* derot, const double* foe, const uint8_t* sky, int B,
                            int W, int H, mav_thr_params thr, unsigned long long* radmax, uint8_t* res, uint8_t* flow_img, uint8_t* phi_img)
{
    if (!res && !flow_img && !phi_img) return;
    const size_t npx = (size_t)W * H;
    if (flow_img) {
        (void)hipMemsetAsync(radmax, 0, sizeof(unsigned long long) * B, st);
        const int gx = (int)std::min<size_t>((npx + 1023) / 1024, 256);   // up to 4 pixels per thread
        hipLaunchKernelGGL(k_render_radmax<FlowT>, dim3(gx, B), dim3(256), 0, st, flow, derot, W, H, radmax);
    }
    const size_t threads = (npx * B + 3) / 4;
    hipLaunchKernelGGL(k_render<FlowT>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, flow, derot, foe, sky, W, H, B, thr,
                       radmax, res, flow_img, phi_img);
}
void launch_render_f32(hipStream_t st, const float* flow, const DerotParams* derot, const double* foe, const uint8_t* sky, int B, int W,
                       int H, mav_thr_params thr, unsigned long long* radmax, uint8_t* res, uint8_t* flow_img, uint8_t* phi_img)
{
    launch_render_t<float>(st, flow, derot, foe, sky, B, W, H, thr, radmax, res, flow_img, phi_img);
}
void launch_render_f64(hipStream_t st, const double* flow, int B, int W, int H, unsigned long long* radmax, uint8_t* flow_img)
{
    launch_render_t<double>(st, flow, nullptr, nullptr, nullptr, B, W, H, mav_thr_params{}, radmax, nullptr, flow_img, nullptr);
}

// ------------------------------------------------------------------------------------------------------------
// The frame of processed.mp4 (src/processor.py:376-392 of the reference), (H, W, 3) u8 BGR per pair:
//   draw_FoE(frame, foe, [0, 255, 0]), then draw_FoE(frame, foe_gt, [255, 255, 255]): filled discs, white over green -> p
//   q = (150, 0, 150) where the fixed mask is set, p elsewhere
//   cv2.addWeighted(p, 0.2, q, 0.8, 0.0) = round((p + 4 q) / 5): the exact value's fraction is a multiple of .2, never a tie, so
//   (p + 4 q + 2) / 5 in integers is the byte float32 gives in any operation order (tests/test_overlay_cpu.py proves it)
// written[b] = the reference's np.sum(result_img) > 0: the mask is non-empty or a disc has a pixel inside the image.

// Half-width of row offset k (0 <= k <= r) of cv2.circle(thickness = -1, LINE_8, shift 0): OpenCV's integer midpoint routine
// Circle(..., fill = 1) emits spans [cx - dx, cx + dx] on rows cy +- dy and [cx - dy, cx + dy] on rows cy +- dx; a row is the widest
// of its spans (r = 10: 10 9 9 9 9 8 8 7 6 4 0).  Restated from the published routine: no image the reference wrote pins it.
static __device__ __forceinline__ int disc_half(int r, int k)
{
    int err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1, h = -1;
    while (dx >= dy) {
        if (dy == k) h = dx > h ? dx : h;
        if (dx == k) h = dy > h ? dy : h;
        dy++;
        err += plus;
        plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m;
        dx += m;
        minus -= m & 2;
    }
    return h;
}

// A centre draw_FoE draws: |v| <= 1e9 on both axes (NaN fails the test: not drawn), truncated toward zero as int() does.
struct Disc { int x, y, on; };
static __device__ __forceinline__ Disc disc_of(const double* c)
{
    const double x = c[0], y = c[1];
    Disc d;
    d.on = fabs(x) <= 1e9 && fabs(y) <= 1e9;
    d.x = d.on ? (int)x : 0;
    d.y = d.on ? (int)y : 0;
    return d;
}
static __device__ __forceinline__ bool in_disc(const Disc& d, int r, int x, int y)
{
    if (!d.on) return false;
    const int dy = y > d.y ? y - d.y : d.y - y, dx = x > d.x ? x - d.x : d.x - x;   // |centre| <= 1e9, r <= 4096: no overflow
    return dy <= r && dx <= r && dx <= disc_half(r, dy);        // the midpoint loop runs only in the disc's bounding square
}

// Four consecutive pixels of the batch per thread, as k_render: three dword loads of the frame, one of the mask, three dword stores.
// The flag: a workgroup whose 1024 pixels lie in one pair ORs its hits and stores once; one across pairs stores per pixel.
__global__ __launch_bounds__(256) void k_overlay(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ mask,
                                                 const double* __restrict__ foe, const double* __restrict__ foe_gt, int W, int H, int B,
                                                 int radius, uint8_t* __restrict__ out, uint8_t* __restrict__ written)
{
    const size_t npx = (size_t)W * H, total = npx * B;
    const size_t g0 = (size_t)blockIdx.x * 1024, g1 = g0 + 1023 < total ? g0 + 1023 : total - 1;
    const bool one_pair = g0 / npx == g1 / npx;
    const size_t p0 = g0 + (size_t)threadIdx.x * 4;
    bool hit_any = false;
    if (p0 < total) {
        const bool full = p0 + 4 <= total;
        unsigned px[4], mk = 0u;
        if (full && (((uintptr_t)frames | (uintptr_t)mask) & 3) == 0) {
            const uint32_t* s = (const uint32_t*)(frames + 3 * p0);
            const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
            px[0] = d0 & 0xFFFFFFu;
            px[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
            px[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
            px[3] = d2 >> 8;
            mk = *(const uint32_t*)(mask + p0);
        } else {
            for (int j = 0; j < 4; j++) {
                px[j] = 0u;
                if (p0 + j >= total) continue;
                const uint8_t* f = frames + 3 * (p0 + j);
                px[j] = (unsigned)f[0] | ((unsigned)f[1] << 8) | ((unsigned)f[2] << 16);
                mk |= (unsigned)mask[p0 + j] << (8 * j);
            }
        }
        unsigned res[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            res[j] = 0u;
            const size_t p = p0 + j;
            if (p >= total) continue;
            const int b = (int)(p / npx);
            const size_t q = p - (size_t)b * npx;
            const int y = (int)(q / W), x = (int)(q - (size_t)y * W);
            const bool green = in_disc(disc_of(foe + 2 * b), radius, x, y);
            const bool white = in_disc(disc_of(foe_gt + 2 * b), radius, x, y);
            const bool m = ((mk >> (8 * j)) & 0xFFu) != 0u;
            const unsigned pp = white ? 0xFFFFFFu : (green ? 0x00FF00u : px[j]);     // byte 0 = B: green is (0, 255, 0)
            const unsigned qq = m ? 0x960096u : pp;                                   // (150, 0, 150)
            unsigned o = 0u;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned a = (pp >> (8 * c)) & 0xFFu, e = (qq >> (8 * c)) & 0xFFu;
                o |= ((a + 4u * e + 2u) / 5u) << (8 * c);
            }
            res[j] = o;
            const bool hit = m || green || white;
            hit_any |= hit;
            if (hit && !one_pair) written[b] = 1;       // every such store writes the same value
        }
        if (full && ((uintptr_t)out & 3) == 0) {
            uint32_t* d = (uint32_t*)(out + 3 * p0);
            d[0] = res[0] | (res[1] << 24);
            d[1] = (res[1] >> 8) | (res[2] << 16);
            d[2] = (res[2] >> 16) | (res[3] << 8);
        } else {
            for (int j = 0; j < 4 && p0 + j < total; j++)
                for (int c = 0; c < 3; c++) out[3 * (p0 + j) + c] = (uint8_t)(res[j] >> (8 * c));
        }
    }
    if (one_pair && __syncthreads_or(hit_any) && threadIdx.x == 0) written[g0 / npx] = 1;   // one_pair is uniform in the workgroup
}

void launch_overlay(hipStream_t st, const uint8_t* frames, const uint8_t* mask, const double* foe, const double* foe_gt, int B, int W, int H,
                    int radius, uint8_t* out, uint8_t* written)
{
    (void)hipMemsetAsync(written, 0, (size_t)B, st);
    const size_t threads = ((size_t)W * H * B + 3) / 4;
    hipLaunchKernelGGL(k_overlay, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, frames, mask, foe, foe_gt, W, H, B, radius, out,
                       written);
}

// cv2.applyColorMap(img, COLORMAP_JET) of a single-channel u8 image: the LUT.  (A 3-channel image goes through BGR2GRAY first, as
// in OpenCV; mav_bgr2gray.)
__global__ __launch_bounds__(256) void k_colormap_jet(const uint8_t* __restrict__ gray, size_t n, uint8_t* __restrict__ bgr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned g = gray[i];
    bgr[3 * i] = c_jet.bgr[g][0]; bgr[3 * i + 1] = c_jet.bgr[g][1]; bgr[3 * i + 2] = c_jet.bgr[g][2];
}
void launch_colormap_jet(hipStream_t st, const uint8_t* gray, size_t n, uint8_t* bgr)
{
    if (n) hipLaunchKernelGGL(k_colormap_jet, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gray, n, bgr);
}

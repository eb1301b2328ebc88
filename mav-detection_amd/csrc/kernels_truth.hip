// Ground-truth flow from depth and pose, and the radial-error histogram of a flow against it (include/mavflow_truth.h).
// Compiled with -ffp-contract=off: every product and sum below is one IEEE operation, in the order tests/truth_ref.py restates and
// the reference's numpy evaluates (src/airsim_optical_flow.py:12-107, src/processor.py:267-275, src/plot_radial_error.py:38-39).
#include "mavflow_internal.h"
#include "../../include/mavflow_truth.h"

// ---- mav_gt_flow ------------------------------------------------------------------------------------------------------------------------
// mat4x4_vec4_mult's row: ((m0*a + m1*b) + m2*c) + m3*d, left to right as numpy adds the four products.
__device__ __forceinline__ double row4(const double* m, double a, double b, double c, double d)
{
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3] * d;
}
__device__ __forceinline__ void store_uv(double2* out, size_t i, double u, double v)
{
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    out[i] = make_double2(u != u ? qnan : u, v != v ? qnan : v);
}
__device__ __forceinline__ void store_uv(float2* out, size_t i, double u, double v)
{
    const float qnan = __uint_as_float(0x7FC00000u), fu = (float)u, fv = (float)v;       // round to nearest even, as astype(float32)
    out[i] = make_float2(fu != fu ? qnan : fu, fv != fv ? qnan : fv);
}
// One thread per pixel, 256 consecutive pixels per workgroup, grid-strided over the image (blockIdx.z = the pair).  The parameter
// block is read through a uniform address: scalar loads, once per workgroup.
template <typename OutT>
__global__ __launch_bounds__(256) void k_gt_flow(const float* __restrict__ depth, const uint8_t* __restrict__ seg,
                                                 const mav_gt_flow_params* __restrict__ params, int W, int H, OutT* __restrict__ out)
{
    const int b = blockIdx.z;
    const unsigned npx = (unsigned)W * (unsigned)H;
    const mav_gt_flow_params* P = params + b;
    const double* Mi = P->view_proj_inv;
    const double* Mp = P->view_proj_prev;
    const double dx = P->displacement[0], dy = P->displacement[1], dz = P->displacement[2];
    const float scale = P->depth_scale;
    const float* dep = depth + (size_t)b * npx;
    const uint8_t* sg = seg ? seg + (size_t)b * npx : nullptr;
    OutT* o = out + (size_t)b * npx;
    const double dW = (double)W, dH = (double)H;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npx; p += gridDim.x * 256u) {
        const unsigned yi = p / (unsigned)W, xi = p - yi * (unsigned)W;
        const float zf = dep[p] * scale;                          // the reference's float32 product
        const bool mav = sg && sg[p] > 0;
        const double x = (double)xi, y = (double)yi;
        // screen_to_world
        const double nx = x / dW, ny = y / dH;
        const double sx = 2.0 * (nx - 0.5), sy = 2.0 * ((1.0 - ny) - 0.5);
        const double s3 = row4(Mi + 12, sx, sy, 1.0, 1.0), e3 = row4(Mi + 12, sx, sy, 0.5, 1.0);
        double S[3], D[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            S[i] = row4(Mi + 4 * i, sx, sy, 1.0, 1.0) / s3;
            const double E = row4(Mi + 4 * i, sx, sy, 0.5, 1.0) / e3;
            D[i] = E - S[i];
        }
        const double n = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
        const double z = (double)zf;
        double P0 = S[0] + (D[0] / n) * z, P1 = S[1] + (D[1] / n) * z, P2 = S[2] + (D[2] / n) * z;
        if (mav) { P0 = P0 - dx; P1 = P1 - dy; P2 = P2 - dz; }
        // world_to_screen
        const double p0 = row4(Mp, P0, P1, P2, 1.0), p1 = row4(Mp + 4, P0, P1, P2, 1.0), p3 = row4(Mp + 12, P0, P1, P2, 1.0);
        const double rhw = 1.0 / p3;
        const double px = p0 * rhw, py = p1 * rhw;
        const double rx = (px * 0.5 + 0.5) * dW - x, ry = ((-py) * 0.5 + 0.5) * dH - y;
        store_uv(o, p, -rx, -ry);
    }
}
void launch_gt_flow(hipStream_t st, const float* depth, const uint8_t* seg, const void* params_, int B, int W, int H, bool out_f64, void* out)
{
    const mav_gt_flow_params* params = (const mav_gt_flow_params*)params_;
    const size_t npx = (size_t)W * H;
    const size_t nblk = (npx + 255) / 256;
    const dim3 grid((unsigned)(nblk < MAV_GT_FLOW_GRID_CAP ? nblk : MAV_GT_FLOW_GRID_CAP), 1, B);
    if (out_f64)
        hipLaunchKernelGGL(k_gt_flow<double2>, grid, dim3(256), 0, st, depth, seg, params, W, H, (double2*)out);
    else
        hipLaunchKernelGGL(k_gt_flow<float2>, grid, dim3(256), 0, st, depth, seg, params, W, H, (float2*)out);
}

// ---- mav_radial_error_hist ----------------------------------------------------------------------------------------------------------------
// A checked edge list travels to the context's device copy as a kernel argument (2 KB by value): stream-ordered, nothing of the
// caller's memory is read after the entry point returns.
__global__ void k_radial_edges(RadialEdges e, double* __restrict__ dst)
{
    for (int i = threadIdx.x; i < e.n; i += blockDim.x) dst[i] = e.e[i];
}
// numpy.histogram2d's bin of t among n sorted edges: k with e[k] <= t < e[k+1], the last bin closed on the right; -1 outside or NaN.
__device__ __forceinline__ int radial_bin(const double* e, int n, double t)
{
    if (!(t >= e[0]) || !(t <= e[n - 1])) return -1;
    int lo = 0, hi = n - 1;                      // e[lo] <= t, and t < e[hi] or hi == n - 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// Workgroup = 1024 threads, 2048 consecutive pixels per step (two per thread, 1024 apart), grid-strided; blockIdx.z = the pair.  The
// two edge lists sit in LDS.  LDS_COUNTS: the cells are uint32 counters of the workgroup's own in LDS, flushed once, non-zero cells
// only, with 64-bit atomics; otherwise (more cells than LDS holds) the adds go to the table directly.  In both forms a wave whose
// counted pixels all fall into ONE cell adds their number once (real fields pile up in a few cells; 64 same-address atomics would
// serialise).  Integer counts: the table does not depend on the order of the additions.
template <bool LDS_COUNTS>
__global__ __launch_bounds__(1024) void k_radial_hist(const float2* __restrict__ flow, const float2* __restrict__ gt,
                                                      const uint8_t* __restrict__ sky, unsigned npx, const double* __restrict__ edges, int nm,
                                                      int ne, unsigned long long* __restrict__ table)
{
    extern __shared__ double sm[];
    __shared__ unsigned part[16][2];
    double* em = sm;
    double* ee = sm + nm;
    unsigned* cnt = (unsigned*)(sm + nm + ne);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.z;
    const int bj = ne - 1, cells = (nm - 1) * bj;
    for (int i = tid; i < nm + ne; i += 1024) sm[i] = edges[i];
    if (LDS_COUNTS)
        for (int i = tid; i < cells; i += 1024) cnt[i] = 0u;
    __syncthreads();
    const float2* fl = flow + (size_t)b * npx;
    const float2* g = gt + (size_t)b * npx;
    const uint8_t* sk = sky ? sky + (size_t)b * npx : nullptr;
    const float rad2deg = 180.0f / 3.14159265358979323846f;       // numpy's float32 loop: x * (180.0f / NPY_PIf)
    unsigned non_sky = 0u, in_range = 0u;
    for (unsigned base = blockIdx.x * 2048u; base < npx; base += gridDim.x * 2048u) {
        float2 f[2], t[2];
        unsigned s[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const unsigned p = base + k * 1024u + tid;
            const unsigned q = p < npx ? p : npx - 1u;            // past the end: re-read the last pixel, never counted
            f[k] = fl[q];
            t[k] = g[q];
            s[k] = sk ? sk[q] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const unsigned p = base + k * 1024u + tid;
            int key = -1;
            if (p < npx && s[k] == 0u) {
                non_sky++;
                const float mag = sqrtf(f[k].x * f[k].x + f[k].y * f[k].y);
                const float err = (atan2f(f[k].y, f[k].x) - atan2f(t[k].y, t[k].x)) * rad2deg;
                const int i = radial_bin(em, nm, (double)mag);
                if (i >= 0) {
                    const int j = radial_bin(ee, ne, (double)err);
                    if (j >= 0) { key = i * bj + j; in_range++; }
                }
            }
            // every lane of the wave arrives here (the step loop's bounds are uniform)
            const unsigned long long any = __ballot(key >= 0);
            if (any) {
                const int first = __shfl(key, __ffsll((long long)any) - 1);
                if (__ballot(key >= 0 && key != first) == 0ull) {
                    if (lane == 0) {
                        const unsigned c = (unsigned)__popcll(any);
                        if (LDS_COUNTS) atomicAdd(&cnt[first], c); else atomicAdd(&table[2 + first], (unsigned long long)c);
                    }
                } else if (key >= 0) {
                    if (LDS_COUNTS) atomicAdd(&cnt[key], 1u); else atomicAdd(&table[2 + key], 1ull);
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { non_sky += __shfl_xor(non_sky, o); in_range += __shfl_xor(in_range, o); }
    if (lane == 0) { part[wv][0] = non_sky; part[wv][1] = in_range; }
    __syncthreads();                                              // ... and every wave's counter updates
    if (tid < 2) {
        unsigned long long v = 0ull;
        for (int w = 0; w < 16; w++) v += part[w][tid];
        if (v) atomicAdd(&table[tid], v);
    }
    if (LDS_COUNTS)
        for (int i = tid; i < cells; i += 1024) {
            const unsigned v = cnt[i];
            if (v) atomicAdd(&table[2 + i], (unsigned long long)v);
        }
}
bool radial_hist_lds_counts(int nm, int ne) { return (size_t)(nm - 1) * (ne - 1) <= MAV_RADIAL_LDS_CELLS; }
int radial_hist_grid(size_t npx, int B)
{
    const size_t nblk = (npx + 2047) / 2048;
    const int cap = MAV_RADIAL_GRID_CAP / B > 0 ? MAV_RADIAL_GRID_CAP / B : 1;
    return (int)(nblk < (size_t)cap ? nblk : (size_t)cap);
}
hipError_t launch_radial_hist(hipStream_t st, const float* flow, const float* gt, const uint8_t* sky, int B, int W, int H, const RadialEdges& mag,
                              const RadialEdges& err, double* edges_dev, bool edges_resident, unsigned long long* table)
{
    const size_t npx = (size_t)W * H;
    const int nm = mag.n, ne = err.n;
    const bool lds = radial_hist_lds_counts(nm, ne);
    const size_t shmem = sizeof(double) * (nm + ne) + (lds ? sizeof(unsigned) * (size_t)(nm - 1) * (ne - 1) : 0);
    if (lds) {                                   // more than the 64 KB a kernel gets unasked
        const hipError_t e = hipFuncSetAttribute((const void*)k_radial_hist<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
    }
    if (!edges_resident) {
        hipLaunchKernelGGL(k_radial_edges, dim3(1), dim3(256), 0, st, mag, edges_dev);
        hipLaunchKernelGGL(k_radial_edges, dim3(1), dim3(256), 0, st, err, edges_dev + nm);
    }
    const dim3 grid(radial_hist_grid(npx, B), 1, B);
    if (lds)
        hipLaunchKernelGGL(k_radial_hist<true>, grid, dim3(1024), shmem, st, (const float2*)flow, (const float2*)gt, sky, (unsigned)npx, edges_dev,
                           nm, ne, table);
    else
        hipLaunchKernelGGL(k_radial_hist<false>, grid, dim3(1024), shmem, st, (const float2*)flow, (const float2*)gt, sky, (unsigned)npx, edges_dev,
                           nm, ne, table);
    return hipSuccess;
}

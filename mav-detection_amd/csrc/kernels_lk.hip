// Sparse optical flow for gfx950: Shi-Tomasi corners (cv2.goodFeaturesToTrack) and the pyramidal Lucas-Kanade tracker
// (cv2.calcOpticalFlowPyrLK, 8-bit path), restated from OpenCV's published routines.
//
// Rule of the file: every sum over a window is an EXACT INTEGER sum, converted to float32 once.  What remains per pixel / per point
// is a handful of scalar IEEE float32 operations in a fixed order (compiled with -ffp-contract=off; float division and sqrtf are
// hipcc's correctly rounded default forms), so the results do not depend on how a wavefront splits a window and a plain numpy
// restatement (tests/lk_ref.py) reproduces them bit for bit.
#include <float.h>

#include "mavflow_internal.h"

// BORDER_REFLECT_101 for any p (a window may leave a small level by more than its size)
__device__ __forceinline__ int refl101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// order-preserving float <-> unsigned key (atomicMax over floats of either sign); key 0 is below every float
__device__ __forceinline__ unsigned key_of(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- corners: cornerMinEigenVal -------------------------------------------------------------------------------------------------
// One 16 x 16 tile per workgroup.  Sobel 3x3 pairs of the tile and its halo of r = block / 2 go to LDS as int16 (|d| <= 1020); the
// derivative at a halo position outside the image is the derivative AT the REFLECT_101 position (boxFilter reflects the product
// images, which is not the derivative of the reflected frame: dx * dy would change sign).  Box sums of dx*dx, dx*dy, dy*dy are
// separable integer sums (<= 225 x 1020^2 < 2^31), then five float32 operations.  The tile's maximum goes to *maxkey; with a mask
// (cv2's minMaxLoc(eig, ..., mask)) only pixels whose mask byte is non-zero take part in it, the map itself is the whole map.
//
// The score is a compile-time policy of the kernel: it holds the kernel's float argument(s) and turns a pixel's three box sums into the
// map's value.  Everything before it (Sobel, halo, box sums) and after it (the store, the masked maximum) is the one body.
//   MinEigScore     cornerMinEigenVal, five float32 operations (mav_good_features and every form of it)
//   HarrisScore     cornerHarris as goodFeaturesToTrack(useHarrisDetector = true) calls it: the same sums and the same scale, then
//                   a = xx s2, b = xy s2, c = yy s2, t = a + c, (a c - b b) - (k t) t, float32 in this order with k rounded to float32
//                   once (the form of OpenCV's vector path).  Responses may be negative: key_of orders floats of either sign.
#define EIG_TILE 16
#define EIG_MAX_R 7
#define EIG_T (EIG_TILE + 2 * EIG_MAX_R)
struct MinEigScore {
    float s2;
    __device__ __forceinline__ float operator()(int xx, int xy, int yy) const
    {
        const float a = (float)xx * s2 * 0.5f, b = (float)xy * s2, c = (float)yy * s2 * 0.5f;
        return (a + c) - sqrtf((a - c) * (a - c) + b * b);
    }
};
struct HarrisScore {
    float s2, k;
    __device__ __forceinline__ float operator()(int xx, int xy, int yy) const
    {
        const float a = (float)xx * s2, b = (float)xy * s2, c = (float)yy * s2, t = a + c;
        return (a * c - b * b) - (k * t) * t;
    }
};
template <typename Score>
__global__ __launch_bounds__(256) void k_min_eig(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int W, int H, int r, Score score,
                                                 float* __restrict__ eig, unsigned* __restrict__ maxkey)
{
    __shared__ short2 d[EIG_T * EIG_T];
    __shared__ int hs[3][EIG_T * EIG_TILE];
    __shared__ unsigned wmax[4];
    const int tid = threadIdx.x, T = EIG_TILE + 2 * r, bs = 2 * r + 1;
    const int x0 = blockIdx.x * EIG_TILE, y0 = blockIdx.y * EIG_TILE;
    for (int k = tid; k < T * T; k += 256) {
        const int ty = k / T, tx = k - ty * T;
        const int gx = refl101(x0 - r + tx, W), gy = refl101(y0 - r + ty, H);
        const int xm = refl101(gx - 1, W), xp = refl101(gx + 1, W);
        const uint8_t* rm = img + (size_t)refl101(gy - 1, H) * W;
        const uint8_t* r0 = img + (size_t)gy * W;
        const uint8_t* rp = img + (size_t)refl101(gy + 1, H) * W;
        const int dx = ((int)rm[xp] + 2 * (int)r0[xp] + (int)rp[xp]) - ((int)rm[xm] + 2 * (int)r0[xm] + (int)rp[xm]);
        const int dy = ((int)rp[xm] + 2 * (int)rp[gx] + (int)rp[xp]) - ((int)rm[xm] + 2 * (int)rm[gx] + (int)rm[xp]);
        d[k] = make_short2((short)dx, (short)dy);
    }
    __syncthreads();
    for (int k = tid; k < T * EIG_TILE; k += 256) {
        const int ty = k / EIG_TILE, ox = k - ty * EIG_TILE;
        int xx = 0, xy = 0, yy = 0;
        for (int i = 0; i < bs; i++) {
            const short2 v = d[ty * T + ox + i];
            xx += (int)v.x * v.x; xy += (int)v.x * v.y; yy += (int)v.y * v.y;
        }
        hs[0][k] = xx; hs[1][k] = xy; hs[2][k] = yy;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4, x = x0 + tx, y = y0 + ty;
    unsigned key = 0;
    if (x < W && y < H) {
        int xx = 0, xy = 0, yy = 0;
        for (int j = 0; j < bs; j++) {
            const int k = (ty + j) * EIG_TILE + tx;
            xx += hs[0][k]; xy += hs[1][k]; yy += hs[2][k];
        }
        const float e = score(xx, xy, yy);
        eig[(size_t)y * W + x] = e;
        if (!mask || mask[(size_t)y * W + x]) key = key_of(e);
    }
    for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(key, m); key = o > key ? o : key; }
    if ((tid & 63) == 0) wmax[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; i++) key = wmax[i] > key ? wmax[i] : key;
        atomicMax(maxkey, key);
    }
}

// threshold (eig > max * qualityLevel), the 3x3 non-maximum test on interior pixels, atomic append of (value bits, linear index).
// *count keeps counting past cap: the pick reports the capacity needed.  The append order is arbitrary; the pick's total order is not.
// A masked-out pixel is no candidate but still suppresses its neighbours; an all-zero mask leaves *maxkey at 0 = NaN: no candidate.
__global__ __launch_bounds__(256) void k_corner_candidates(const float* __restrict__ eig, const uint8_t* __restrict__ mask, int W, int H,
                                                           const unsigned* __restrict__ maxkey, double quality, uint2* __restrict__ cand,
                                                           unsigned* __restrict__ count, unsigned cap)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)W * H) return;
    const int y = (int)(idx / W), x = (int)(idx - (size_t)y * W);
    if (x < 1 || x > W - 2 || y < 1 || y > H - 2) return;
    if (mask && !mask[idx]) return;
    const float thr = (float)((double)float_of(*maxkey) * quality);
    const float v = eig[idx];
    if (!(v > thr)) return;
    for (int j = -1; j <= 1; j++)
        for (int i = -1; i <= 1; i++)
            if (eig[idx + (ptrdiff_t)j * W + i] > v) return;
    const unsigned slot = atomicAdd(count, 1u);
    if (slot < cap) cand[slot] = make_uint2(__float_as_uint(v), (unsigned)idx);
}

void launch_min_eig(hipStream_t st, const uint8_t* img, const uint8_t* mask, int W, int H, int block_size, float s2, float* eig, unsigned* maxkey)
{
    dim3 grid((W + EIG_TILE - 1) / EIG_TILE, (H + EIG_TILE - 1) / EIG_TILE);
    hipLaunchKernelGGL(k_min_eig<MinEigScore>, grid, dim3(256), 0, st, img, mask, W, H, block_size / 2, MinEigScore{s2}, eig, maxkey);
}
void launch_harris(hipStream_t st, const uint8_t* img, const uint8_t* mask, int W, int H, int block_size, float s2, float k, float* eig,
                   unsigned* maxkey)
{
    dim3 grid((W + EIG_TILE - 1) / EIG_TILE, (H + EIG_TILE - 1) / EIG_TILE);
    hipLaunchKernelGGL(k_min_eig<HarrisScore>, grid, dim3(256), 0, st, img, mask, W, H, block_size / 2, HarrisScore{s2, k}, eig, maxkey);
}
void launch_corner_candidates(hipStream_t st, const float* eig, const uint8_t* mask, int W, int H, const unsigned* maxkey, double quality,
                              uint2* cand, unsigned* count, unsigned cap)
{
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(k_corner_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, eig, mask, W, H, maxkey, quality, cand, count, cap);
}

// ---- corners: the sort and the greedy minimum-distance pick ----------------------------------------------------------------------
// Every launch below is enqueued without the host knowing the candidate count n: kernels read it from *n_ptr, and workgroups (whole
// launches, for a small n) beyond it leave.  n > cap (overflow) makes every sort kernel leave and the pick report -n.
//
// Sort: bitonic, in place, descending by the key (value bits << 32) | linear index, over Np = n rounded up to a power of two (cap is
// one); the first launch turns cand[n .. Np) into zero keys, which sort behind every candidate.  Strides below PICK_SORT_CHUNK run in
// LDS (32 KB of keys per workgroup), the others as one launch per (k, j) step.
#define PICK_SORT_CHUNK 4096u
#define PICK_WG 1024
__device__ __forceinline__ unsigned long long pick_key(uint2 c) { return ((unsigned long long)c.x << 32) | c.y; }
__device__ __forceinline__ uint2 pick_unkey(unsigned long long k) { return make_uint2((unsigned)(k >> 32), (unsigned)k); }
__device__ __forceinline__ unsigned pick_np2(unsigned n) { return n <= 1 ? 1u : 1u << (32 - __clz(n - 1)); }

// k_from == 0: the chunk's own sort, k = 2 .. min(Np, chunk).  Otherwise the strides chunk / 2 .. 1 of merge step k = k_from.
__global__ __launch_bounds__(PICK_WG) void k_pick_sort_local(uint2* __restrict__ cand, const unsigned* __restrict__ n_ptr, unsigned cap, unsigned k_from)
{
    __shared__ unsigned long long s[PICK_SORT_CHUNK];
    const unsigned n = *n_ptr;
    if (n > cap) return;
    const unsigned Np = pick_np2(n), base = blockIdx.x * PICK_SORT_CHUNK;
    if (k_from > Np || base >= Np) return;
    const unsigned L = Np < PICK_SORT_CHUNK ? Np : PICK_SORT_CHUNK, tid = threadIdx.x;
    for (unsigned t = tid; t < L; t += PICK_WG) s[t] = base + t < n || k_from ? pick_key(cand[base + t]) : 0ull;
    __syncthreads();
    for (unsigned k = k_from ? k_from : 2; k <= (k_from ? k_from : L); k <<= 1)
        for (unsigned j = (k >> 1) < (L >> 1) ? (k >> 1) : (L >> 1); j > 0; j >>= 1) {
            for (unsigned t = tid; t < (L >> 1); t += PICK_WG) {
                const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool desc = ((base + i) & k) == 0;
                const unsigned long long a = s[i], b = s[l];
                if ((a < b) == desc) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    for (unsigned t = tid; t < L; t += PICK_WG) cand[base + t] = pick_unkey(s[t]);
}
// one compare-exchange step (k, j) with j >= PICK_SORT_CHUNK: a thread owns the pair (i, i | j)
__global__ __launch_bounds__(256) void k_pick_sort_global(uint2* __restrict__ cand, const unsigned* __restrict__ n_ptr, unsigned cap, unsigned k, unsigned j)
{
    const unsigned n = *n_ptr;
    if (n > cap) return;
    const unsigned Np = pick_np2(n), t = blockIdx.x * 256 + threadIdx.x;
    if (k > Np || t >= (Np >> 1)) return;
    const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const unsigned long long a = pick_key(cand[i]), b = pick_key(cand[l]);
    if ((a < b) == ((i & k) == 0)) { cand[i] = pick_unkey(b); cand[l] = pick_unkey(a); }
}
void launch_pick_sort(hipStream_t st, uint2* cand, const unsigned* n_ptr, unsigned cap)
{
    const unsigned chunks = (cap + PICK_SORT_CHUNK - 1) / PICK_SORT_CHUNK;
    hipLaunchKernelGGL(k_pick_sort_local, dim3(chunks), dim3(PICK_WG), 0, st, cand, n_ptr, cap, 0u);
    for (unsigned k = 2 * PICK_SORT_CHUNK; k <= cap; k <<= 1) {
        for (unsigned j = k >> 1; j >= PICK_SORT_CHUNK; j >>= 1)
            hipLaunchKernelGGL(k_pick_sort_global, dim3((cap / 2 + 255) / 256), dim3(256), 0, st, cand, n_ptr, cap, k, j);
        hipLaunchKernelGGL(k_pick_sort_local, dim3(chunks), dim3(PICK_WG), 0, st, cand, n_ptr, cap, k);
    }
}

// Pick: ONE workgroup walks the sorted candidates in chunks of PICK_WG ranks.  Accepted corners of earlier chunks live in a grid of
// cells of `cell` = ceil(min_distance) pixels (a.grid, zeroed by the caller; slot = linear index + 1, filled front to back): a corner
// nearer than min_distance lies in one of the 3 x 3 cells around, and a cell holds at most `slots` corners (pairwise >= min_distance
// apart inside cell x cell pixels: 1 for cell 1, 2 for cell 2, at most 4 otherwise -- one per quadrant).  Per chunk:
//   1. a candidate in range of a grid corner is rejected; the others (survivors) are compacted in rank order into LDS;
//   2. rounds over the survivors: undecided -> rejected if an earlier survivor in range is accepted, accepted if every earlier
//      survivor in range is rejected (or there is none), otherwise it waits at that survivor.  Decisions are final, so reading a state
//      while its owner writes it only delays; the first undecided survivor always decides, so a chunk needs at most PICK_WG rounds;
//   3. the accepted ones take the next output places in rank order (cut at max_corners) and go into the grid.
// The loop ends with the candidates or with max_corners accepted: exactly the sequential greedy rule with its early stop.
__device__ __forceinline__ bool pick_in_range(int x, int y, int ox, int oy, double md2)
{
    const double dx = x - ox, dy = y - oy;
    return dx * dx + dy * dy < md2;
}
__global__ __launch_bounds__(PICK_WG) void k_corner_pick(LkPickArgs a)
{
    __shared__ int s_x[PICK_WG], s_y[PICK_WG], s_state[PICK_WG];
    __shared__ int s_wcount[PICK_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = a.W, maxc = a.max_corners;
    const unsigned n = *a.n_ptr;
    if (n > a.cap) {                                          // overflow: the count, negated, and no corner
        if (tid == 0) { *a.count = -(int)n; a.stats[0] = 0; a.stats[1] = 0; }
        return;
    }
    if (!a.pick) {                                            // min_distance < 1: the first max_corners in key order
        const unsigned m = n < (unsigned)maxc ? n : (unsigned)maxc;
        for (unsigned i = tid; i < m; i += PICK_WG) {
            const unsigned idx = a.cand[i].y, y = idx / (unsigned)W;
            a.corners[2 * i] = (float)(idx - y * W); a.corners[2 * i + 1] = (float)y;
        }
        if (tid == 0) { *a.count = (int)m; a.stats[0] = 0; a.stats[1] = 0; }
        return;
    }
    int acc = 0;
    unsigned chunks = 0, rounds = 0;
    for (unsigned base = 0; base < n && acc < maxc; base += PICK_WG, chunks++) {
        const unsigned r = base + tid;
        int x = 0, y = 0;
        bool alive = false;
        if (r < n) {
            const unsigned idx = a.cand[r].y;
            y = (int)(idx / (unsigned)W); x = (int)(idx - (unsigned)y * W);
            alive = true;
            const int cx = x / a.cell, cy = y / a.cell;
            const int y1 = cy + 1 < a.gh ? cy + 1 : a.gh - 1, x1 = cx + 1 < a.gw ? cx + 1 : a.gw - 1;
            for (int yy = cy > 0 ? cy - 1 : 0; alive && yy <= y1; yy++)
                for (int xx = cx > 0 ? cx - 1 : 0; alive && xx <= x1; xx++) {
                    const unsigned* cellp = a.grid + ((size_t)yy * a.gw + xx) * a.slots;
                    for (int s = 0; s < a.slots; s++) {
                        // the slot may have been written by another wave of this workgroup one chunk ago: read it at the L2
                        const unsigned v = __hip_atomic_load(cellp + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (!v) break;
                        const int oy = (int)((v - 1) / (unsigned)W), ox = (int)((v - 1) - (unsigned)oy * W);
                        if (pick_in_range(x, y, ox, oy, a.md2)) { alive = false; break; }
                    }
                }
        }
        // survivors, compacted in rank order
        unsigned long long bal = __ballot(alive);
        if (lane == 0) s_wcount[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, S = 0;
        for (int w = 0; w < PICK_WG / 64; w++) { if (w < wv) off += s_wcount[w]; S += s_wcount[w]; }
        if (alive) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1));
            s_x[pos] = x; s_y[pos] = y; s_state[pos] = 0;
        }
        __syncthreads();
        // rounds: thread t owns survivor t.  state 0 undecided, 1 accepted, 2 rejected
        const bool mine = tid < S;
        const int mx = mine ? s_x[tid] : 0, my = mine ? s_y[tid] : 0;
        int st = 0, ptr = 0;
        for (;;) {
            if (mine && st == 0) {
                while (ptr < tid) {
                    if (pick_in_range(mx, my, s_x[ptr], s_y[ptr], a.md2)) {
                        const int o = __hip_atomic_load(&s_state[ptr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (o == 1) st = 2;
                        if (o != 2) break;
                    }
                    ptr++;
                }
                if (st == 0 && ptr == tid) st = 1;
                if (st) __hip_atomic_store(&s_state[tid], st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            rounds++;
            if (!__syncthreads_or(mine && st == 0)) break;
        }
        // output places in rank order
        const bool isacc = mine && st == 1;
        bal = __ballot(isacc);
        if (lane == 0) s_wcount[wv] = __popcll(bal);
        __syncthreads();
        off = 0;
        int T = 0;
        for (int w = 0; w < PICK_WG / 64; w++) { if (w < wv) off += s_wcount[w]; T += s_wcount[w]; }
        const int o = acc + off + __popcll(bal & ((1ull << lane) - 1));
        if (isacc && o < maxc) {
            a.corners[2 * o] = (float)mx; a.corners[2 * o + 1] = (float)my;
            unsigned* cellp = a.grid + ((size_t)(my / a.cell) * a.gw + mx / a.cell) * a.slots;
            const unsigned v = (unsigned)my * (unsigned)W + (unsigned)mx + 1u;
            for (int s = 0; s < a.slots; s++)
                if (atomicCAS(cellp + s, 0u, v) == 0u) break;
        }
        acc += T;
        __threadfence();
        __syncthreads();
    }
    if (tid == 0) { *a.count = acc < maxc ? acc : maxc; a.stats[0] = chunks; a.stats[1] = rounds; }
}
void launch_corner_pick(hipStream_t st, const LkPickArgs& a) { hipLaunchKernelGGL(k_corner_pick, dim3(1), dim3(PICK_WG), 0, st, a); }

// ---- pyramid: pyrDown, 5x5 [1 4 6 4 1] x [1 4 6 4 1], REFLECT_101, (sum + 128) >> 8 -----------------------------------------------
__global__ __launch_bounds__(256) void k_lk_pyrdown(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    int xs[5];
    for (int i = 0; i < 5; i++) xs[i] = refl101(2 * x - 2 + i, sw);
    const int kw[5] = {1, 4, 6, 4, 1};
    int sum = 0;
    for (int j = 0; j < 5; j++) {
        const uint8_t* row = src + (size_t)refl101(2 * y - 2 + j, sh) * sw;
        sum += kw[j] * ((int)row[xs[0]] + 4 * (int)row[xs[1]] + 6 * (int)row[xs[2]] + 4 * (int)row[xs[3]] + (int)row[xs[4]]);
    }
    dst[(size_t)y * dw + x] = (uint8_t)((sum + 128) >> 8);
}
void launch_lk_pyrdown(hipStream_t st, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh)
{
    hipLaunchKernelGGL(k_lk_pyrdown, dim3((dw + 63) / 64, (dh + 3) / 4), dim3(256), 0, st, src, sw, sh, dst, dw, dh);
}

// Scharr pairs (Ix, Iy) as int16 of every level of one pyramid in one launch (blockIdx.y = level), REFLECT_101 at the image edge
__global__ __launch_bounds__(256) void k_lk_scharr(const uint8_t* __restrict__ pyr, LkLevels lv, short2* __restrict__ out)
{
    const int level = blockIdx.y, w = lv.w[level], h = lv.h[level];
    const size_t n = (size_t)w * h;
    const uint8_t* img = pyr + lv.off[level];
    short2* o = out + lv.off[level];
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
        const int y = (int)(idx / w), x = (int)(idx - (size_t)y * w);
        const int xm = refl101(x - 1, w), xp = refl101(x + 1, w);
        const uint8_t* rm = img + (size_t)refl101(y - 1, h) * w;
        const uint8_t* r0 = img + (size_t)y * w;
        const uint8_t* rp = img + (size_t)refl101(y + 1, h) * w;
        // t0 = 3 (r[y-1] + r[y+1]) + 10 r[y], t1 = r[y+1] - r[y-1] per column
        const int t0m = 3 * ((int)rm[xm] + (int)rp[xm]) + 10 * (int)r0[xm], t0p = 3 * ((int)rm[xp] + (int)rp[xp]) + 10 * (int)r0[xp];
        const int t1m = (int)rp[xm] - (int)rm[xm], t10 = (int)rp[x] - (int)rm[x], t1p = (int)rp[xp] - (int)rm[xp];
        o[idx] = make_short2((short)(t0p - t0m), (short)(3 * (t1m + t1p) + 10 * t10));
    }
}
void launch_lk_scharr(hipStream_t st, const uint8_t* pyr, const LkLevels& lv, int levels, short2* out)
{
    size_t blocks = ((size_t)lv.w[0] * lv.h[0] + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_lk_scharr, dim3((unsigned)blocks, levels), dim3(256), 0, st, pyr, lv, out);
}

// ---- tracker ----------------------------------------------------------------------------------------------------------------------
// One 64-lane wavefront per point, four points per workgroup, every level of a point inside the one launch.  A lane owns the window
// pixels k = lane, lane + 64, ...: it writes their I / dIx / dIy (int16) to the point's LDS block and is the only one to read them
// back, so no barrier is needed and a wave whose point has converged simply leaves.  Window sums are per-lane int64 partials reduced
// through __shfl_xor.  Floor of a coordinate is tested in float before it is converted: NaN, inf and anything outside the level fail
// the bounds test (cv2's cvFloor gives INT_MIN there) and never index memory.
struct LkWeights { int w00, w01, w10, w11; };
__device__ __forceinline__ LkWeights lk_weights(float a, float b)
{
    LkWeights q;
    q.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    q.w01 = (int)rintf(a * (1.f - b) * 16384.f);
    q.w10 = (int)rintf((1.f - a) * b * 16384.f);
    q.w11 = 16384 - q.w00 - q.w01 - q.w10;
    return q;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int lk_image_value(const uint8_t* __restrict__ img, int w, int h, int x, int y, const LkWeights& q)
{
    const int xa = refl101(x, w), xb = refl101(x + 1, w);
    const uint8_t* ra = img + (size_t)refl101(y, h) * w;
    const uint8_t* rb = img + (size_t)refl101(y + 1, h) * w;
    return ((int)ra[xa] * q.w00 + (int)ra[xb] * q.w01 + (int)rb[xa] * q.w10 + (int)rb[xb] * q.w11 + 256) >> 9;
}

// The form is a compile-time policy of the one body.  LkPlain (mav_lk_track, _dev, _ex_dev) is the tracker as it always was.  LkErr
// takes cv2's `err` output and the flags at run time (LkTrackErrArgs), same launch shape and LDS:
//   OPTFLOW_USE_INITIAL_FLOW       the top level starts at out[p] * (1 / 2^level), read before anything is written (out is in and out)
//   OPTFLOW_LK_GET_MIN_EIGENVALS   err = minEig of every level that passes the first bounds test, written before the threshold test, so
//                                  level 0's stays; 0 when level 0 fails the first bounds test
//   err without that flag          a point still at status 1 after level 0's loop: q = out - halfWin, the bounds test on floor(q)
//                                  (failing it clears the status, err stays 0), then S = sum |J(q + k) - Iw[k]| over the window with
//                                  the iteration's own interpolation, Iw = level 0's plane still in LDS; err = (float)S / (float)(32 w h)
//                                  (a float32 division).  S is an exact integer <= 8160 x 33 x 33 < 2^24: no summation order in it.
// The iteration histogram does not count the error pass.
struct LkPlain { typedef LkTrackArgs Args; static constexpr bool ERR = false; };
struct LkErr { typedef LkTrackErrArgs Args; static constexpr bool ERR = true; };
template <typename Form>
__global__ __launch_bounds__(256) void k_lk_track(typename Form::Args a)
{
    extern __shared__ short lk_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = blockIdx.x * 4 + wv;
    int n = a.n;
    if (a.n_dev) { const int m = *a.n_dev; n = m < n ? m : n; }      // the count lives on the device: waves beyond it (all, if negative) leave
    if (p >= n) return;                                       // wave-uniform; the kernel has no barrier
    const int win_w = a.win_w, win_h = a.win_h, npix = win_w * win_h;
    short* Iw = lk_lds + (size_t)wv * 3 * npix;
    short* Dx = Iw + npix;
    short* Dy = Dx + npix;
    const float ptx = a.pts[2 * p], pty = a.pts[2 * p + 1];
    float gx = 0.f, gy = 0.f, errv = 0.f;                     // LkErr only: the initial position, the error output
    if constexpr (Form::ERR)
        if (a.flags & MAV_OPTFLOW_USE_INITIAL_FLOW) { gx = a.out[2 * p]; gy = a.out[2 * p + 1]; }
    const float halfx = (win_w - 1) * 0.5f, halfy = (win_h - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    float outx = 0.f, outy = 0.f;
    int status = 1;
    for (int level = a.lv.n - 1; level >= 0; level--) {
        const int w = a.lv.w[level], h = a.lv.h[level];
        const float sc = 1.f / (float)(1 << level);
        float px = ptx * sc, py = pty * sc, nx, ny;
        if (level == a.lv.n - 1) { nx = px; ny = py; } else { nx = outx * 2.f; ny = outy * 2.f; }
        if constexpr (Form::ERR)
            if (level == a.lv.n - 1 && (a.flags & MAV_OPTFLOW_USE_INITIAL_FLOW)) { nx = gx * sc; ny = gy * sc; }
        outx = nx; outy = ny;
        px -= halfx; py -= halfy;
        float fx = floorf(px), fy = floorf(py);
        if (!(fx >= (float)-win_w && fx < (float)w && fy >= (float)-win_h && fy < (float)h)) {
            if (level == 0) { status = 0; errv = 0.f; }
            continue;
        }
        const uint8_t* I = a.I + a.lv.off[level];
        const uint8_t* J = a.J + a.lv.off[level];
        const short2* D = a.D + a.lv.off[level];
        int ix = (int)fx, iy = (int)fy;
        LkWeights q = lk_weights(px - fx, py - fy);
        long long s11 = 0, s12 = 0, s22 = 0;
        for (int k = lane; k < npix; k += 64) {
            const int j = k / win_w, i = k - j * win_w, x = ix + i, y = iy + j;
            const int iv = lk_image_value(I, w, h, x, y, q);
            // the derivative is 0 outside the level (constant border), the image itself continues by REFLECT_101
            const bool xa = (unsigned)x < (unsigned)w, xb = (unsigned)(x + 1) < (unsigned)w;
            const bool ya = (unsigned)y < (unsigned)h, yb = (unsigned)(y + 1) < (unsigned)h;
            const short2 z = make_short2(0, 0);
            const short2 d00 = xa && ya ? D[(size_t)y * w + x] : z, d01 = xb && ya ? D[(size_t)y * w + x + 1] : z;
            const short2 d10 = xa && yb ? D[(size_t)(y + 1) * w + x] : z, d11 = xb && yb ? D[(size_t)(y + 1) * w + x + 1] : z;
            const int dx = ((int)d00.x * q.w00 + (int)d01.x * q.w01 + (int)d10.x * q.w10 + (int)d11.x * q.w11 + 8192) >> 14;
            const int dy = ((int)d00.y * q.w00 + (int)d01.y * q.w01 + (int)d10.y * q.w10 + (int)d11.y * q.w11 + 8192) >> 14;
            Iw[k] = (short)iv; Dx[k] = (short)dx; Dy[k] = (short)dy;
            s11 += (long long)(dx * dx); s12 += (long long)(dx * dy); s22 += (long long)(dy * dy);
        }
        s11 = wave_sum(s11); s12 = wave_sum(s12); s22 = wave_sum(s22);
        const float A11 = (float)(double)s11 * FLT_SCALE, A12 = (float)(double)s12 * FLT_SCALE, A22 = (float)(double)s22 * FLT_SCALE;
        float Dt = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win_w * win_h);
        if constexpr (Form::ERR)
            if (a.flags & MAV_OPTFLOW_LK_GET_MIN_EIGENVALS) errv = minEig;
        if (minEig < a.min_eig || Dt < FLT_EPSILON) {
            if (level == 0) status = 0;
            continue;
        }
        Dt = 1.f / Dt;
        nx -= halfx; ny -= halfy;
        float pdx = 0.f, pdy = 0.f;
        int j = 0;
        for (; j < a.max_count; j++) {
            fx = floorf(nx); fy = floorf(ny);
            if (!(fx >= (float)-win_w && fx < (float)w && fy >= (float)-win_h && fy < (float)h)) {
                if (level == 0) status = 0;
                break;
            }
            ix = (int)fx; iy = (int)fy;
            q = lk_weights(nx - fx, ny - fy);
            long long b1 = 0, b2 = 0;
            for (int k = lane; k < npix; k += 64) {
                const int jj = k / win_w, i = k - jj * win_w;
                const int diff = lk_image_value(J, w, h, ix + i, iy + jj, q) - (int)Iw[k];
                b1 += (long long)(diff * (int)Dx[k]); b2 += (long long)(diff * (int)Dy[k]);
            }
            b1 = wave_sum(b1); b2 = wave_sum(b2);
            const float fb1 = (float)(double)b1 * FLT_SCALE, fb2 = (float)(double)b2 * FLT_SCALE;
            const float dx = (A12 * fb2 - A22 * fb1) * Dt, dy = (A12 * fb1 - A11 * fb2) * Dt;
            nx += dx; ny += dy;
            outx = nx + halfx; outy = ny + halfy;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= a.eps2) { j++; break; }
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                j++;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (lane == 0 && a.iter_hist) atomicAdd(a.iter_hist + (j < MAV_LK_HIST - 1 ? j : MAV_LK_HIST - 1), 1u);
    }
    if constexpr (Form::ERR) {
        if (a.err && status && !(a.flags & MAV_OPTFLOW_LK_GET_MIN_EIGENVALS)) {
            const int w = a.lv.w[0], h = a.lv.h[0];
            const float qx = outx - halfx, qy = outy - halfy;
            const float fx = floorf(qx), fy = floorf(qy);
            if (!(fx >= (float)-win_w && fx < (float)w && fy >= (float)-win_h && fy < (float)h)) status = 0;
            else {
                const int ix = (int)fx, iy = (int)fy;
                const LkWeights q = lk_weights(qx - fx, qy - fy);
                const uint8_t* J = a.J + a.lv.off[0];
                long long S = 0;
                for (int k = lane; k < npix; k += 64) {
                    const int jj = k / win_w, i = k - jj * win_w;
                    const int diff = lk_image_value(J, w, h, ix + i, iy + jj, q) - (int)Iw[k];
                    S += (long long)(diff < 0 ? -diff : diff);
                }
                S = wave_sum(S);
                errv = (float)S / (float)(32 * win_w * win_h);
            }
        }
    }
    if (lane == 0) {
        a.out[2 * p] = outx; a.out[2 * p + 1] = outy;
        a.status[p] = (uint8_t)status;
        if constexpr (Form::ERR)
            if (a.err) a.err[p] = errv;
    }
}
size_t lk_track_lds_bytes(int win_w, int win_h) { return (size_t)4 * 3 * win_w * win_h * sizeof(short); }
void launch_lk_track(hipStream_t st, const LkTrackArgs& a)
{
    if (a.n < 1) return;
    hipLaunchKernelGGL(k_lk_track<LkPlain>, dim3((a.n + 3) / 4), dim3(256), lk_track_lds_bytes(a.win_w, a.win_h), st, a);
}
void launch_lk_track_err(hipStream_t st, const LkTrackErrArgs& a)
{
    if (a.n < 1) return;
    hipLaunchKernelGGL(k_lk_track<LkErr>, dim3((a.n + 3) / 4), dim3(256), lk_track_lds_bytes(a.win_w, a.win_h), st, a);
}

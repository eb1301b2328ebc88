// Connected components of u8 masks (any non-zero byte is set), 4- or 8-connectivity, batched: labels in raster order of each component's
// first pixel, per-component box / area / coordinate sums.  Integer arithmetic only.  DESIGN.md section 4e has the plan; in short:
//
//   L (int32 per pixel): -1 on background, otherwise the per-image linear index of another pixel of the same component with
//   L[i] <= i ("parent"); a pixel with L[i] == i is a root.  INVARIANT: L[i] <= i at every moment, and every store to a set pixel's word
//   only lowers it.  A root chase therefore strictly descends and ends after at most i steps whatever other threads do meanwhile; a
//   union lowers max(a, b) in every round (cc_union below) and ends likewise.  No thread ever waits for another thread's store; the
//   kernel boundaries are the only global synchronisation.  The root of a finished tree is the smallest index of its component, i.e.
//   the component's first pixel in raster order: every output is a function of the partition into components, not of scheduling.
//
//   1 k_cc_tile      one workgroup per MAV_CC_TILE_W x MAV_CC_TILE_H tile: union-find in LDS, L = image index of the tile-local root, A = 0
//   2 k_cc_merge     one thread per pixel on a tile's top row / left column: union with its neighbours across the border (agent-scope atomics)
//   3 k_cc_flatten   L[p] = root(p); A[root] += 1 per pixel (one atomic per distinct root of a wave)
//   4 k_cc_count     per chunk of 256 pixels: roots, and roots with area >= min_area
//   5 k_cc_scan      per image: exclusive scan of the chunk counts; counts[b] = the totals
//   6 k_cc_rank      roots: label = 1 + roots before it; slot = qualifying roots before it; A[root] = label, L[root] = slot code,
//                    the slot's record initialised
//   7 k_cc_stats     labels out; box and coordinate sums into slots < max_blobs (one set of atomics per distinct slot of a wave)
//   8 k_cc_finalize  x1 / y1 -> w / h
#include "mavflow_internal.h"

#define CC_THREADS 256
#define CC_NO_SLOT INT32_MIN      // L[root] after k_cc_rank: -(slot + 2), or this when the component has no record

static_assert(MAV_CC_TILE_W == 64, "a tile row is one wave: k_cc_tile takes a row's runs from one ballot");
static_assert(MAV_CC_TILE_W * MAV_CC_TILE_H <= 32767 && MAV_CC_TILE_H % (CC_THREADS / 64) == 0, "tile shape");
static_assert(sizeof(mav_blob) == 40 && sizeof(mav_cc_counts) == 8, "record layouts of include/mavflow.h");

// ---- union-find on a word array whose entries only decrease -----------------------------------------------------------------------
// LDS form (one workgroup's tile).  Every round either ends the loop or lowers max(a, b) (old < a when old != a, because lab[a] <= a):
// at most a + 1 rounds.  An entry that is not a root may be lowered too: the edge a -- old it held is replaced by a -- b and the pending
// union (old, b), which keeps a, old and b connected.
__device__ __forceinline__ int cc_find_lds(volatile int* lab, int v)
{
    int n;
    while ((n = lab[v]) != v) v = n;
    return v;
}
__device__ __forceinline__ void cc_union_lds(int* lab, int a, int b)
{
    a = cc_find_lds(lab, a);
    b = cc_find_lds(lab, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) break;
        a = old;
    }
}
// Global form.  In k_cc_merge workgroups on different XCDs read and write the same words: every access is an agent-scope atomic (a
// plain load may be served stale from the XCD's L2).  Relaxed order is enough: the values are indices, nothing is published behind them.
__device__ __forceinline__ int cc_load(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_find(const int* L, int v)
{
    int n;
    while ((n = cc_load(L, v)) != v) v = n;
    return v;
}
__device__ __forceinline__ void cc_union(int* L, int a, int b)
{
    a = cc_find(L, a);
    b = cc_find(L, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) break;
        a = old;
    }
}

// ---- 1: tile pass -----------------------------------------------------------------------------------------------------------------
// Wave w takes tile rows w, w + 4, ...; lane = column.  A row's horizontal runs come from the row's ballot (every pixel starts at its
// run's first pixel), so only the vertical and diagonal unions go through the loop.  Pixels outside the image are background.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_tile(const uint8_t* __restrict__ mask, int W, int H, int tiles_x, int* __restrict__ L,
                                                        int* __restrict__ A)
{
    __shared__ int lab[MAV_CC_TILE_W * MAV_CC_TILE_H];
    __shared__ unsigned long long rowm[MAV_CC_TILE_H];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * MAV_CC_TILE_W, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * MAV_CC_TILE_H;
    const size_t img = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const int x = x0 + lane;
    for (int r = wave; r < MAV_CC_TILE_H; r += CC_THREADS / 64) {
        const int y = y0 + r;
        const bool set = x < W && y < H && mask[img + (size_t)y * W + x] != 0;
        const unsigned long long m = __ballot(set);
        if (lane == 0) rowm[r] = m;
        const unsigned long long z = ~m & ((1ull << lane) - 1);           // unset columns left of this one
        const int start = z ? 64 - __clzll((long long)z) : 0;             // first column of this pixel's run
        lab[r * MAV_CC_TILE_W + lane] = set ? r * MAV_CC_TILE_W + start : -1;
    }
    __syncthreads();
    for (int r = wave ? wave : CC_THREADS / 64; r < MAV_CC_TILE_H; r += CC_THREADS / 64) {
        const unsigned long long m = rowm[r], up = rowm[r - 1];
        if (!((m >> lane) & 1)) continue;
        const int i = r * MAV_CC_TILE_W + lane;
        if ((up >> lane) & 1) cc_union_lds(lab, i, i - MAV_CC_TILE_W);
        else if (CONN == 8) {                // a diagonal neighbour next to a set `up` is joined through `up`
            if (lane > 0 && ((up >> (lane - 1)) & 1)) cc_union_lds(lab, i, i - MAV_CC_TILE_W - 1);
            if (lane < 63 && ((up >> (lane + 1)) & 1)) cc_union_lds(lab, i, i - MAV_CC_TILE_W + 1);
        }
    }
    __syncthreads();
    for (int r = wave; r < MAV_CC_TILE_H; r += CC_THREADS / 64) {
        const int y = y0 + r;
        if (x >= W || y >= H) continue;
        int v = lab[r * MAV_CC_TILE_W + lane];
        if (v >= 0) {
            v = cc_find_lds(lab, v);
            v = (y0 + v / MAV_CC_TILE_W) * W + x0 + v % MAV_CC_TILE_W;     // raster order inside the tile and in the image agree
        }
        const size_t p = img + (size_t)y * W + x;
        L[p] = v;
        A[p] = 0;
    }
}

// ---- 2: border merge --------------------------------------------------------------------------------------------------------------
// Threads [0, nh): pixel x of the k-th horizontal border (y = (k + 1) * TILE_H): up and, for 8-connectivity, the two upper diagonals.
// Threads [nh, nh + nv): pixel y of the k-th vertical border (x = (k + 1) * TILE_W): left and the two left diagonals.  Diagonals across
// a tile corner are among them.  A diagonal next to a set straight neighbour is skipped: it is joined through that neighbour, by the
// tile pass or by the other border's thread.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_merge(int W, int H, int nh, int nv, int* L_all)
{
    const int t = (int)(blockIdx.x * CC_THREADS + threadIdx.x);
    if (t >= nh + nv) return;
    int* L = L_all + (size_t)blockIdx.y * (size_t)W * (size_t)H;
    int x, y, dx, dy;                       // the pixel, and the step to its straight neighbour across the border
    if (t < nh) { x = t % W; y = (t / W + 1) * MAV_CC_TILE_H; dx = 0; dy = -1; }
    else { const int u = t - nh; y = u % H; x = (u / H + 1) * MAV_CC_TILE_W; dx = -1; dy = 0; }
    const int p = y * W + x;
    if (cc_load(L, p) < 0) return;
    const int q = (y + dy) * W + x + dx;
    if (cc_load(L, q) >= 0) { cc_union(L, p, q); return; }
    if (CONN != 8) return;
    for (int s = -1; s <= 1; s += 2) {      // the two diagonals: along the border on either side of q
        const int qx = x + dx + (dx ? 0 : s), qy = y + dy + (dy ? 0 : s);
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const int d = qy * W + qx;
        if (cc_load(L, d) >= 0) cc_union(L, p, d);
    }
}

// ---- 3: flatten + area ------------------------------------------------------------------------------------------------------------
// The roots are settled (kernel boundary).  Other threads' L[p] = root stores race with the chases only in the harmless way: any
// value a word has held is an ancestor <= its index.  Area: one atomic per distinct root among a wave's lanes -- inside a blob that is
// one per wave; each round retires at least the leader's lane.
__global__ __launch_bounds__(CC_THREADS) void k_cc_flatten(int n, int* L_all, int* A_all)
{
    const int p = (int)(blockIdx.x * CC_THREADS + threadIdx.x);
    const size_t img = (size_t)blockIdx.y * (size_t)n;
    int* L = L_all + img;
    int* A = A_all + img;
    int root = -1;
    if (p < n) {
        const int v = cc_load(L, p);
        if (v >= 0) {
            root = cc_find(L, v);
            if (root != v) __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long active = __ballot(root >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int r = __shfl(root, leader);
        const unsigned long long m = __ballot(root == r);
        if (lane == leader) atomicAdd(&A[r], __popcll(m));
        active &= ~m;
    }
}

// ---- 4 - 6: rank ------------------------------------------------------------------------------------------------------------------
// cnt: [image][chunk][2] = roots, roots with area >= min_area, of the chunk's 256 pixels; after the scan: of all chunks before it.
__device__ __forceinline__ void cc_flags(const int* L, const int* A, int p, int n, int min_area, bool* root, bool* big)
{
    *root = p < n && L[p] == p;
    *big = *root && A[p] >= min_area;
}
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(int n, int nchunks, int min_area, const int* __restrict__ L_all, const int* __restrict__ A_all,
                                                         int* __restrict__ cnt)
{
    __shared__ int part[CC_THREADS / 64][2];
    const int p = (int)(blockIdx.x * CC_THREADS + threadIdx.x);
    const size_t img = (size_t)blockIdx.y * (size_t)n;
    bool root, big;
    cc_flags(L_all + img, A_all + img, p, n, min_area, &root, &big);
    const unsigned long long mr = __ballot(root), mb = __ballot(big);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = __popcll(mr); part[threadIdx.x >> 6][1] = __popcll(mb); }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
        for (int w = 0; w < CC_THREADS / 64; w++) s += part[w][threadIdx.x];
        cnt[((size_t)blockIdx.y * nchunks + blockIdx.x) * 2 + threadIdx.x] = s;
    }
}
// one workgroup per image: thread t owns chunks [t * per, (t + 1) * per)
__global__ __launch_bounds__(CC_THREADS) void k_cc_scan(int nchunks, int* __restrict__ cnt_all, mav_cc_counts* __restrict__ counts)
{
    __shared__ int tot[CC_THREADS][2];
    int* cnt = cnt_all + (size_t)blockIdx.x * nchunks * 2;
    const int per = (nchunks + CC_THREADS - 1) / CC_THREADS, c0 = (int)threadIdx.x * per, c1 = min(c0 + per, nchunks);
    int s0 = 0, s1 = 0;
    for (int c = c0; c < c1; c++) { s0 += cnt[2 * c]; s1 += cnt[2 * c + 1]; }
    tot[threadIdx.x][0] = s0; tot[threadIdx.x][1] = s1;
    __syncthreads();
    if (threadIdx.x < 2) {                   // 256 partial sums: a serial exclusive scan per column
        int run = 0;
        for (int t = 0; t < CC_THREADS; t++) { const int v = tot[t][threadIdx.x]; tot[t][threadIdx.x] = run; run += v; }
        if (threadIdx.x == 0) counts[blockIdx.x].n_components = run; else counts[blockIdx.x].n_blobs = run;
    }
    __syncthreads();
    s0 = tot[threadIdx.x][0]; s1 = tot[threadIdx.x][1];
    for (int c = c0; c < c1; c++) {
        const int v0 = cnt[2 * c], v1 = cnt[2 * c + 1];
        cnt[2 * c] = s0; cnt[2 * c + 1] = s1;
        s0 += v0; s1 += v1;
    }
}
__global__ __launch_bounds__(CC_THREADS) void k_cc_rank(int n, int W, int nchunks, int min_area, int max_blobs, int* __restrict__ L_all,
                                                        int* __restrict__ A_all, const int* __restrict__ cnt, mav_blob* __restrict__ blobs)
{
    __shared__ int part[CC_THREADS / 64][2];
    const int p = (int)(blockIdx.x * CC_THREADS + threadIdx.x), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)blockIdx.y * (size_t)n;
    int* L = L_all + img;
    int* A = A_all + img;
    bool root, big;
    cc_flags(L, A, p, n, min_area, &root, &big);
    const unsigned long long mr = __ballot(root), mb = __ballot(big), below = (1ull << lane) - 1;
    if (lane == 0) { part[wave][0] = __popcll(mr); part[wave][1] = __popcll(mb); }
    __syncthreads();
    if (!root) return;
    const int* base = cnt + ((size_t)blockIdx.y * nchunks + blockIdx.x) * 2;
    int label = base[0] + __popcll(mr & below) + 1, slot = base[1] + __popcll(mb & below);
    for (int w = 0; w < wave; w++) { label += part[w][0]; slot += part[w][1]; }
    const int area = A[p];
    A[p] = label;
    if (big && slot < max_blobs) {
        L[p] = -(slot + 2);
        mav_blob rec;
        rec.label = label; rec.x = p % W; rec.y = p / W; rec.w = rec.x; rec.h = rec.y; rec.area = area;   // w, h hold x1, y1 until k_cc_finalize
        rec.sum_x = 0; rec.sum_y = 0;
        blobs[(size_t)blockIdx.y * max_blobs + slot] = rec;
    } else L[p] = CC_NO_SLOT;
}

// ---- 7: labels out + statistics ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_wave_min(int v) { for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d)); return v; }
__device__ __forceinline__ int cc_wave_max(int v) { for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d)); return v; }
__device__ __forceinline__ unsigned long long cc_wave_sum(unsigned long long v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d); return v; }
__global__ __launch_bounds__(CC_THREADS) void k_cc_stats(int n, int W, int max_blobs, const int* __restrict__ L_all, const int* __restrict__ A_all,
                                                         int* __restrict__ labels, mav_blob* __restrict__ blobs_all)
{
    const int p = (int)(blockIdx.x * CC_THREADS + threadIdx.x), lane = threadIdx.x & 63;
    const size_t img = (size_t)blockIdx.y * (size_t)n;
    const int* L = L_all + img;
    const int* A = A_all + img;
    int slot = -1, x = 0, y = 0;
    if (p < n) {
        int v = L[p], label = 0;
        if (v != -1) {
            const int r = v >= 0 ? v : p;      // a root's own word already holds its slot code
            if (v >= 0) v = L[r];
            label = A[r];
            if (v != CC_NO_SLOT) slot = -v - 2;
            x = p % W; y = p / W;
        }
        if (labels) labels[img + p] = label;
    }
    mav_blob* blobs = blobs_all + (size_t)blockIdx.y * max_blobs;
    // one set of atomics per distinct slot among the wave's lanes (inside a blob: one per wave); each round retires the leader's lanes
    unsigned long long active = __ballot(slot >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int s = __shfl(slot, leader);
        const bool mine = slot == s;
        const unsigned long long m = __ballot(mine);
        const int x0 = cc_wave_min(mine ? x : INT32_MAX), x1 = cc_wave_max(mine ? x : -1), y1 = cc_wave_max(mine ? y : -1);
        const unsigned long long sx = cc_wave_sum(mine ? (unsigned long long)x : 0ull), sy = cc_wave_sum(mine ? (unsigned long long)y : 0ull);
        if (lane == leader) {
            mav_blob* b = blobs + s;            // y0 is the root's row: set by k_cc_rank
            atomicMin(&b->x, x0);
            atomicMax(&b->w, x1);
            atomicMax(&b->h, y1);
            atomicAdd((unsigned long long*)&b->sum_x, sx);
            atomicAdd((unsigned long long*)&b->sum_y, sy);
        }
        active &= ~m;
    }
}
__global__ __launch_bounds__(CC_THREADS) void k_cc_finalize(int max_blobs, const mav_cc_counts* __restrict__ counts, mav_blob* __restrict__ blobs)
{
    const int s = (int)(blockIdx.x * CC_THREADS + threadIdx.x);
    if (s >= max_blobs || s >= counts[blockIdx.y].n_blobs) return;
    mav_blob* b = blobs + (size_t)blockIdx.y * max_blobs + s;
    b->w = b->w - b->x + 1;
    b->h = b->h - b->y + 1;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
size_t cc_workspace_per_image(int W, int H)
{
    const size_t n = (size_t)W * H, nchunks = (n + CC_THREADS - 1) / CC_THREADS;
    return ((n * 2 * sizeof(int) + nchunks * 2 * sizeof(int)) + 255) & ~(size_t)255;
}
void launch_components(hipStream_t st, const CcArgs& a)
{
    const int W = a.W, H = a.H, B = a.B, n = W * H;
    const int tiles_x = (W + MAV_CC_TILE_W - 1) / MAV_CC_TILE_W, tiles_y = (H + MAV_CC_TILE_H - 1) / MAV_CC_TILE_H;
    const int nchunks = (n + CC_THREADS - 1) / CC_THREADS;
    const int nh = (tiles_y - 1) * W, nv = (tiles_x - 1) * H;
    int* L = (int*)a.ws;
    int* A = L + (size_t)B * n;
    int* cnt = A + (size_t)B * n;
    const dim3 px(nchunks, B), th(CC_THREADS);
    if (a.connectivity == 8) hipLaunchKernelGGL(k_cc_tile<8>, dim3(tiles_x * tiles_y, B), th, 0, st, a.mask, W, H, tiles_x, L, A);
    else hipLaunchKernelGGL(k_cc_tile<4>, dim3(tiles_x * tiles_y, B), th, 0, st, a.mask, W, H, tiles_x, L, A);
    if (nh + nv > 0) {
        const dim3 g((nh + nv + CC_THREADS - 1) / CC_THREADS, B);
        if (a.connectivity == 8) hipLaunchKernelGGL(k_cc_merge<8>, g, th, 0, st, W, H, nh, nv, L);
        else hipLaunchKernelGGL(k_cc_merge<4>, g, th, 0, st, W, H, nh, nv, L);
    }
    hipLaunchKernelGGL(k_cc_flatten, px, th, 0, st, n, L, A);
    hipLaunchKernelGGL(k_cc_count, px, th, 0, st, n, nchunks, a.min_area, L, A, cnt);
    hipLaunchKernelGGL(k_cc_scan, dim3(B), th, 0, st, nchunks, cnt, a.counts);
    hipLaunchKernelGGL(k_cc_rank, px, th, 0, st, n, W, nchunks, a.min_area, a.max_blobs, L, A, cnt, a.blobs);
    hipLaunchKernelGGL(k_cc_stats, px, th, 0, st, n, W, a.max_blobs, L, A, a.labels, a.blobs);
    hipLaunchKernelGGL(k_cc_finalize, dim3((a.max_blobs + CC_THREADS - 1) / CC_THREADS, B), th, 0, st, a.max_blobs, a.counts, a.blobs);
}

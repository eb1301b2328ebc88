// k-means clustering on the device (include/mavflow_cluster.h has the algorithm and the order of its sums; tests/kmeans_ref.py restates
// both).  Compiled with -ffp-contract=off: a distance is D subtractions, D products and D - 1 additions in float32, each rounded on its own.
// One call is a fixed sequence of launches on the context's stream; what the data decides (which attempts are done, which clusters are
// empty, the donor, the best attempt) is in the image's KmState, and a launch with nothing to do for its image leaves at once.  All
// attempts of an image advance in the same launches.
//   k_km_init     the control block from the caller's centres
//   k_km_assign   the hot pass: a chunk's samples in registers, labelled against every live attempt's centres (LDS); u8 labels; per-cluster
//                 partial sums per lane -> wave -> workgroup, written to the slab [chunk][attempt][cluster][component + count]
//   k_km_sums     one workgroup per image: the slab added in chunk order; the first empty cluster and its donor chosen
//   k_km_far      (guarded, K - 1 rounds) the donor's farthest sample: integer maximum of dist bits << 32 | index
//   k_km_move     (guarded) one thread per attempt moves that sample and chooses the next empty cluster
//   k_km_update   new centres, shift, done flags
//   k_km_dist     compactness partials, the same slab scheme;  k_km_finish  their sum, the best attempt, centres and record;
//   k_km_labels   the best attempt's labels widened to int32
// The pass is arithmetic-bound (A * K distances per sample read once), not a stream.
#include "mavflow_internal.h"
#include "../../include/mavflow_cluster.h"

static_assert(KM_THREADS * KM_PER_THREAD == MAV_KMEANS_CHUNK, "chunk");

struct KmDims { int n, A, K, D; size_t image_bytes, labels_off, slab_off; };
__device__ __forceinline__ KmState* km_state(char* ws, const KmDims& g, int b) { return (KmState*)(ws + g.image_bytes * b); }
__device__ __forceinline__ uint8_t* km_lbl(char* ws, const KmDims& g, int b) { return (uint8_t*)(ws + g.image_bytes * b + g.labels_off); }
__device__ __forceinline__ double* km_slab(char* ws, const KmDims& g, int b) { return (double*)(ws + g.image_bytes * b + g.slab_off); }

template <int D> __device__ __forceinline__ float km_dist(const float* x, const float* c)
{
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; d++) { const float t = x[d] - c[d]; s = s + t * t; }
    return s;
}
__device__ __forceinline__ double km_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// The first empty cluster of attempt a and the cluster that gives it a sample; pending = -1 when none is empty.
__device__ void km_decide(KmState* st, int a, int K, int D)
{
    int empty = -1;
    for (int k = 0; k < K; k++) if (st->n[a][k] == 0) { empty = k; break; }
    st->pending[a] = empty;
    if (empty < 0) return;
    int dn = 0;
    for (int k = 1; k < K; k++) if (st->n[a][dn] < st->n[a][k]) dn = k;
    st->donor[a] = dn;
    for (int d = 0; d < D; d++) st->mean[a][d] = (float)(st->S[a][dn][d] / (double)st->n[a][dn]);
    st->key[a] = 0ull;
}

__global__ __launch_bounds__(KM_THREADS) void k_km_init(const float* __restrict__ init, KmDims g, char* ws)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    KmState* st = km_state(ws, g, b);
    unsigned* w = (unsigned*)st;
    for (unsigned i = tid; i < sizeof(KmState) / 4; i += KM_THREADS) w[i] = 0u;
    __syncthreads();
    const int E = g.A * g.K * g.D;
    for (int e = tid; e < E; e += KM_THREADS) {
        const int a = e / (g.K * g.D), r = e - a * g.K * g.D, k = r / g.D, d = r - k * g.D;
        st->c[a][k][d] = init[(size_t)b * E + e];
    }
    if (tid < 16) st->pending[tid] = -1;
    if (tid == 0) st->live = g.A;
}

template <int D, typename T>
__global__ __launch_bounds__(KM_THREADS) void k_km_assign(const T* __restrict__ samples, KmDims g, char* ws)
{
    __shared__ float s_c[16 * 16 * D];
    __shared__ int s_done[16];
    __shared__ double s_part[4][16][D + 1];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    KmState* st = km_state(ws, g, b);
    if (st->live == 0) {                                             // (uniform over the launch's workgroups of this image)
        if (blockIdx.x == 0 && tid == 0) st->skipped++;
        return;
    }
    const int A = g.A, K = g.K, n = g.n;
    for (int e = tid; e < A * K * D; e += KM_THREADS) {
        const int a = e / (K * D), r = e - a * K * D, k = r / D, d = r - k * D;
        s_c[e] = st->c[a][k][d];
    }
    if (tid < 16) s_done[tid] = tid < A ? st->done[tid] : 1;
    __syncthreads();
    const T* xs = samples + (size_t)b * n * D;
    uint8_t* lbl = km_lbl(ws, g, b);
    double* slab = km_slab(ws, g, b);
    const size_t chunks = ((size_t)n + MAV_KMEANS_CHUNK - 1) / MAV_KMEANS_CHUNK;
    const int E = K * (D + 1);
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        float x[KM_PER_THREAD][D];
        const size_t i0 = chunk * MAV_KMEANS_CHUNK + tid;
#pragma unroll
        for (int j = 0; j < KM_PER_THREAD; j++) {
            const size_t i = i0 + (size_t)j * KM_THREADS;
#pragma unroll
            for (int d = 0; d < D; d++) x[j][d] = i < (size_t)n ? (float)xs[i * D + d] : 0.f;
        }
        for (int a = 0; a < A; a++) {
            if (s_done[a]) continue;                                 // (uniform: every thread reaches the barriers below)
            const float* ca = s_c + a * K * D;
            float bd[KM_PER_THREAD];
            int lab[KM_PER_THREAD];
#pragma unroll
            for (int j = 0; j < KM_PER_THREAD; j++) { bd[j] = km_dist<D>(x[j], ca); lab[j] = 0; }
            for (int k = 1; k < K; k++) {
                float ck[D];
#pragma unroll
                for (int d = 0; d < D; d++) ck[d] = ca[k * D + d];
#pragma unroll
                for (int j = 0; j < KM_PER_THREAD; j++) {
                    const float dk = km_dist<D>(x[j], ck);
                    if (dk < bd[j]) { bd[j] = dk; lab[j] = k; }      // strict: the first minimum stays
                }
            }
#pragma unroll
            for (int j = 0; j < KM_PER_THREAD; j++) {
                const size_t i = i0 + (size_t)j * KM_THREADS;
                if (i < (size_t)n) lbl[(size_t)a * n + i] = (uint8_t)lab[j]; else lab[j] = -1;
            }
            for (int k = 0; k < K; k++) {
                double v[D];
                int cn = 0;
#pragma unroll
                for (int d = 0; d < D; d++) v[d] = 0.0;
#pragma unroll
                for (int j = 0; j < KM_PER_THREAD; j++) {
                    const bool m = lab[j] == k;
                    cn += m;
#pragma unroll
                    for (int d = 0; d < D; d++) v[d] = v[d] + (m ? (double)x[j][d] : 0.0);
                }
#pragma unroll
                for (int d = 0; d < D; d++) v[d] = km_wave_sum(v[d]);
                for (int o = 32; o > 0; o >>= 1) cn += __shfl_xor(cn, o);
                if (lane == 0) {
#pragma unroll
                    for (int d = 0; d < D; d++) s_part[wv][k][d] = v[d];
                    s_part[wv][k][D] = (double)cn;
                }
            }
            __syncthreads();
            if (tid < E) {
                const int k = tid / (D + 1), d = tid - k * (D + 1);
                slab[(chunk * A + a) * E + tid] = ((s_part[0][k][d] + s_part[1][k][d]) + s_part[2][k][d]) + s_part[3][k][d];
            }
            __syncthreads();
        }
    }
}

// One workgroup per image: S and n of every live attempt from the slab, chunk by chunk; then the first repair decision.
__global__ __launch_bounds__(KM_THREADS) void k_km_sums(KmDims g, char* ws)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    KmState* st = km_state(ws, g, b);
    if (st->live == 0) {
        if (tid == 0) st->skipped++;
        return;
    }
    const int A = g.A, K = g.K, D = g.D, E = K * (D + 1);
    const double* slab = km_slab(ws, g, b);
    const size_t chunks = ((size_t)g.n + MAV_KMEANS_CHUNK - 1) / MAV_KMEANS_CHUNK;
    for (int e = tid; e < A * E; e += KM_THREADS) {
        const int a = e / E, r = e - a * E, k = r / (D + 1), d = r - k * (D + 1);
        if (st->done[a]) continue;
        double s = 0.0;
        for (size_t c = 0; c < chunks; c++) s = s + slab[c * A * E + e];
        if (d == D) st->n[a][k] = (int)s; else st->S[a][k][d] = s;
    }
    __syncthreads();
    if (tid < A && !st->done[tid]) { st->iters[tid]++; km_decide(st, tid, K, D); }
    __syncthreads();
    if (tid == 0) {
        int any = 0;
        for (int a = 0; a < A; a++) any |= st->pending[a] >= 0;
        st->any_pending = any;
    }
}

template <int D, typename T>
__global__ __launch_bounds__(KM_THREADS) void k_km_far(const T* __restrict__ samples, KmDims g, char* ws)
{
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    KmState* st = km_state(ws, g, b);
    if (st->any_pending == 0) {
        if (blockIdx.x == 0 && tid == 0) st->skipped++;
        return;
    }
    const int n = g.n;
    const T* xs = samples + (size_t)b * n * D;
    const uint8_t* lbl = km_lbl(ws, g, b);
    for (int a = 0; a < g.A; a++) {
        if (st->pending[a] < 0) continue;                             // (uniform)
        const int dn = st->donor[a];
        float m[D];
#pragma unroll
        for (int d = 0; d < D; d++) m[d] = st->mean[a][d];
        unsigned long long best = 0ull;
        bool has = false;
        for (size_t i = (size_t)blockIdx.x * KM_THREADS + tid; i < (size_t)n; i += (size_t)gridDim.x * KM_THREADS) {
            if (lbl[(size_t)a * n + i] != dn) continue;
            float x[D];
#pragma unroll
            for (int d = 0; d < D; d++) x[d] = (float)xs[i * D + d];
            const unsigned long long key = ((unsigned long long)__float_as_uint(km_dist<D>(x, m)) << 32) | (unsigned long long)i;
            if (!has || key > best) best = key;
            has = true;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            const int oh = __shfl_xor((int)has, o);
            if (oh && (!has || other > best)) best = other;
            has = has || oh;
        }
        if (lane == 0 && has) atomicMax(&st->key[a], best);
    }
}

template <typename T>
__global__ __launch_bounds__(64) void k_km_move(const T* __restrict__ samples, KmDims g, char* ws)
{
    const int b = blockIdx.x, a = threadIdx.x;
    KmState* st = km_state(ws, g, b);
    if (st->any_pending == 0) {
        if (a == 0) st->skipped++;
        return;
    }
    const int n = g.n, D = g.D;
    if (a < g.A && st->pending[a] >= 0) {
        const int k = st->pending[a], dn = st->donor[a];
        const size_t j = (size_t)(st->key[a] & 0xFFFFFFFFull);
        const T* x = samples + ((size_t)b * n + j) * D;
        km_lbl(ws, g, b)[(size_t)a * n + j] = (uint8_t)k;
        st->n[a][dn]--; st->n[a][k]++;
        for (int d = 0; d < D; d++) {
            const double v = (double)(float)x[d];
            st->S[a][dn][d] = st->S[a][dn][d] - v;
            st->S[a][k][d] = st->S[a][k][d] + v;
        }
        st->repairs[a]++;
        km_decide(st, a, g.K, D);
    }
    __syncthreads();
    if (a == 0) {
        int any = 0;
        for (int q = 0; q < g.A; q++) any |= st->pending[q] >= 0;
        st->any_pending = any;
    }
}

__global__ __launch_bounds__(64) void k_km_update(KmDims g, char* ws, int last, double eps2)
{
    const int b = blockIdx.x, a = threadIdx.x;
    KmState* st = km_state(ws, g, b);
    if (st->live == 0) {
        if (a == 0) st->skipped++;
        return;
    }
    if (a < g.A && !st->done[a]) {
        double shift = 0.0;
        for (int k = 0; k < g.K; k++) {
            double s = 0.0;
            for (int d = 0; d < g.D; d++) {
                const float nw = (float)(st->S[a][k][d] / (double)st->n[a][k]);
                const double t = (double)(nw - st->c[a][k][d]);
                s = s + t * t;
                st->c[a][k][d] = nw;
            }
            shift = s > shift ? s : shift;
        }
        st->shift[a] = shift;
        if (last || shift <= eps2) st->done[a] = 1;
    }
    __syncthreads();
    if (a == 0) {
        int live = 0;
        for (int q = 0; q < g.A; q++) live += !st->done[q];
        st->live = live;
    }
}

template <int D, typename T>
__global__ __launch_bounds__(KM_THREADS) void k_km_dist(const T* __restrict__ samples, KmDims g, char* ws)
{
    __shared__ float s_c[16 * 16 * D];
    __shared__ double s_part[4][16];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    KmState* st = km_state(ws, g, b);
    const int A = g.A, K = g.K, n = g.n;
    for (int e = tid; e < A * K * D; e += KM_THREADS) {
        const int a = e / (K * D), r = e - a * K * D, k = r / D, d = r - k * D;
        s_c[e] = st->c[a][k][d];
    }
    __syncthreads();
    const T* xs = samples + (size_t)b * n * D;
    const uint8_t* lbl = km_lbl(ws, g, b);
    double* slab = km_slab(ws, g, b);
    const size_t chunks = ((size_t)n + MAV_KMEANS_CHUNK - 1) / MAV_KMEANS_CHUNK;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        float x[KM_PER_THREAD][D];
        const size_t i0 = chunk * MAV_KMEANS_CHUNK + tid;
#pragma unroll
        for (int j = 0; j < KM_PER_THREAD; j++) {
            const size_t i = i0 + (size_t)j * KM_THREADS;
#pragma unroll
            for (int d = 0; d < D; d++) x[j][d] = i < (size_t)n ? (float)xs[i * D + d] : 0.f;
        }
        for (int a = 0; a < A; a++) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < KM_PER_THREAD; j++) {
                const size_t i = i0 + (size_t)j * KM_THREADS;
                if (i < (size_t)n) v = v + (double)km_dist<D>(x[j], s_c + (a * K + (lbl[(size_t)a * n + i] & 15)) * D);
            }
            v = km_wave_sum(v);
            if (lane == 0) s_part[wv][a] = v;
        }
        __syncthreads();
        if (tid < A) slab[chunk * A + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_km_finish(KmDims g, char* ws, float* __restrict__ centers, mav_kmeans_record* __restrict__ records)
{
    const int b = blockIdx.x, a = threadIdx.x;
    KmState* st = km_state(ws, g, b);
    const double* slab = km_slab(ws, g, b);
    const size_t chunks = ((size_t)g.n + MAV_KMEANS_CHUNK - 1) / MAV_KMEANS_CHUNK;
    if (a < g.A) {
        double s = 0.0;
        for (size_t c = 0; c < chunks; c++) s = s + slab[c * g.A + a];
        st->compact[a] = s;
    }
    __syncthreads();
    if (a == 0) {
        int best = 0, repairs = 0;
        for (int q = 1; q < g.A; q++) if (st->compact[q] < st->compact[best]) best = q;     // strict: the first smallest stays
        for (int q = 0; q < g.A; q++) repairs += st->repairs[q];
        st->best = best;
        mav_kmeans_record r;
        r.compactness = st->compact[best];
        r.shift = st->shift[best];
        r.best_attempt = best;
        r.iterations = st->iters[best];
        r.repairs = repairs;
        r.skipped = st->skipped;
        for (int k = 0; k < 16; k++) r.counts[k] = k < g.K ? st->n[best][k] : 0;
        records[b] = r;
        for (int k = 0; k < g.K; k++)
            for (int d = 0; d < g.D; d++) centers[((size_t)b * g.K + k) * g.D + d] = st->c[best][k][d];
    }
}

__global__ __launch_bounds__(KM_THREADS) void k_km_labels(KmDims g, char* ws, int32_t* __restrict__ labels)
{
    const int b = blockIdx.z;
    const KmState* st = km_state(ws, g, b);
    const uint8_t* lbl = km_lbl(ws, g, b) + (size_t)st->best * g.n;
    int32_t* out = labels + (size_t)b * g.n;
    for (size_t i = (size_t)blockIdx.x * KM_THREADS + threadIdx.x; i < (size_t)g.n; i += (size_t)gridDim.x * KM_THREADS) out[i] = (int32_t)lbl[i];
}

template <int D, typename T> static void km_run(hipStream_t st, const KmCall& k, const KmDims& g)
{
    const T* xs = (const T*)k.samples;
    const size_t chunks = km_chunks(k.n), blocks = ((size_t)k.n + KM_THREADS - 1) / KM_THREADS;
    const dim3 by_chunk((unsigned)(chunks < KM_GRID_CAP ? chunks : KM_GRID_CAP), 1, k.B), by_sample((unsigned)(blocks < KM_GRID_CAP ? blocks : KM_GRID_CAP), 1, k.B);
    hipLaunchKernelGGL(k_km_init, dim3(k.B), dim3(KM_THREADS), 0, st, k.init, g, k.ws);
    for (int it = 1; it < k.max_iter; it++) {
        hipLaunchKernelGGL((k_km_assign<D, T>), by_chunk, dim3(KM_THREADS), 0, st, xs, g, k.ws);
        hipLaunchKernelGGL(k_km_sums, dim3(k.B), dim3(KM_THREADS), 0, st, g, k.ws);
        for (int r = 1; r < k.K; r++) {
            hipLaunchKernelGGL((k_km_far<D, T>), by_sample, dim3(KM_THREADS), 0, st, xs, g, k.ws);
            hipLaunchKernelGGL((k_km_move<T>), dim3(k.B), dim3(64), 0, st, xs, g, k.ws);
        }
        hipLaunchKernelGGL(k_km_update, dim3(k.B), dim3(64), 0, st, g, k.ws, it == k.max_iter - 1 ? 1 : 0, k.eps2);
    }
    hipLaunchKernelGGL((k_km_dist<D, T>), by_chunk, dim3(KM_THREADS), 0, st, xs, g, k.ws);
    hipLaunchKernelGGL(k_km_finish, dim3(k.B), dim3(64), 0, st, g, k.ws, k.centers, (mav_kmeans_record*)k.records);
    hipLaunchKernelGGL(k_km_labels, by_sample, dim3(KM_THREADS), 0, st, g, k.ws, k.labels);
}
template <typename T> static void km_run_dims(hipStream_t st, const KmCall& k, const KmDims& g)
{
    switch (k.D) {
    case 1: km_run<1, T>(st, k, g); break;
    case 2: km_run<2, T>(st, k, g); break;
    case 3: km_run<3, T>(st, k, g); break;
    case 4: km_run<4, T>(st, k, g); break;
    }
}
void launch_kmeans(hipStream_t st, const KmCall& k)
{
    KmDims g;
    g.n = k.n; g.A = k.A; g.K = k.K; g.D = k.D;
    g.image_bytes = km_image_bytes(k.n, k.A, k.K, k.D);
    g.labels_off = km_state_bytes();
    g.slab_off = km_state_bytes() + km_labels_bytes(k.n, k.A);
    if (k.u8) km_run_dims<uint8_t>(st, k, g); else km_run_dims<float>(st, k, g);
}

// Detector.clustering after the cv2 call: the table from the device centres, then one byte per sample component.
__global__ __launch_bounds__(KM_THREADS) void k_km_paint(const int32_t* __restrict__ labels, const float* __restrict__ centers, int n, int K, int D,
                                                         uint8_t* __restrict__ res, uint8_t* __restrict__ mask)
{
    __shared__ uint8_t s_lut[16 * 4];
    const int b = blockIdx.z, tid = threadIdx.x;
    const float* c = centers + (size_t)b * K * D;
    if (tid < 64) {
        float mx = c[0];
        for (int e = 1; e < K * D; e++) mx = c[e] > mx ? c[e] : mx;
        if (mx == 0.f) mx = 1.f;
        uint8_t v = 0;
        if (tid < K * D) {
            const float p = c[tid] * 255.f, q = p / mx;
            v = (uint8_t)(int)q;
        }
        s_lut[tid] = v;
    }
    __syncthreads();
    const int32_t* lb = labels + (size_t)b * n;
    uint8_t* out = res + (size_t)b * n * D;
    for (size_t i = (size_t)blockIdx.x * KM_THREADS + tid; i < (size_t)n; i += (size_t)gridDim.x * KM_THREADS) {
        const int l = lb[i] & 15;
        for (int d = 0; d < D; d++) out[i * D + d] = s_lut[l * D + d];
        if (mask) mask[(size_t)b * n + i] = s_lut[l * D] >= 225 ? 1 : 0;
    }
}
void launch_kmeans_paint(hipStream_t st, const int32_t* labels, const float* centers, int n, int B, int K, int D, uint8_t* res, uint8_t* mask)
{
    const size_t blocks = ((size_t)n + KM_THREADS - 1) / KM_THREADS;
    hipLaunchKernelGGL(k_km_paint, dim3((unsigned)(blocks < KM_GRID_CAP ? blocks : KM_GRID_CAP), 1, B), dim3(KM_THREADS), 0, st, labels, centers, n, K, D, res, mask);
}

// Robust fundamental-matrix fit and the dense epipolar residual (include/mavflow_fundamental.h has the algorithm; tests/fundamental_ref.py
// restates it in numpy and the device equals it byte for byte).  Four kernels of the fit on one stream: the hypotheses' models (seven-point
// solver: elimination with full pivoting, the cubic by bracketing and bisection), the slots' inlier counts, the sequential choice, and the
// winner's mask and record; then the dense pass.  float64 throughout, compiled with -ffp-contract=off; integer counts from ballots; the
// only atomics are the dense pass's integer ones (a 64-bit max and two adds per workgroup), whose result does not depend on order: the same
// bytes on every run, at every batch position and in every context.  Every loop has a fixed bound; nothing is read through an index that
// was not range-checked first, whatever the subsets hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mavflow_internal.h"
#include "../../include/mavflow_fundamental.h"

#define FM_THREADS 256
#define FM_WAVES (FM_THREADS / 64)
#define FM_CHUNK 1024                   // pairs of one LDS chunk: 4 planes of doubles, 32 B per pair, 32 KiB
#define FM_SLOTS_PER_WAVE 4             // slots a wave scores per staged chunk where the grid is not capped
#define FM_GRID_CAP 2048                // workgroups of the score kernel in all items of a call
#define EPI_WG 256
#define EPI_CAP 512                     // workgroups per image of the dense pass (the warp_method pass's cap; 2048 measured slower here, profiles/fundamental/)

__device__ static inline bool fm_finite(double v) { return v - v == 0.0; }
__device__ static inline double fm_det3(double m0, double m1, double m2, double m3, double m4, double m5, double m6, double m7, double m8)
{
    return (m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6)) + m2 * (m3 * m7 - m4 * m6);
}
// det3 of `a` with row i taken from `b`
__device__ static inline double fm_det_row(const double* a, const double* b, int i)
{
    const double* r0 = i == 0 ? b : a;
    const double* r1 = i == 1 ? b : a;
    const double* r2 = i == 2 ? b : a;
    return fm_det3(r0[0], r0[1], r0[2], r1[3], r1[4], r1[5], r2[6], r2[7], r2[8]);
}
// the symmetric squared distance to the epipolar lines
__device__ static inline double fm_err(const double* f, double x, double y, double X, double Y)
{
    const double a = (f[0] * x + f[1] * y) + f[2], b = (f[3] * x + f[4] * y) + f[5], c = (f[6] * x + f[7] * y) + f[8];
    const double d2 = (X * a + Y * b) + c, s2 = 1.0 / (a * a + b * b);
    const double a_ = (f[0] * X + f[3] * Y) + f[6], b_ = (f[1] * X + f[4] * Y) + f[7], c_ = (f[2] * X + f[5] * Y) + f[8];
    const double d1 = (x * a_ + y * b_) + c_, s1 = 1.0 / (a_ * a_ + b_ * b_);
    const double e1 = (d1 * d1) * s1, e2 = (d2 * d2) * s2;
    return (e1 > e2 || e1 != e1) ? e1 : e2;
}

// ---- the hypotheses' models ----------------------------------------------------------------------------------------------------------------
// One lane per hypothesis, one wavefront per workgroup.  The 7 x 9 system lives in LDS, element-major and lane-minor (element e of lane l
// at e * 64 + l: the pivot search indexes it at run time, a private array would go to scratch memory, and this layout has no bank
// conflict).  A lane touches its own column of LDS only, so there is no barrier.  The column permutation is nine nibbles of one integer.
// Output per hypothesis: 27 doubles (three slots' models, zero where a slot is invalid) and one word of two int32 (slots with a root,
// bit mask of the valid ones).
#define FM_A(r, c) lds[((r) * 9 + (c)) * 64 + lane]
__global__ __launch_bounds__(64) void k_fm_models(FmCall a)
{
    __shared__ double lds[63 * 64];
    const int b = blockIdx.y, lane = threadIdx.x, it = blockIdx.x * 64 + lane, n = a.n;
    if (it >= a.max_iters) return;
    const double* src = a.src + (size_t)b * n * 2;
    const double* dst = a.dst + (size_t)b * n * 2;
    const int32_t* sub = a.subsets + ((size_t)b * a.max_iters + it) * 7;
    double* out = (double*)(a.ws + fm_models_offset(n)) + ((size_t)b * a.max_iters + it) * 28;
    double F[3][9];
    for (int s = 0; s < 3; s++)
        for (int j = 0; j < 9; j++) F[s][j] = 0.0;
    int nroots = 0, vmask = 0;

    int idx[7];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) { idx[j] = sub[j]; ok = ok && idx[j] >= 0 && idx[j] < n; }
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int i = 0; i < j; i++) ok = ok && idx[i] != idx[j];
    if (ok) {
#pragma unroll
        for (int r = 0; r < 7; r++) {
            const double x = src[2 * idx[r]], y = src[2 * idx[r] + 1], X = dst[2 * idx[r]], Y = dst[2 * idx[r] + 1];
            FM_A(r, 0) = X * x; FM_A(r, 1) = X * y; FM_A(r, 2) = X; FM_A(r, 3) = Y * x; FM_A(r, 4) = Y * y; FM_A(r, 5) = Y;
            FM_A(r, 6) = x; FM_A(r, 7) = y; FM_A(r, 8) = 1.0;
        }
        unsigned long long perm = 0x876543210ull;
#pragma unroll 1
        for (int k = 0; k < 7 && ok; k++) {
            double pv = 0.0;
            int pr = k, pc = k;
            for (int r = k; r < 7; r++)
                for (int c = k; c < 9; c++) {
                    const double v = fabs(FM_A(r, c));
                    if (v > pv) { pv = v; pr = r; pc = c; }
                }
            if (!(pv > 0.0 && fm_finite(pv))) { ok = false; break; }
            for (int c = 0; c < 9; c++) { const double t = FM_A(k, c); FM_A(k, c) = FM_A(pr, c); FM_A(pr, c) = t; }
            for (int r = 0; r < 7; r++) { const double t = FM_A(r, k); FM_A(r, k) = FM_A(r, pc); FM_A(r, pc) = t; }
            const unsigned long long nk = (perm >> (4 * k)) & 15ull, nc = (perm >> (4 * pc)) & 15ull;
            perm = (perm & ~(15ull << (4 * k))) | (nc << (4 * k));
            perm = (perm & ~(15ull << (4 * pc))) | (nk << (4 * pc));
            const double p = FM_A(k, k);
            for (int c = k + 1; c < 9; c++) FM_A(k, c) = FM_A(k, c) / p;
            for (int r = 0; r < 7; r++) {
                if (r == k) continue;
                const double m = FM_A(r, k);
                for (int c = k + 1; c < 9; c++) FM_A(r, c) = FM_A(r, c) - m * FM_A(k, c);
            }
        }
        if (ok) {
            double n1[7], n2[7];
#pragma unroll
            for (int i = 0; i < 7; i++) { n1[i] = FM_A(i, 7); n2[i] = FM_A(i, 8); }
            // the null vectors, un-permuted, through this lane's first 18 LDS elements (run-time indices again)
#pragma unroll
            for (int j = 0; j < 18; j++) lds[j * 64 + lane] = 0.0;
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const int q = (int)((perm >> (4 * i)) & 15ull);
                lds[q * 64 + lane] = -n1[i];
                lds[(9 + q) * 64 + lane] = -n2[i];
            }
            lds[(int)((perm >> 28) & 15ull) * 64 + lane] = 1.0;
            lds[(9 + (int)((perm >> 32) & 15ull)) * 64 + lane] = 1.0;
            double f1[9], f2[9];
#pragma unroll
            for (int j = 0; j < 9; j++) { f1[j] = lds[j * 64 + lane]; f2[j] = lds[(9 + j) * 64 + lane]; }

            const double c3 = fm_det3(f1[0], f1[1], f1[2], f1[3], f1[4], f1[5], f1[6], f1[7], f1[8]);
            const double c0 = fm_det3(f2[0], f2[1], f2[2], f2[3], f2[4], f2[5], f2[6], f2[7], f2[8]);
            const double c2 = (fm_det_row(f1, f2, 0) + fm_det_row(f1, f2, 1)) + fm_det_row(f1, f2, 2);
            const double c1 = (fm_det_row(f2, f1, 0) + fm_det_row(f2, f1, 1)) + fm_det_row(f2, f1, 2);
            double root[3] = {0.0, 0.0, 0.0};
            if (c3 != 0.0 && fm_finite(c3) && fm_finite(c2) && fm_finite(c1) && fm_finite(c0)) {
                const double q2 = fabs(c2 / c3), q1 = fabs(c1 / c3), q0 = fabs(c0 / c3);
                double mx = q2;
                mx = q1 > mx ? q1 : mx;
                mx = q0 > mx ? q0 : mx;
                const double R = 1.0 + mx;
                if (fm_finite(R)) {
                    auto horner = [&](double l) { return ((c3 * l + c2) * l + c1) * l + c0; };
                    const double disc = c2 * c2 - (3.0 * c3) * c1;
                    double e[4] = {-R, R, R, R};
                    int np = 2;
                    if (disc > 0.0) {
                        const double q = sqrt(disc);
                        const double u = (-c2 - q) / (3.0 * c3), v = (-c2 + q) / (3.0 * c3);
                        double ta = u < v ? u : v, tb = u < v ? v : u;
                        ta = ta < -R ? -R : (ta > R ? R : ta);
                        tb = tb < -R ? -R : (tb > R ? R : tb);
                        e[1] = ta; e[2] = tb;
                        np = 4;
                    }
                    double val[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) val[j] = horner(e[j]);
                    auto push = [&](double l) {
                        if (nroots == 0) root[0] = l;
                        else if (nroots == 1) root[1] = l;
                        else root[2] = l;
                        nroots++;
                    };
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (j >= np) continue;
                        if (val[j] == 0.0 && nroots < 3) push(e[j]);
                        if (j + 1 < np && ((val[j] < 0.0 && val[j < 3 ? j + 1 : 3] > 0.0) || (val[j] > 0.0 && val[j < 3 ? j + 1 : 3] < 0.0)) && nroots < 3) {
                            double lo = e[j], hi = e[j < 3 ? j + 1 : 3];
                            const bool neg = val[j] < 0.0;
                            for (int step = 0; step < 128; step++) {
                                const double mid = 0.5 * (lo + hi);
                                if (mid == lo || mid == hi) break;
                                const double fm = horner(mid);
                                if (fm == 0.0) { lo = mid; break; }
                                if ((fm < 0.0) == neg) lo = mid;
                                else hi = mid;
                            }
                            push(lo);
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 3; s++) {
                if (s >= nroots) continue;
                const double l = root[s];
                double G[9], q = 0.0;
#pragma unroll
                for (int j = 0; j < 9; j++) { G[j] = l * f1[j] + f2[j]; q = q + G[j] * G[j]; }
                const double nrm = sqrt(q);
                if (!(nrm > 0.0 && fm_finite(nrm))) continue;
                double big = 0.0, at = 0.0;
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    G[j] = G[j] / nrm;
                    if (fabs(G[j]) > big) { big = fabs(G[j]); at = G[j]; }
                }
                const bool flip = at < 0.0;
#pragma unroll
                for (int j = 0; j < 9; j++) F[s][j] = flip ? -G[j] : G[j];
                vmask |= 1 << s;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int j = 0; j < 9; j++) out[9 * s + j] = F[s][j];
    ((int32_t*)(out + 27))[0] = nroots;
    ((int32_t*)(out + 27))[1] = vmask;
}

// ---- the slots' counts --------------------------------------------------------------------------------------------------------------------
// grid (x, B).  A workgroup stages the item's pairs chunk by chunk in LDS; each of its four wavefronts scores one model slot at a time
// against the chunk, lanes striding over it, inliers counted by ballot and population count; lane 0 stores count[slot] (first chunk) or
// adds the chunk's count to it (later chunks; only this wavefront ever touches count[slot]).  The model is read from the workspace.
__global__ __launch_bounds__(FM_THREADS) void k_fm_score(FmCall a)
{
    __shared__ double sx[FM_CHUNK], sy[FM_CHUNK], sX[FM_CHUNK], sY[FM_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nslots = 3 * a.max_iters;
    const double* src = a.src + (size_t)b * a.n * 2;
    const double* dst = a.dst + (size_t)b * a.n * 2;
    const double* models = (const double*)(a.ws + fm_models_offset(a.n)) + (size_t)b * a.max_iters * 28;
    int32_t* count = (int32_t*)(a.ws + fm_counts_offset(a.n, a.B, a.max_iters)) + (size_t)b * nslots;
    const int first = blockIdx.x * FM_WAVES + wave, stride = gridDim.x * FM_WAVES;
    for (int base = 0; base < a.n; base += FM_CHUNK) {
        const int len = a.n - base < FM_CHUNK ? a.n - base : FM_CHUNK;
        __syncthreads();                                  // the previous chunk's readers are done
        for (int k = tid; k < len; k += FM_THREADS) {
            const size_t o = 2 * (size_t)(base + k);
            sx[k] = src[o]; sy[k] = src[o + 1]; sX[k] = dst[o]; sY[k] = dst[o + 1];
        }
        __syncthreads();
        for (int sl = first; sl < nslots; sl += stride) {
            const int it = sl / 3, s = sl - 3 * it;
            const double* m = models + (size_t)it * 28;
            const bool valid = (((const int32_t*)(m + 27))[1] >> s) & 1;
            int cnt = 0;
            if (valid) {
                double f[9];
#pragma unroll
                for (int j = 0; j < 9; j++) f[j] = m[9 * s + j];
                for (int k0 = 0; k0 < len; k0 += 64) {
                    const int k = k0 + lane;
                    bool in = false;
                    if (k < len) in = fm_err(f, sx[k], sy[k], sX[k], sY[k]) <= a.t2;          // a NaN error is no inlier
                    cnt += __popcll(__ballot(in));
                }
            }
            if (lane == 0) count[sl] = !valid ? -1 : base == 0 ? cnt : count[sl] + cnt;
        }
    }
}

// ---- the choice --------------------------------------------------------------------------------------------------------------------------
// One wavefront per item reproduces the sequential loop 64 slots at a time over the flattened slots (iteration = index / 3): within a
// block of 64 the next slot the loop would accept is the FIRST lane whose count beats best_count and whose iteration began -- it is
// below niters, or it is the iteration of the last accepted slot (an iteration that began is finished).  Accepting it moves best_count and
// niters, and the ballot is taken again.  choice[b] = (best slot index, iterations that began, valid slots among them, best_count).
__global__ __launch_bounds__(64) void k_fm_choose(FmCall a)
{
    const int b = blockIdx.x, lane = threadIdx.x, nslots = 3 * a.max_iters;
    const int32_t* need = (const int32_t*)a.ws;
    const int32_t* count = (const int32_t*)(a.ws + fm_counts_offset(a.n, a.B, a.max_iters)) + (size_t)b * nslots;
    int32_t* choice = (int32_t*)(a.ws + fm_choice_offset(a.n, a.B, a.max_iters)) + 4 * (size_t)b;
    int niters = a.max_iters, best = -1, best_it = -1, best_count = 6;
    for (int base = 0; base < nslots; base += 64) {
        if (base / 3 >= niters && base / 3 != best_it) break;
        const int sl = base + lane, it = sl / 3;
        const int c = sl < nslots ? count[sl] : -1;
        for (int r = 0; r < 64; r++) {
            const unsigned long long cand = __ballot(c > best_count && (it < niters || it == best_it));
            if (!cand) break;
            const int f = __ffsll((long long)cand) - 1;
            int cf = __shfl(c, f);
            cf = cf > a.n ? a.n : cf;                     // (a count never exceeds n; the table has n + 1 entries)
            best = base + f;
            best_it = best / 3;
            best_count = cf;
            const int nd = need[cf];
            niters = nd < niters ? nd : niters;
        }
    }
    const int ran = best < 0 ? a.max_iters : (niters > best_it + 1 ? niters : best_it + 1);
    int valid = 0;
    for (int base = 0; base < nslots; base += 64) {
        const int sl = base + lane;
        valid += __popcll(__ballot(sl < 3 * ran && count[sl] >= 0));
    }
    if (lane == 0) { choice[0] = best; choice[1] = ran; choice[2] = valid; choice[3] = best < 0 ? 0 : best_count; }
}

// ---- mask and record ------------------------------------------------------------------------------------------------------------------------
// The sum over k = 0 .. n - 1 in plain index order with one accumulator (the affine fit's form): all threads compute a chunk's terms into
// LDS, then thread 0 adds them up in order.
__global__ __launch_bounds__(FM_THREADS) void k_fm_finish(FmCall a)
{
    __shared__ double term[FM_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
    const double* src = a.src + (size_t)b * n * 2;
    const double* dst = a.dst + (size_t)b * n * 2;
    const int32_t* choice = (const int32_t*)(a.ws + fm_choice_offset(n, a.B, a.max_iters)) + 4 * (size_t)b;
    double* Fo = a.F + 9 * (size_t)b;
    uint8_t* inl = a.inliers + (size_t)b * n;
    mav_fundamental_record* rec = (mav_fundamental_record*)a.records + b;
    const int best = choice[0], ran = choice[1], valid = choice[2], g = choice[3];
    if (best < 0 || best >= 3 * a.max_iters) {            // (uniform over the workgroup)
        for (int k = tid; k < n; k += FM_THREADS) inl[k] = 0;
        if (tid < 9) Fo[tid] = 0.0;
        if (tid == 0) { rec->ok = 0; rec->inliers = 0; rec->best_iter = -1; rec->best_slot = -1; rec->iters_run = ran; rec->valid = valid; rec->sq_error = 0.0; }
        return;
    }
    const int it = best / 3, s = best - 3 * it;
    const double* m = (const double*)(a.ws + fm_models_offset(n)) + ((size_t)b * a.max_iters + it) * 28 + 9 * s;
    double f[9];
#pragma unroll
    for (int j = 0; j < 9; j++) f[j] = m[j];
    double sum = 0.0;
    for (int base = 0; base < n; base += FM_CHUNK) {
        const int len = n - base < FM_CHUNK ? n - base : FM_CHUNK;
        __syncthreads();
        for (int k = tid; k < len; k += FM_THREADS) {
            const int p = base + k;
            const double e = fm_err(f, src[2 * p], src[2 * p + 1], dst[2 * p], dst[2 * p + 1]);
            const bool in = e <= a.t2;
            inl[p] = in ? 1 : 0;
            term[k] = in ? e : 0.0;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < len; k++) sum = sum + term[k];
    }
    if (tid < 9) Fo[tid] = f[tid];
    if (tid == 0) { rec->ok = 1; rec->inliers = g; rec->best_iter = it; rec->best_slot = s; rec->iters_run = ran; rec->valid = valid; rec->sq_error = sum; }
}

// ---- the dense epipolar residual ------------------------------------------------------------------------------------------------------
// While a call runs, an image's record holds its key (64 bits), the movers and the not-finite count (32 bits each); k_epi_init clears them,
// the pass raises and adds, k_epi_finish writes the record over them.  The key of a pixel whose err is finite is
// bit 63 | (float bits of the residual << 32) | (0xFFFFFFFF - pixel index): the largest residual, the first pixel among equals (a residual
// is >= +0.0, so bit 63 is free; with it set, a key of 0 means that no pixel was finite).
__global__ void k_epi_init(unsigned long long* rec, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B)
        for (int j = 0; j < 4; j++) rec[4 * b + j] = 0ull;
}
__global__ void k_epi_finish(unsigned long long* rec, int B, int W)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long key = rec[4 * b];
    const uint32_t* cnt = (const uint32_t*)(rec + 4 * b + 1);
    const uint32_t movers = cnt[0], nf = cnt[1];
    mav_epipolar_record r;
    if (key) {
        const unsigned p = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        const unsigned row = p / (unsigned)W;
        r.max_residual = __uint_as_float((unsigned)(key >> 32) & 0x7FFFFFFFu);
        r.max_row = (int32_t)row;
        r.max_col = (int32_t)(p - row * (unsigned)W);
    } else {
        r.max_residual = 0.0f; r.max_row = -1; r.max_col = -1;
    }
    r.movers = (int32_t)movers; r.not_finite = (int32_t)nf; r.pad[0] = r.pad[1] = r.pad[2] = 0;
    *((mav_epipolar_record*)rec + b) = r;
}
__global__ __launch_bounds__(EPI_WG) void k_epipolar_residual(const float* __restrict__ flow_, const double* __restrict__ F_, double t2, int W, int H,
                                                              float* residual_, uint8_t* mask_, unsigned long long* rec)
{
    const size_t img = blockIdx.y, n0 = (size_t)W * H;
    const float* flow = flow_ + img * n0 * 2;
    float* residual = residual_ ? residual_ + img * n0 : nullptr;
    uint8_t* mask = mask_ ? mask_ + img * n0 : nullptr;
    double f[9];
#pragma unroll
    for (int j = 0; j < 9; j++) f[j] = F_[9 * img + j];
    unsigned long long best = 0ull;
    unsigned movers = 0, nf = 0;
    for (size_t p = (size_t)blockIdx.x * EPI_WG + threadIdx.x; p < n0; p += (size_t)gridDim.x * EPI_WG) {
        const int y = (int)((unsigned)p / (unsigned)W), x = (int)((unsigned)p - (unsigned)y * (unsigned)W);
        const double xd = (double)x, yd = (double)y;
        const double e = fm_err(f, xd, yd, xd + (double)flow[2 * p], yd + (double)flow[2 * p + 1]);
        const bool fin = fm_finite(e);
        const float r = fin ? (float)sqrt(e) : 0.0f;
        const bool mv = fin && e > t2;
        if (residual) residual[p] = r;
        if (mask) mask[p] = mv ? 255 : 0;
        movers += mv ? 1u : 0u;
        nf += fin ? 0u : 1u;
        if (fin) {
            const unsigned long long key = (1ull << 63) | ((unsigned long long)__float_as_uint(r) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
            best = key > best ? key : best;
        }
    }
    // the workgroup's maximum and counts meet in LDS first: one 64-bit atomicMax and two integer adds per workgroup
    __shared__ unsigned long long w_best[EPI_WG / 64];
    __shared__ unsigned w_mv[EPI_WG / 64], w_nf[EPI_WG / 64];
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
        movers += __shfl_xor(movers, o);
        nf += __shfl_xor(nf, o);
    }
    if ((threadIdx.x & 63) == 0) { w_best[threadIdx.x >> 6] = best; w_mv[threadIdx.x >> 6] = movers; w_nf[threadIdx.x >> 6] = nf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EPI_WG / 64; w++) { best = w_best[w] > best ? w_best[w] : best; movers += w_mv[w]; nf += w_nf[w]; }
        if (best) atomicMax(&rec[4 * img], best);
        if (movers) atomicAdd((unsigned*)(rec + 4 * img + 1), movers);
        if (nf) atomicAdd((unsigned*)(rec + 4 * img + 1) + 1, nf);
    }
}

void launch_fm_models(hipStream_t st, const FmCall& a) { hipLaunchKernelGGL(k_fm_models, dim3((a.max_iters + 63) / 64, a.B), dim3(64), 0, st, a); }
void launch_fm_score(hipStream_t st, const FmCall& a)
{
    const int slots = 3 * a.max_iters;
    const int per = (slots + FM_WAVES * FM_SLOTS_PER_WAVE - 1) / (FM_WAVES * FM_SLOTS_PER_WAVE);
    const int cap = FM_GRID_CAP / a.B < 1 ? 1 : FM_GRID_CAP / a.B;
    hipLaunchKernelGGL(k_fm_score, dim3(per < cap ? per : cap, a.B), dim3(FM_THREADS), 0, st, a);
}
void launch_fm_choose(hipStream_t st, const FmCall& a) { hipLaunchKernelGGL(k_fm_choose, dim3(a.B), dim3(64), 0, st, a); }
void launch_fm_finish(hipStream_t st, const FmCall& a) { hipLaunchKernelGGL(k_fm_finish, dim3(a.B), dim3(FM_THREADS), 0, st, a); }
void launch_epipolar_residual(hipStream_t st, const float* flow, const double* F, double t2, int W, int H, int B, float* residual, uint8_t* mask, void* records)
{
    unsigned long long* rec = (unsigned long long*)records;
    const dim3 one((B + 63) / 64), lanes(64);
    const size_t need = ((size_t)W * H + EPI_WG - 1) / EPI_WG;
    hipLaunchKernelGGL(k_epi_init, one, lanes, 0, st, rec, B);
    hipLaunchKernelGGL(k_epipolar_residual, dim3((unsigned)(need < EPI_CAP ? (need ? need : 1) : EPI_CAP), (unsigned)B), dim3(EPI_WG), 0, st, flow, F, t2, W, H,
                       residual, mask, rec);
    hipLaunchKernelGGL(k_epi_finish, one, lanes, 0, st, rec, B, W);
}

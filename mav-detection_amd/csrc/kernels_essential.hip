// Robust essential-matrix fit (include/mavflow_essential.h has the algorithm; tests/essential_ref.py restates it in numpy and the device
// equals it byte for byte).  Four kernels on one stream, the shape of kernels_fundamental.hip: the hypotheses' models (Nister's five-point
// solver: two eliminations, the tenth-degree polynomial, its real roots by a derivative ladder of bisections), the slots' inlier counts
// under the Sampson error, the sequential choice over ten slots per iteration, and the winner's mask, record, E and F.  float64
// throughout, compiled with -ffp-contract=off; integer counts from ballots; no atomics: the same bytes on every run, at every batch
// position and in every context.  Every loop has a fixed bound; nothing is read through an index that was not range-checked first,
// whatever the subsets hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mavflow_internal.h"
#include "../../include/mavflow_essential.h"

#define EM_THREADS 256
#define EM_WAVES (EM_THREADS / 64)
#define EM_CHUNK 1024                   // pairs of one LDS chunk: 4 planes of doubles, 32 B per pair, 32 KiB
#define EM_SLOTS_PER_WAVE 4             // slots a wave scores per staged chunk where the grid is not capped
#define EM_GRID_CAP 2048                // workgroups of the score kernel in all items of a call
#define EM_LANES 32                     // hypotheses of one workgroup of the models kernel
#define EM_ELEMS 245                    // doubles of LDS per hypothesis: 45 (the 5 x 9 system, then e1 .. e4) + 200 (the 10 x 20 matrix, then the ladder)

__device__ static inline bool em_finite(double v) { return v - v == 0.0; }
// the Sampson error on normalised points
__device__ static inline double em_err(const double* e, double x, double y, double X, double Y)
{
    const double a0 = (e[0] * x + e[1] * y) + e[2], a1 = (e[3] * x + e[4] * y) + e[5], a2 = (e[6] * x + e[7] * y) + e[8];
    const double b0 = (e[0] * X + e[3] * Y) + e[6], b1 = (e[1] * X + e[4] * Y) + e[7];
    const double d = (X * a0 + Y * a1) + a2;
    return (d * d) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}

// the place in Q of a product of two of (x, y, z, 1), and in C of a monomial of Q times one of (x, y, z, 1)
__device__ static const int EM_M2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
__device__ static const int EM_M3[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                                            {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
// (all loops below unroll completely: every index is a constant and the arrays live in registers)
__device__ static inline void em_mul2(const double* a, const double* b, double* q)
{
#pragma unroll
    for (int m = 0; m < 10; m++) q[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) q[EM_M2[i][j]] = q[EM_M2[i][j]] + a[i] * b[j];
}
__device__ static inline void em_mul3(const double* q, const double* l, double* c)
{
#pragma unroll
    for (int m = 0; m < 20; m++) c[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 10; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[EM_M3[i][j]] = c[EM_M3[i][j]] + q[i] * l[j];
}
// q = mul2(a, b) - mul2(c, d)
__device__ static inline void em_minor(const double* a, const double* b, const double* c, const double* d, double* q)
{
    double u[10], v[10];
    em_mul2(a, b, u);
    em_mul2(c, d, v);
#pragma unroll
    for (int m = 0; m < 10; m++) q[m] = u[m] - v[m];
}
// q = (mul2(a0, b0) + mul2(a1, b1)) + mul2(a2, b2)
__device__ static inline void em_dot2(const double* a0, const double* b0, const double* a1, const double* b1, const double* a2, const double* b2, double* q)
{
    double u[10], v[10], w[10];
    em_mul2(a0, b0, u);
    em_mul2(a1, b1, v);
    em_mul2(a2, b2, w);
#pragma unroll
    for (int m = 0; m < 10; m++) q[m] = (u[m] + v[m]) + w[m];
}
template <int DA, int DB>
__device__ static inline void em_conv(const double* a, const double* b, double* o)
{
#pragma unroll
    for (int m = 0; m <= DA + DB; m++) o[m] = 0.0;
#pragma unroll
    for (int i = 0; i <= DA; i++)
#pragma unroll
        for (int j = 0; j <= DB; j++) o[i + j] = o[i + j] + a[i] * b[j];
}
template <int D>
__device__ static inline double em_horner(const double* a, double t)
{
    double v = a[D];
#pragma unroll
    for (int j = D - 1; j >= 0; j--) v = v * t + a[j];
    return v;
}

// the header's POLISH: EM_POLISH_STEPS Gauss-Newton steps of p = (x, y, z) on the ten constraints, evaluated on the 3 x 3 matrix itself
#define EM_POLISH_STEPS 4
__device__ static inline double em_det3(const double* m)
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ static inline double em_abt(const double* a, const double* b, int i, int j)     // (A B^T)[i][j]
{
    return (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2];
}
__device__ static inline double em_ab(const double* a, const double* b, int i, int j)      // (A B)[i][j]
{
    return (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
__device__ static inline void em_polish(const double (&e)[4][9], double* p)
{
#pragma unroll 1
    for (int step = 0; step < EM_POLISH_STEPS; step++) {
        double G[9], S[9], r[10], C[9], J[3][10];
#pragma unroll
        for (int m = 0; m < 9; m++) G[m] = ((p[0] * e[0][m] + p[1] * e[1][m]) + p[2] * e[2][m]) + e[3][m];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) S[3 * i + j] = em_abt(G, G, i, j);
        const double h = 0.5 * ((S[0] + S[4]) + S[8]);
        r[0] = em_det3(G);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) r[1 + 3 * i + j] = em_ab(S, G, i, j) - h * G[3 * i + j];
        C[0] = G[4] * G[8] - G[5] * G[7]; C[1] = G[5] * G[6] - G[3] * G[8]; C[2] = G[3] * G[7] - G[4] * G[6];
        C[3] = G[2] * G[7] - G[1] * G[8]; C[4] = G[0] * G[8] - G[2] * G[6]; C[5] = G[1] * G[6] - G[0] * G[7];
        C[6] = G[1] * G[5] - G[2] * G[4]; C[7] = G[2] * G[3] - G[0] * G[5]; C[8] = G[0] * G[4] - G[1] * G[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double* D = e[q];
            double j0 = 0.0, T[9], dS[9];
#pragma unroll
            for (int m = 0; m < 9; m++) j0 = j0 + C[m] * D[m];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) T[3 * i + j] = em_abt(D, G, i, j);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) dS[3 * i + j] = T[3 * i + j] + T[3 * j + i];
            const double dh = 0.5 * ((dS[0] + dS[4]) + dS[8]);
            J[q][0] = j0;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    J[q][1 + 3 * i + j] = ((em_ab(dS, G, i, j) + em_ab(S, D, i, j)) - dh * G[3 * i + j]) - h * D[3 * i + j];
        }
        double N[9], g[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = a; b < 3; b++) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 10; k++) acc = acc + J[a][k] * J[b][k];
                N[3 * a + b] = acc;
                N[3 * b + a] = acc;
            }
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 10; k++) acc = acc + J[a][k] * r[k];
            g[a] = acc;
        }
        const double dd = em_det3(N);
        double delta[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            double Na[9];
#pragma unroll
            for (int m = 0; m < 9; m++) Na[m] = N[m];
            Na[a] = g[0]; Na[3 + a] = g[1]; Na[6 + a] = g[2];
            delta[a] = em_det3(Na) / dd;
        }
        if (dd != 0.0 && em_finite(delta[0]) && em_finite(delta[1]) && em_finite(delta[2])) {
#pragma unroll
            for (int a = 0; a < 3; a++) p[a] = p[a] - delta[a];
        }
    }
}

// ---- the hypotheses' models ----------------------------------------------------------------------------------------------------------------
// One lane per hypothesis, 32 hypotheses per workgroup: a hypothesis needs 245 doubles that are indexed at run time (the pivot searches,
// the row exchanges, the ladder's lists) -- a private array would go to scratch memory -- and 32 x 245 x 8 = 62720 bytes is what a
// 64 KiB static allocation holds.  Element e of lane l at e * 32 + l: 32 consecutive doubles, no bank conflict.  A lane touches its own
// column of LDS only, so there is no barrier.  The ten cubics are built in registers (every index a constant) and stored row by row.
// Output per hypothesis: EM_STRIDE doubles: ten slots' models (zero where a slot is invalid) and two int32 (slots with a root, bit mask
// of the valid ones).
#define EM_L(e) lds[(e) * EM_LANES + lane]
#define EM_A(r, c) EM_L((r) * 9 + (c))
#define EM_M(r, c) EM_L(45 + (r) * 20 + (c))
#define EM_DOFF(k) ((k) * 11 - ((k) * ((k) - 1)) / 2)                      // where the k-th derivative's 11 - k coefficients begin; 65 in all
#define EM_P(j) EM_L(45 + (j))                                             // the points of a level: 12 elements
#define EM_N(j) EM_L(57 + (j))                                             // the list a level makes: 10 elements
__global__ __launch_bounds__(EM_LANES) void k_em_models(EmCall a)
{
    __shared__ double lds[EM_ELEMS * EM_LANES];
    const int b = blockIdx.y, lane = threadIdx.x, it = blockIdx.x * EM_LANES + lane, n = a.n;
    if (it >= a.max_iters) return;
    const double* src = a.src + (size_t)b * n * 2;
    const double* dst = a.dst + (size_t)b * n * 2;
    const int32_t* sub = a.subsets + ((size_t)b * a.max_iters + it) * 5;
    double* out = (double*)(a.ws + em_models_offset(n)) + ((size_t)b * a.max_iters + it) * EM_STRIDE;
    int nroots = 0, vmask = 0;
    double B0[13], B1[13];                                // rows 0 and 1 of B(z): bx (4), by (4), b1 (5)
#pragma unroll
    for (int j = 0; j < 13; j++) { B0[j] = 0.0; B1[j] = 0.0; }

    do {
        int idx[5];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 5; j++) { idx[j] = sub[j]; ok = ok && idx[j] >= 0 && idx[j] < n; }
#pragma unroll
        for (int j = 0; j < 5; j++)
#pragma unroll
            for (int i = 0; i < j; i++) ok = ok && idx[i] != idx[j];
        if (!ok) break;
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const double x = (src[2 * idx[r]] - a.cx) / a.fx, y = (src[2 * idx[r] + 1] - a.cy) / a.fy;
            const double X = (dst[2 * idx[r]] - a.cx) / a.fx, Y = (dst[2 * idx[r] + 1] - a.cy) / a.fy;
            EM_A(r, 0) = X * x; EM_A(r, 1) = X * y; EM_A(r, 2) = X; EM_A(r, 3) = Y * x; EM_A(r, 4) = Y * y; EM_A(r, 5) = Y;
            EM_A(r, 6) = x; EM_A(r, 7) = y; EM_A(r, 8) = 1.0;
        }
        unsigned long long perm = 0x876543210ull;
#pragma unroll 1
        for (int k = 0; k < 5 && ok; k++) {
            double pv = 0.0;
            int pr = k, pc = k;
            for (int r = k; r < 5; r++)
                for (int c = k; c < 9; c++) {
                    const double v = fabs(EM_A(r, c));
                    if (v > pv) { pv = v; pr = r; pc = c; }
                }
            if (!(pv > 0.0 && em_finite(pv))) { ok = false; break; }
            for (int c = 0; c < 9; c++) { const double t = EM_A(k, c); EM_A(k, c) = EM_A(pr, c); EM_A(pr, c) = t; }
            for (int r = 0; r < 5; r++) { const double t = EM_A(r, k); EM_A(r, k) = EM_A(r, pc); EM_A(r, pc) = t; }
            const unsigned long long nk = (perm >> (4 * k)) & 15ull, nc = (perm >> (4 * pc)) & 15ull;
            perm = (perm & ~(15ull << (4 * k))) | (nc << (4 * k));
            perm = (perm & ~(15ull << (4 * pc))) | (nk << (4 * pc));
            const double p = EM_A(k, k);
            for (int c = k + 1; c < 9; c++) EM_A(k, c) = EM_A(k, c) / p;
            for (int r = 0; r < 5; r++) {
                if (r == k) continue;
                const double m = EM_A(r, k);
                for (int c = k + 1; c < 9; c++) EM_A(r, c) = EM_A(r, c) - m * EM_A(k, c);
            }
        }
        if (!ok) break;
        {
            // the null vectors, un-permuted, through this lane's first 36 LDS elements (run-time indices again): ej at 9 * (j - 1)
            double nv[4][5];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 5; i++) nv[j][i] = EM_A(i, 5 + j);
#pragma unroll
            for (int e = 0; e < 36; e++) EM_L(e) = 0.0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int i = 0; i < 5; i++) EM_L(9 * j + (int)((perm >> (4 * i)) & 15ull)) = -nv[j][i];
                EM_L(9 * j + (int)((perm >> (4 * (5 + j))) & 15ull)) = 1.0;
            }
        }
        {
            // the ten cubics; E[m] is the linear form of entry m
            double E[9][4];
#pragma unroll
            for (int m = 0; m < 9; m++)
#pragma unroll
                for (int j = 0; j < 4; j++) E[m][j] = EM_L(9 * j + m);
            {
                double P0[10], P1[10], P2[10], t0[20], t1[20], t2[20];
                em_minor(E[4], E[8], E[5], E[7], P0);
                em_minor(E[3], E[8], E[5], E[6], P1);
                em_minor(E[3], E[7], E[4], E[6], P2);
                em_mul3(P0, E[0], t0);
                em_mul3(P1, E[1], t1);
                em_mul3(P2, E[2], t2);
#pragma unroll
                for (int c = 0; c < 20; c++) EM_M(0, c) = (t0[c] - t1[c]) + t2[c];
            }
            double S[3][3][10];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = i; j < 3; j++) em_dot2(E[3 * i], E[3 * j], E[3 * i + 1], E[3 * j + 1], E[3 * i + 2], E[3 * j + 2], S[i][j]);
#pragma unroll
            for (int m = 0; m < 10; m++) {
                const double T = (S[0][0][m] + S[1][1][m]) + S[2][2][m];
                const double h = 0.5 * T;
                S[0][0][m] = S[0][0][m] - h; S[1][1][m] = S[1][1][m] - h; S[2][2][m] = S[2][2][m] - h;
                S[1][0][m] = S[0][1][m]; S[2][0][m] = S[0][2][m]; S[2][1][m] = S[1][2][m];
            }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    double t0[20], t1[20], t2[20];
                    em_mul3(S[i][0], E[j], t0);
                    em_mul3(S[i][1], E[3 + j], t1);
                    em_mul3(S[i][2], E[6 + j], t2);
#pragma unroll
                    for (int c = 0; c < 20; c++) EM_M(1 + 3 * i + j, c) = (t0[c] + t1[c]) + t2[c];
                }
        }
#pragma unroll 1
        for (int k = 0; k < 10 && ok; k++) {
            double pv = 0.0;
            int pr = k;
            for (int r = k; r < 10; r++) {
                const double v = fabs(EM_M(r, k));
                if (v > pv) { pv = v; pr = r; }
            }
            if (!(pv > 0.0 && em_finite(pv))) { ok = false; break; }
            for (int c = k; c < 20; c++) { const double t = EM_M(k, c); EM_M(k, c) = EM_M(pr, c); EM_M(pr, c) = t; }
            const double p = EM_M(k, k);
            for (int c = k + 1; c < 20; c++) EM_M(k, c) = EM_M(k, c) / p;
            for (int r = 0; r < 10; r++) {
                if (r == k || !(r > k || r >= 4)) continue;
                const double m = EM_M(r, k);
                for (int c = k + 1; c < 20; c++) EM_M(r, c) = EM_M(r, c) - m * EM_M(k, c);
            }
        }
        if (!ok) break;
        double c[11];
        {
            double B2[13];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double e[10], f[10], B[13];
#pragma unroll
                for (int j = 0; j < 10; j++) { e[j] = EM_M(4 + 2 * q, 10 + j); f[j] = EM_M(5 + 2 * q, 10 + j); }
                B[0] = e[2]; B[1] = e[1] - f[2]; B[2] = e[0] - f[1]; B[3] = -f[0];
                B[4] = e[5]; B[5] = e[4] - f[5]; B[6] = e[3] - f[4]; B[7] = -f[3];
                B[8] = e[9]; B[9] = e[8] - f[9]; B[10] = e[7] - f[8]; B[11] = e[6] - f[7]; B[12] = -f[6];
#pragma unroll
                for (int j = 0; j < 13; j++) {
                    if (q == 0) B0[j] = B[j];
                    if (q == 1) B1[j] = B[j];
                    if (q == 2) B2[j] = B[j];
                }
            }
            double u[8], v[8], p1[8], p2[8], p3[7], w3[7], x3[7];
            em_conv<3, 4>(B1 + 4, B2 + 8, u); em_conv<4, 3>(B1 + 8, B2 + 4, v);
#pragma unroll
            for (int j = 0; j < 8; j++) p1[j] = u[j] - v[j];
            em_conv<3, 4>(B1, B2 + 8, u); em_conv<4, 3>(B1 + 8, B2, v);
#pragma unroll
            for (int j = 0; j < 8; j++) p2[j] = u[j] - v[j];
            em_conv<3, 3>(B1, B2 + 4, w3); em_conv<3, 3>(B1 + 4, B2, x3);
#pragma unroll
            for (int j = 0; j < 7; j++) p3[j] = w3[j] - x3[j];
            double t0[11], t1[11], t2[11];
            em_conv<3, 7>(B0, p1, t0); em_conv<3, 7>(B0 + 4, p2, t1); em_conv<4, 6>(B0 + 8, p3, t2);
#pragma unroll
            for (int j = 0; j < 11; j++) c[j] = (t0[j] - t1[j]) + t2[j];
        }
        bool fin = c[10] != 0.0;
#pragma unroll
        for (int j = 0; j < 11; j++) fin = fin && em_finite(c[j]);
        if (!fin) break;
        double mx = 0.0;
#pragma unroll
        for (int j = 0; j < 10; j++) { const double q = fabs(c[j] / c[10]); mx = q > mx ? q : mx; }
        const double R = 1.0 + mx;
        if (!em_finite(R)) break;
        // the derivative ladder: the derivatives' coefficients in registers (the level loop unrolls completely, so every index into D
        // is a constant), the points and lists in the LDS the matrix has left
        double D[65];
#pragma unroll
        for (int j = 0; j < 11; j++) D[j] = c[j];
#pragma unroll
        for (int k = 0; k < 9; k++)
#pragma unroll
            for (int j = 1; j <= 10 - k; j++) D[EM_DOFF(k + 1) + j - 1] = (double)j * D[EM_DOFF(k) + j];
        int m = 1;
        {
            const double t = (-D[EM_DOFF(9)]) / D[EM_DOFF(9) + 1];
            EM_P(1) = t < -R ? -R : (t > R ? R : t);
        }
#pragma unroll
        for (int k = 8; k >= 0; k--) {
            const int d = 10 - k, np = m + 2;
            auto horner = [&](double t) {
                double v = D[EM_DOFF(k) + d];
#pragma unroll
                for (int j = d - 1; j >= 0; j--) v = v * t + D[EM_DOFF(k) + j];
                return v;
            };
            EM_P(0) = -R;
            EM_P(m + 1) = R;
            int cnt = 0;
            double vj = horner(-R);
            for (int j = 0; j < 12; j++) {
                if (j >= np) break;
                const double ej = EM_P(j);
                if (vj == 0.0 && cnt < d) { EM_N(cnt) = ej; cnt++; }
                if (j + 1 < np) {
                    const double en = EM_P(j + 1), vn = horner(en);
                    if (((vj < 0.0 && vn > 0.0) || (vj > 0.0 && vn < 0.0)) && cnt < d) {
                        double lo = ej, hi = en;
                        const bool neg = vj < 0.0;
                        for (int step = 0; step < 128; step++) {
                            const double mid = 0.5 * (lo + hi);
                            if (mid == lo || mid == hi) break;
                            const double fm = horner(mid);
                            if (fm == 0.0) { lo = mid; break; }
                            if ((fm < 0.0) == neg) lo = mid;
                            else hi = mid;
                        }
                        EM_N(cnt) = lo;
                        cnt++;
                    }
                    vj = vn;
                }
            }
            for (int i = 0; i < 10; i++)
                if (i < cnt) EM_P(1 + i) = EM_N(i);
            m = cnt;
        }
        nroots = m;
    } while (false);

    // the slots: root s is EM_P(1 + s), e1 .. e4 are this lane's first 36 elements
    for (int s = 0; s < EM_SLOTS; s++) {
        double G[9];
        bool valid = false;
        if (s < nroots) {
            const double z = EM_P(1 + s);
            const double kx = em_horner<3>(B0, z), ky = em_horner<3>(B0 + 4, z), k1 = em_horner<4>(B0 + 8, z);
            const double lx = em_horner<3>(B1, z), ly = em_horner<3>(B1 + 4, z), l1 = em_horner<4>(B1 + 8, z);
            const double v0 = ky * l1 - k1 * ly, v1 = k1 * lx - kx * l1, v2 = kx * ly - ky * lx;
            const double x = v0 / v2, y = v1 / v2;
            if (v2 != 0.0 && em_finite(x) && em_finite(y)) {
                double ev[4][9];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int m = 0; m < 9; m++) ev[j][m] = EM_L(9 * j + m);
                double p[3] = {x, y, z};
                em_polish(ev, p);
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    G[j] = ((p[0] * ev[0][j] + p[1] * ev[1][j]) + p[2] * ev[2][j]) + ev[3][j];
                    q = q + G[j] * G[j];
                }
                const double nrm = sqrt(q);
                if (nrm > 0.0 && em_finite(nrm)) {
                    double big = 0.0, at = 0.0;
#pragma unroll
                    for (int j = 0; j < 9; j++) {
                        G[j] = G[j] / nrm;
                        if (fabs(G[j]) > big) { big = fabs(G[j]); at = G[j]; }
                    }
                    const bool flip = at < 0.0;
#pragma unroll
                    for (int j = 0; j < 9; j++) G[j] = flip ? -G[j] : G[j];
                    valid = true;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 9; j++) out[9 * s + j] = valid ? G[j] : 0.0;
        vmask |= valid ? 1 << s : 0;
    }
    ((int32_t*)(out + 90))[0] = nroots;
    ((int32_t*)(out + 90))[1] = vmask;
}

// ---- the slots' counts --------------------------------------------------------------------------------------------------------------------
// k_fm_score's structure with ten slots per hypothesis: a workgroup stages the item's pairs chunk by chunk in LDS, NORMALISED as they are
// staged; each of its four wavefronts scores one model slot at a time against the chunk, inliers counted by ballot and population count;
// lane 0 stores count[slot] (first chunk) or adds the chunk's count to it (only this wavefront ever touches count[slot]).
__global__ __launch_bounds__(EM_THREADS) void k_em_score(EmCall a)
{
    __shared__ double sx[EM_CHUNK], sy[EM_CHUNK], sX[EM_CHUNK], sY[EM_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nslots = EM_SLOTS * a.max_iters;
    const double* src = a.src + (size_t)b * a.n * 2;
    const double* dst = a.dst + (size_t)b * a.n * 2;
    const double* models = (const double*)(a.ws + em_models_offset(a.n)) + (size_t)b * a.max_iters * EM_STRIDE;
    int32_t* count = (int32_t*)(a.ws + em_counts_offset(a.n, a.B, a.max_iters)) + (size_t)b * nslots;
    const int first = blockIdx.x * EM_WAVES + wave, stride = gridDim.x * EM_WAVES;
    for (int base = 0; base < a.n; base += EM_CHUNK) {
        const int len = a.n - base < EM_CHUNK ? a.n - base : EM_CHUNK;
        __syncthreads();                                  // the previous chunk's readers are done
        for (int k = tid; k < len; k += EM_THREADS) {
            const size_t o = 2 * (size_t)(base + k);
            sx[k] = (src[o] - a.cx) / a.fx; sy[k] = (src[o + 1] - a.cy) / a.fy; sX[k] = (dst[o] - a.cx) / a.fx; sY[k] = (dst[o + 1] - a.cy) / a.fy;
        }
        __syncthreads();
        for (int sl = first; sl < nslots; sl += stride) {
            const int it = sl / EM_SLOTS, s = sl - EM_SLOTS * it;
            const double* m = models + (size_t)it * EM_STRIDE;
            const bool valid = (((const int32_t*)(m + 90))[1] >> s) & 1;
            int cnt = 0;
            if (valid) {
                double f[9];
#pragma unroll
                for (int j = 0; j < 9; j++) f[j] = m[9 * s + j];
                for (int k0 = 0; k0 < len; k0 += 64) {
                    const int k = k0 + lane;
                    bool in = false;
                    if (k < len) in = em_err(f, sx[k], sy[k], sX[k], sY[k]) <= a.t2;          // a NaN error is no inlier
                    cnt += __popcll(__ballot(in));
                }
            }
            if (lane == 0) count[sl] = !valid ? -1 : base == 0 ? cnt : count[sl] + cnt;
        }
    }
}

// ---- the choice --------------------------------------------------------------------------------------------------------------------------
// k_fm_choose with ten slots per iteration: one wavefront per item reproduces the sequential loop 64 slots at a time over the flattened
// slots (iteration = index / 10): within a block of 64 the next slot the loop would accept is the FIRST lane whose count beats best_count
// and whose iteration began -- it is below niters, or it is the iteration of the last accepted slot (an iteration that began is finished,
// also where its ten slots lie either side of a block boundary: the next block is entered while its first slot's iteration is that one).
// choice[b] = (best slot index, iterations that began, valid slots among them, best_count).
__global__ __launch_bounds__(64) void k_em_choose(EmCall a)
{
    const int b = blockIdx.x, lane = threadIdx.x, nslots = EM_SLOTS * a.max_iters;
    const int32_t* need = (const int32_t*)a.ws;
    const int32_t* count = (const int32_t*)(a.ws + em_counts_offset(a.n, a.B, a.max_iters)) + (size_t)b * nslots;
    int32_t* choice = (int32_t*)(a.ws + em_choice_offset(a.n, a.B, a.max_iters)) + 4 * (size_t)b;
    int niters = a.max_iters, best = -1, best_it = -1, best_count = 4;
    for (int base = 0; base < nslots; base += 64) {
        if (base / EM_SLOTS >= niters && base / EM_SLOTS != best_it) break;
        const int sl = base + lane, it = sl / EM_SLOTS;
        const int c = sl < nslots ? count[sl] : -1;
        for (int r = 0; r < 64; r++) {
            const unsigned long long cand = __ballot(c > best_count && (it < niters || it == best_it));
            if (!cand) break;
            const int f = __ffsll((long long)cand) - 1;
            int cf = __shfl(c, f);
            cf = cf > a.n ? a.n : cf;                     // (a count never exceeds n; the table has n + 1 entries)
            best = base + f;
            best_it = best / EM_SLOTS;
            best_count = cf;
            const int nd = need[cf];
            niters = nd < niters ? nd : niters;
        }
    }
    const int ran = best < 0 ? a.max_iters : (niters > best_it + 1 ? niters : best_it + 1);
    int valid = 0;
    for (int base = 0; base < nslots; base += 64) {
        const int sl = base + lane;
        valid += __popcll(__ballot(sl < EM_SLOTS * ran && count[sl < nslots ? sl : 0] >= 0));
    }
    if (lane == 0) { choice[0] = best; choice[1] = ran; choice[2] = valid; choice[3] = best < 0 ? 0 : best_count; }
}

// ---- mask, record, E and F ----------------------------------------------------------------------------------------------------------------
// k_fm_finish's structure: the sum over k = 0 .. n - 1 in plain index order with one accumulator; thread 0 forms F = K^-T E K^-1.
__global__ __launch_bounds__(EM_THREADS) void k_em_finish(EmCall a)
{
    __shared__ double term[EM_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
    const double* src = a.src + (size_t)b * n * 2;
    const double* dst = a.dst + (size_t)b * n * 2;
    const int32_t* choice = (const int32_t*)(a.ws + em_choice_offset(n, a.B, a.max_iters)) + 4 * (size_t)b;
    double *Eo = a.E + 9 * (size_t)b, *Fo = a.F + 9 * (size_t)b;
    uint8_t* inl = a.inliers + (size_t)b * n;
    mav_essential_record* rec = (mav_essential_record*)a.records + b;
    const int best = choice[0], ran = choice[1], valid = choice[2], g = choice[3];
    if (best < 0 || best >= EM_SLOTS * a.max_iters) {     // (uniform over the workgroup)
        for (int k = tid; k < n; k += EM_THREADS) inl[k] = 0;
        if (tid < 9) { Eo[tid] = 0.0; Fo[tid] = 0.0; }
        if (tid == 0) { rec->ok = 0; rec->inliers = 0; rec->best_iter = -1; rec->best_slot = -1; rec->iters_run = ran; rec->valid = valid; rec->sq_error = 0.0; }
        return;
    }
    const int it = best / EM_SLOTS, s = best - EM_SLOTS * it;
    const double* m = (const double*)(a.ws + em_models_offset(n)) + ((size_t)b * a.max_iters + it) * EM_STRIDE + 9 * s;
    double f[9];
#pragma unroll
    for (int j = 0; j < 9; j++) f[j] = m[j];
    double sum = 0.0;
    for (int base = 0; base < n; base += EM_CHUNK) {
        const int len = n - base < EM_CHUNK ? n - base : EM_CHUNK;
        __syncthreads();
        for (int k = tid; k < len; k += EM_THREADS) {
            const int p = base + k;
            const double x = (src[2 * p] - a.cx) / a.fx, y = (src[2 * p + 1] - a.cy) / a.fy;
            const double X = (dst[2 * p] - a.cx) / a.fx, Y = (dst[2 * p + 1] - a.cy) / a.fy;
            const double e = em_err(f, x, y, X, Y);
            const bool in = e <= a.t2;
            inl[p] = in ? 1 : 0;
            term[k] = in ? e : 0.0;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < len; k++) sum = sum + term[k];
    }
    if (tid < 9) Eo[tid] = f[tid];
    if (tid == 0) {
        double G[9], H[9];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            G[3 * i] = f[3 * i] / a.fx;
            G[3 * i + 1] = f[3 * i + 1] / a.fy;
            G[3 * i + 2] = (f[3 * i + 2] - G[3 * i] * a.cx) - G[3 * i + 1] * a.cy;
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            H[j] = G[j] / a.fx;
            H[3 + j] = G[3 + j] / a.fy;
            H[6 + j] = (G[6 + j] - H[j] * a.cx) - H[3 + j] * a.cy;
        }
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 9; j++) q = q + H[j] * H[j];
        const double nrm = sqrt(q);
        const bool fok = nrm > 0.0 && em_finite(nrm);
        double big = 0.0, at = 0.0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            H[j] = H[j] / nrm;
            if (fabs(H[j]) > big) { big = fabs(H[j]); at = H[j]; }
        }
        const bool flip = at < 0.0;
#pragma unroll
        for (int j = 0; j < 9; j++) Fo[j] = !fok ? 0.0 : flip ? -H[j] : H[j];
        rec->ok = 1; rec->inliers = g; rec->best_iter = it; rec->best_slot = s; rec->iters_run = ran; rec->valid = valid; rec->sq_error = sum;
    }
}

void launch_em_models(hipStream_t st, const EmCall& a)
{
    hipLaunchKernelGGL(k_em_models, dim3((a.max_iters + EM_LANES - 1) / EM_LANES, a.B), dim3(EM_LANES), 0, st, a);
}
void launch_em_score(hipStream_t st, const EmCall& a)
{
    const int slots = EM_SLOTS * a.max_iters;
    const int per = (slots + EM_WAVES * EM_SLOTS_PER_WAVE - 1) / (EM_WAVES * EM_SLOTS_PER_WAVE);
    const int cap = EM_GRID_CAP / a.B < 1 ? 1 : EM_GRID_CAP / a.B;
    hipLaunchKernelGGL(k_em_score, dim3(per < cap ? per : cap, a.B), dim3(EM_THREADS), 0, st, a);
}
void launch_em_choose(hipStream_t st, const EmCall& a) { hipLaunchKernelGGL(k_em_choose, dim3(a.B), dim3(64), 0, st, a); }
void launch_em_finish(hipStream_t st, const EmCall& a) { hipLaunchKernelGGL(k_em_finish, dim3(a.B), dim3(EM_THREADS), 0, st, a); }

// Dense-flow kernels for gfx950 (MI355X): Gaussian pyramid layer, polynomial expansion, UpdateMatrices and the
// fused {box blur -> 2x2 solve -> UpdateMatrices} iteration of Farneback's algorithm.
//
// What they compute is cv2.calcOpticalFlowFarneback as called at /root/reference/src/farneback.py:76-80
// (OpenCV modules/video/src/optflowgf.cpp).  How they compute it is new: M lives in HBM as 5
// separate f32 planes per pair (coalesced 128-B row segments per wave), R as (h, w, 5), every stencil stage stages
// its tile + halo through LDS once, box sums are separable sliding sums done in place in LDS, and the solve and
// the next UpdateMatrices are fused behind the blur so M makes exactly one HBM round trip per iteration.
// The path is HBM/LDS-bound stencil work: no MFMA.
#include "mavflow_internal.h"

#include <algorithm>
#include <type_traits>

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------------
// Workgroup -> tile mapping shared by the tiled kernels (64 x 16 pixel tiles over G images).
// Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one, each XCD has its own 4 MB L2), so workgroup b
// takes tile (b & 7) * per + (b >> 3): every XCD walks ONE contiguous run of tiles and the halo rows / gather rows that
// vertically adjacent tiles share are re-read from that XCD's L2 instead of HBM (a plain 2-D grid puts neighbours on
// different XCDs: measured 3.9x read over-fetch in the expansion kernel).  Inside an image the run goes through column
// STRIPS of strip_w tiles, row by row inside a strip: the tiles resident on an XCD at one time (~160) then span several
// tile rows of the strip, so a tile's upper neighbour is still in L2 when it is needed -- on a 3840-wide layer one tile row
// is 60 tiles and without strips the reuse distance exceeds the L2.  Speed only: every tile is computed exactly once and
// nothing depends on the order.  Grid = n_tiles rounded up to a multiple of 8.
// ------------------------------------------------------------------------------------------------------------
struct TileMap { int tiles_x, tiles_y, per_img, n_tiles, strip_w, xcd, ty0; };   // xcd = 0: plain row-major order; ty0: first tile row (a band launch)
static __device__ __forceinline__ bool tile_of_block(const TileMap& tm, int* s, int* tx, int* ty)
{
    const int per = ((int)gridDim.x + 7) >> 3;
    const int tile = tm.xcd ? (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (tile >= tm.n_tiles) return false;
    const int img = tile / tm.per_img;
    int tr = tile - img * tm.per_img;
    const int strip_tiles = tm.strip_w * tm.tiles_y;          // every strip but the last is strip_w tiles wide
    const int st = tr / strip_tiles;
    tr -= st * strip_tiles;
    const int x_base = st * tm.strip_w;
    const int sw = min(tm.strip_w, tm.tiles_x - x_base);
    const int row = tr / sw;
    *s = img; *ty = row + tm.ty0; *tx = x_base + tr - row * sw;
    return true;
}
// rows [ty0, ty1) of the tile grid only (a band of the image); ty1 < 0 = all rows.  strip > 0: strips of that many tiles (option "strip").
static TileMap make_tile_map(int w, int h, int G, int tile_w, int tile_h, int ty0 = 0, int ty1 = -1, int strip = 0)
{
    TileMap tm;
    tm.xcd = 1;
    tm.tiles_x = (w + tile_w - 1) / tile_w;
    tm.tiles_y = (h + tile_h - 1) / tile_h;
    tm.ty0 = ty0 > 0 ? (ty0 < tm.tiles_y ? ty0 : tm.tiles_y) : 0;
    if (ty1 >= 0 && ty1 < tm.tiles_y) tm.tiles_y = ty1;
    tm.tiles_y = tm.tiles_y > tm.ty0 ? tm.tiles_y - tm.ty0 : 0;
    tm.per_img = tm.tiles_x * tm.tiles_y;
    tm.n_tiles = tm.per_img * G;
    int sw = tm.tiles_x;
    if (strip > 0) sw = strip < tm.tiles_x ? strip : tm.tiles_x;
    else if (tm.tiles_x > 40) { const int ns = (tm.tiles_x + 29) / 30; sw = (tm.tiles_x + ns - 1) / ns; }
    tm.strip_w = sw;
    return tm;
}
static inline unsigned tile_grid(const TileMap& tm) { return (unsigned)(((tm.n_tiles + 7) / 8) * 8); }

#ifdef MAV_STAMPS   // diagnostic build only (tools/phase_stamps.py): per-phase wave cycles of the sweep kernel, never in the product .so
#define MAV_STAMP_WAVES (1 << 17)
__device__ unsigned long long g_phase_cycles[MAV_STAMP_WAVES * 8];   // one row per wave slot of a launch: plain += (launches are serial)
#define STAMP(var) unsigned long long var; __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory"); __builtin_amdgcn_sched_barrier(0)
#define STAMP_ADD(i, a, b) do { if ((threadIdx.x & 63) == 0) { const unsigned wid = (blockIdx.x * 4u + (threadIdx.x >> 6)) & (MAV_STAMP_WAVES - 1); g_phase_cycles[wid * 8 + (i)] += (unsigned long long)((b) - (a)); } } while (0)
extern "C" int mav_debug_read_stamps(unsigned long long* out, int reset)
{
    static unsigned long long host[MAV_STAMP_WAVES * 8];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase_cycles), sizeof(host)) != hipSuccess) return -1;
    for (int i = 0; i < 8; i++) out[i] = 0;
    for (size_t w = 0; w < MAV_STAMP_WAVES; w++) for (int i = 0; i < 8; i++) out[i] += host[w * 8 + i];
    if (reset) { static unsigned long long z[MAV_STAMP_WAVES * 8]; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#else
#define STAMP(var)
#define STAMP_ADD(i, a, b)
#endif

// ------------------------------------------------------------------------------------------------------------
// Layer image: convertTo(f32) -> GaussianBlur(ksize, sigma, REFLECT_101) -> resize(INTER_LINEAR)   (A.2).
// ------------------------------------------------------------------------------------------------------------
// Two separable passes for the coarse layers (any ksize / scale), table-free: along each axis the output is
//   a0 * B[s0] + a1 * B[s0 + 1],   B[c] = sum_t g[t] * src[reflect101(c - r + t)]
// with (s0, a1) from the half-pixel-centre rule of resize(INTER_LINEAR).  Away from the border the two Gaussian sums share
// their pixels (B[s0+1] is B[s0] shifted by one), so a tap costs one load and two FMAs; g[t] is wave-uniform (scalar loads).
//   pass H   tmp[y][dx]   for every source row y            (H x w f32; 4 rows per thread share the column arithmetic)
//   pass V   out[dy][dx]  from tmp                          (h x w f32)
// MACs per output drop from (ksize+1)^2 to ~(ksize+1)(H/h + 1): the 95-tap layer of the 4K / 5-layer preset costs the same as
// the 5-tap one.
static __device__ __forceinline__ void resize_coord(int o, int S, int d, double scale, int* s0, float* f)
{
#pragma clang fp contract(off)                       // (o + 0.5) * scale - 0.5 with separate roundings, as OpenCV's host code evaluates it
    if (d == S) { *s0 = o; *f = 0.f; return; }
    float t = (float)((o + 0.5) * scale - 0.5);
    int s = (int)floorf(t);
    t -= s;
    if (s < 0) { t = 0.f; s = 0; }
    if (s >= S - 1) { t = 0.f; s = S - 1; }
    *s0 = s; *f = t;
}
static __device__ __forceinline__ int reflect101d(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// Image z of a launch over two runs of images (the `prev` frames and the `next` frames of a group): z < split comes from run a.
template <typename T>
static __device__ __forceinline__ const T* image_of(const T* a, const T* b, int split, size_t stride, int z)
{
    return z < split ? a + (size_t)z * stride : b + (size_t)(z - split) * stride;
}

// Source depths.  A frame is uint8_t, uint16_t or float (cv2's CV_8U, CV_16U, CV_32F); every loader below converts a pixel with
// (float)v -- convertTo(CV_32F), exact for both integer depths -- and everything after that conversion is the same arithmetic in the
// same order for every depth, so frames of any depth that hold the same values give the same bits.  A QUAD is four consecutive pixels,
// the unit of the staged / aligned loads: one dword of u8, two of u16, four of f32.  The u8 forms keep their dword streams re-aligned
// with v_alignbyte; the wider forms read their pixels from LDS one element at a time (an element is LDS-addressable, so no re-alignment).
template <typename T> struct QuadOf;
template <> struct QuadOf<uint8_t> { typedef uint32_t type; };
template <> struct QuadOf<uint16_t> { typedef uint2 type; };
template <> struct QuadOf<float> { typedef uint4 type; };
template <typename T>      // the wider depths' quads (the u8 forms unpack their dwords where they use them)
static __device__ __forceinline__ void quad_px(typename QuadOf<T>::type q, float o[4])
{
    if constexpr (sizeof(T) == 2) {
        o[0] = (float)(q.x & 0xffffu); o[1] = (float)(q.x >> 16); o[2] = (float)(q.y & 0xffffu); o[3] = (float)(q.y >> 16);
    } else {
        o[0] = __uint_as_float(q.x); o[1] = __uint_as_float(q.y); o[2] = __uint_as_float(q.z); o[3] = __uint_as_float(q.w);
    }
}

// ---- The separable passes: ONE body per pass, two compile-time policies --------------------------------------------------------
// Along an axis the output is  out = fmaf(B[s0 + 1], f, B[s0] * (1 - f)).  Away from the border the two Gaussian sums share their
// pixels: pixel j (0 .. ksize) of the run that starts at s0 - r contributes g[j] * p to B[s0] (j < ksize) and g[j - 1] * p to
// B[s0 + 1] (j >= 1), and each sum is ONE chain of fused multiply-adds in increasing j.  That order is the whole bit contract: every
// form below (fused == two-pass, u8 values == u8 bits at every depth) keeps it, whichever policies it picks.
//   Px    where pixel j of the thread's four rows comes from: PxBytes (u8: aligned dwords re-aligned with v_alignbyte, from staged
//         LDS rows or from global memory) or PxElems (one addressable element per pixel: uint16 / float staged rows, any depth from
//         global memory)
//   Taps  how a pixel is accumulated: TapsScalar (two scalar fmaf, g[] from the kernel argument) or TapsPairs (one packed fma of the
//         pair (g[j], g[j - 1]) with (p, p); the pairs sit in LDS -- stage_tap_pairs -- or in registers -- TapPairs<KS>)
// KS > 0: ksize known at compile time (the loops unroll: all loads of a thread issue together); KS == 0: a loop over ksize.
typedef float mav_f2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ int tap_pairs_padded(int ksize) { return (ksize + 1 + 3) & ~3; }

// word(k, i) = aligned dword i of the byte stream of the thread's k-th row; the row's pixel 0 is byte sh[k] of dword 0.  Pixels
// 4c .. 4c + 3 need dwords c and c + 1, so the stream reads one dword past the last pixel's: staged rows carry a word of slack for
// that (tile_columns, staged_pitch_words), and a word function over global memory returns 0 for dwords that hold no needed byte
// instead of reading them.
template <typename WordFn> struct PxBytes {
    static constexpr int STEP = 4;                       // pixels per advance()
    static constexpr bool whole_words = true;            // pixels past ksize are bytes like any other: finite, free to meet a zero tap
    WordFn word;
    unsigned sh[4];
    uint32_t lo[4], cur[4];
    __device__ __forceinline__ void begin()
    {
#pragma unroll
        for (int k = 0; k < 4; k++) lo[k] = word(k, 0);
    }
    __device__ __forceinline__ void advance(int c)
    {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t hi = word(k, c + 1);
            cur[k] = __builtin_amdgcn_alignbyte(hi, lo[k], sh[k]);
            lo[k] = hi;
        }
    }
    __device__ __forceinline__ float get(int k, int c, int b) const { return (float)((cur[k] >> (8 * b)) & 0xffu); }
};
template <typename WordFn>
static __device__ __forceinline__ PxBytes<WordFn> px_bytes(WordFn word, unsigned s0, unsigned s1, unsigned s2, unsigned s3)
{
    return PxBytes<WordFn>{word, {s0, s1, s2, s3}, {}, {}};
}
// four rows staged in LDS by stage_rows (or the fast tile's own loop): row(k) = first dword of the thread's k-th row, off = byte
// offset of the thread's pixel 0 in it
template <typename RowFn>
static __device__ __forceinline__ auto px_staged_bytes(RowFn row, int off)
{
    const int w0 = off >> 2;
    const unsigned sh = (unsigned)(off & 3);
    return px_bytes([=](int k, int i) { return row(k)[w0 + i]; }, sh, sh, sh, sh);
}
// elem(k, j) = pixel j of the thread's k-th row, already a float.  Nothing past pixel ksize is ever read (a float frame's staging
// slack is unwritten LDS and may hold NaN).
template <typename ElemFn> struct PxElems {
    static constexpr int STEP = 1;
    static constexpr bool whole_words = false;
    ElemFn elem;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void advance(int) {}
    __device__ __forceinline__ float get(int k, int c, int) const { return elem(k, c); }
};
template <typename ElemFn> static __device__ __forceinline__ PxElems<ElemFn> px_elems(ElemFn elem) { return PxElems<ElemFn>{elem}; }

// g[] behind the kernel argument: wave-uniform scalar loads, a tap serves both sums (B[s0] with the pixel before, B[s0 + 1] with this one)
struct TapsScalar {
    static constexpr bool zero_padded = false;
    struct Acc { float b0, b1, prev; };
    typedef float Tap;
    const float* g;
    __device__ __forceinline__ Tap tap(int j) const { return j > 0 ? g[j - 1] : 0.f; }
    __device__ __forceinline__ void add(Acc& a, Tap t, int j, float p) const
    {
        if (j > 0) { a.b0 = fmaf(t, a.prev, a.b0); a.b1 = fmaf(t, p, a.b1); }
        a.prev = p;
    }
    static __device__ __forceinline__ float b0(const Acc& a) { return a.b0; }
    static __device__ __forceinline__ float b1(const Acc& a) { return a.b1; }
};
// The (B[s0], B[s0 + 1]) accumulators of ONE row as a packed pair: pixel j costs one conversion and one v_pk_fma_f32 with
// pair(j) = (g[j], g[j - 1]), where pair(0) = (g[0], 0) and pair(ksize) = (0, g[ksize - 1]).  ZERO_PADDED: pair(j) is (0, 0) from
// ksize + 1 up to tap_pairs_padded(ksize), so a byte stream may run to the end of its last word -- a fused multiply-add with a zero
// tap returns its accumulator unchanged (pixels are finite, the accumulators start at +0).
template <typename PairFn, bool ZERO_PADDED> struct TapsPairs {
    static constexpr bool zero_padded = ZERO_PADDED;
    typedef mav_f2 Acc;
    typedef mav_f2 Tap;
    PairFn pair;
    __device__ __forceinline__ Tap tap(int j) const { return pair(j); }
    __device__ __forceinline__ void add(Acc& a, Tap t, int, float p) const { a = __builtin_elementwise_fma(t, (mav_f2)(p, p), a); }
    static __device__ __forceinline__ float b0(const Acc& a) { return a.x; }
    static __device__ __forceinline__ float b1(const Acc& a) { return a.y; }
};
// the pairs in LDS (the two-pass kernel: long Gaussians, one broadcast ds_read_b64 per tap for all four rows), padded with zeros
static __device__ __forceinline__ void stage_tap_pairs(const BlurParams& bp, mav_f2* __restrict__ G2)
{
    const int n = tap_pairs_padded(bp.ksize);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        mav_f2 v;
        v.x = t < bp.ksize ? bp.g[t] : 0.f;
        v.y = (t >= 1 && t <= bp.ksize) ? bp.g[t - 1] : 0.f;
        G2[t] = v;
    }
}
static __device__ __forceinline__ auto taps_lds_pairs(const mav_f2* __restrict__ G2)
{
    auto pair = [=](int j) { return G2[j]; };
    return TapsPairs<decltype(pair), true>{pair};
}
// the pairs in registers, for a Gaussian whose length is a template argument (the fused fast tile: 13 taps)
template <int KS> struct TapPairs {
    mav_f2 G[KS + 1];
    __device__ __forceinline__ void load(const BlurParams& bp)
    {
#pragma unroll
        for (int t = 0; t <= KS; t++) { G[t].x = t < KS ? bp.g[t] : 0.f; G[t].y = t >= 1 ? bp.g[t - 1] : 0.f; }
    }
    __device__ __forceinline__ auto taps() const
    {
        auto pair = [this](int j) { return G[j]; };
        return TapsPairs<decltype(pair), false>{pair};
    }
};

// Horizontal pass of the thread's four rows, interior form (the rows' ksize + 1 pixels are all there: inside the image, or staged
// with their BORDER_REFLECT_101 pixels in place).
template <int KS, class Px, class Taps>
static __device__ __forceinline__ void blur_h4_run(Px px, const Taps& taps, int ksize, float f, float out[4])
{
    // pixels to visit: 0 .. ksize, or whole words of them where both policies allow it (no bounds test per byte in the long loops)
    const int n = KS > 0 ? KS + 1 : (Px::whole_words && Taps::zero_padded ? tap_pairs_padded(ksize) : ksize + 1);
    typename Taps::Acc acc[4] = {};
    px.begin();
    auto step = [&](int c) {
        px.advance(c);
#pragma unroll
        for (int b = 0; b < Px::STEP; b++) {
            const int j = Px::STEP * c + b;
            if (!(Px::whole_words && Taps::zero_padded) && j >= n) break;       // (n is whole words where both hold)
            const typename Taps::Tap t = taps.tap(j);
#pragma unroll
            for (int k = 0; k < 4; k++) taps.add(acc[k], t, j, px.get(k, c, b));
        }
    };
    if constexpr (KS > 0) {
#pragma unroll
        for (int c = 0; Px::STEP * c < KS + 1; c++) step(c);
    } else {
        for (int c = 0; Px::STEP * c < n; c++) step(c);
    }
    const float a0 = 1.f - f;
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = fmaf(Taps::b1(acc[k]), f, Taps::b0(acc[k]) * a0);
}
// scalar taps, ksize dispatched at run time: 5 (the reference's preset: layer 1, scale 0.4, sigma 0.75) and 13 unroll
template <class Px>
static __device__ __forceinline__ void blur_h4_scalar(Px px, float f, const BlurParams& bp, float out[4])
{
    const TapsScalar taps{bp.g};
    if (bp.ksize == 5) blur_h4_run<5>(px, taps, 5, f, out);
    else if (bp.ksize == 13) blur_h4_run<13>(px, taps, 13, f, out);
    else blur_h4_run<0>(px, taps, bp.ksize, f, out);
}

// Horizontal pass at destination column (s0, f) for the four source rows y0 .. y0 + 3 (clamped to the image) read from GLOBAL memory:
// the unstaged fused tile (u8 frames whose rows are not quad-addressable behind 13 taps) and the direct kernel (ksize >= 123).
template <typename T>
static __device__ __forceinline__ void blur_h4(const T* __restrict__ base, int W, int H, int y0, int s0, float f,
                                               const BlurParams& bp, float out[4])
{
    const int r = bp.ksize >> 1;
    const T* rows[4];
#pragma unroll
    for (int k = 0; k < 4; k++) rows[k] = base + (size_t)min(y0 + k, H - 1) * W;
    if (s0 - r >= 0 && s0 + 1 + r < W) {               // interior: B[s0+1] re-uses B[s0]'s pixels shifted by one
        const TapsScalar taps{bp.g};
        if constexpr (sizeof(T) > 1) {                     // one aligned element load per pixel
            blur_h4_run<0>(px_elems([&](int k, int j) { return (float)rows[k][s0 - r + j]; }), taps, bp.ksize, f, out);
        } else {
            // the ksize + 1 consecutive bytes of a row come as ALIGNED dwords -- a quarter of the load instructions.  Only words
            // that hold a needed byte are read (an aligned dword never crosses a page, so nothing unmapped is touched).
            const uint32_t* wp[4];
            unsigned sh[4];
            int last[4];                                     // the needed bytes sit at positions sh .. sh + ksize of the word stream
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uintptr_t a = (uintptr_t)(rows[k] + (s0 - r));
                wp[k] = (const uint32_t*)(a & ~(uintptr_t)3);
                sh[k] = (unsigned)(a & 3);
                last[k] = ((int)sh[k] + bp.ksize) / 4;
            }
            blur_h4_run<0>(px_bytes([&](int k, int i) { return i <= last[k] ? wp[k][i] : 0u; }, sh[0], sh[1], sh[2], sh[3]), taps,
                           bp.ksize, f, out);
        }
        return;
    }
    // border: the columns of B[s0] and of B[s0 + 1] reflect separately and share no pixels
    const int s1 = s0 + 1 < W ? s0 + 1 : s0;
    float b0[4] = {0.f, 0.f, 0.f, 0.f}, b1[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < bp.ksize; t++) {
        const float g = bp.g[t];
        const int c0 = reflect101d(s0 - r + t, W), c1 = reflect101d(s1 - r + t, W);
#pragma unroll
        for (int k = 0; k < 4; k++) { b0[k] = fmaf(g, (float)rows[k][c0], b0[k]); b1[k] = fmaf(g, (float)rows[k][c1], b1[k]); }
    }
    const float a0 = 1.f - f;
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = fmaf(b1[k], f, b0[k] * a0);
}

// Source rows [y0, y0 + n_rows) (row index clamped to the image), pixel columns [xb, xb + 4 words) of one image -> LDS, row pitch
// pitch_w quads (u8: dwords); xb is a multiple of 4 (possibly negative).  Columns outside the image hold their BORDER_REFLECT_101 pixels.
// Quad-addressable rows: coalesced quad loads (dword / dwordx2 / dwordx4); frames whose width is no multiple of 4: pixel by pixel.
template <typename T, int NB = 8>      // NB loads of a thread in flight before the first LDS store
static __device__ __forceinline__ void stage_rows(const T* __restrict__ base, int W, int H, int y0, int n_rows, int xb, int words,
                                                  bool dword_ok, uint32_t* __restrict__ sw, int pitch_w)
{
    typedef typename QuadOf<T>::type Q;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T* sb = (T*)sw;
    Q* sq = (Q*)sw;
    if (dword_ok) {
        // words inside the image as dwords (xb and W are multiples of 4); the few columns outside it byte by byte, reflected.
        // A wave's (row, 64-word chunk) items go eight at a time: eight independent loads in flight, then eight LDS stores (a plain
        // load -> store loop serialises one memory round trip per row: 11 of them per wave for the preset's layer 1).
        const int wlo = xb < 0 ? (-xb) >> 2 : 0, whi = min(words, (W - xb) >> 2);
        const int n_left = 4 * wlo, n_out = n_left + 4 * max(words - whi, 0);
        const int n_chunks = (whi - wlo + 63) >> 6, rows_w = n_rows > wv ? (n_rows - wv + 3) >> 2 : 0;
        const int n_items = rows_w * n_chunks;
        for (int it0 = 0; it0 < n_items; it0 += NB) {
            Q v[NB];
            int dst[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int it = it0 + u;
                const int ri = n_chunks == 1 ? it : it / n_chunks, ch = it - ri * n_chunks;
                const int row = wv + 4 * ri, wd = wlo + 64 * ch + lane;
                const bool ok = it < n_items && wd < whi;
                dst[u] = ok ? row * pitch_w + wd : -1;
                const Q* g = (const Q*)(base + (size_t)min(y0 + (ok ? row : 0), H - 1) * W + xb);
                v[u] = g[ok ? wd : wlo];
            }
#pragma unroll
            for (int u = 0; u < NB; u++)
                if (dst[u] >= 0) sq[dst[u]] = v[u];
        }
        if (n_out > 0)
            for (int row = wv; row < n_rows; row += 4) {
                const T* p = base + (size_t)min(y0 + row, H - 1) * W;
                for (int j = lane; j < n_out; j += 64) {
                    const int col = j < n_left ? j : 4 * whi + (j - n_left);
                    sb[row * pitch_w * 4 + col] = p[reflect101d(xb + col, W)];
                }
            }
    } else {
        for (int row = wv; row < n_rows; row += 4) {
            const T* p = base + (size_t)min(y0 + row, H - 1) * W;
            for (int j = lane; j < 4 * words; j += 64) sb[row * pitch_w * 4 + j] = p[reflect101d(xb + j, W)];
        }
    }
}
// the source columns the 64 destination columns from dx0 on need: first staged byte column (multiple of 4) and dwords per row.
// s0 = this lane's source column (lane = destination column dx0 + lane, clamped to w - 1): the tile's first and last source
// columns are lane 0's and lane 63's, read across the wave instead of evaluating resize_coord (double arithmetic) twice more.
static __device__ __forceinline__ void tile_columns(int s0, const BlurParams& bp, int* xb, int* words)
{
    const int c0 = __builtin_amdgcn_readlane(s0, 0), c1 = __builtin_amdgcn_readlane(s0, 63);
    const int r = bp.ksize >> 1;
    *xb = (c0 - r) & ~3;
    *words = ((c1 + 1 + r - *xb) >> 2) + 2;                  // + 1: PxBytes reads one word ahead
}

// Vertical pass, interior form, of one column: row(j) = the horizontal pass's value at source row (s0 - r) + j of this thread's
// column, j = 0 .. ksize.  The same chains in the same order as blur_h4_run, with the same Taps policies.
template <int KS, typename RowFn, class Taps>
static __device__ __forceinline__ float blur_v1_run(RowFn row, const Taps& taps, int ksize, float f)
{
    typename Taps::Acc acc = {};
    if constexpr (KS > 0) {                                // the KS + 1 rows of the thread requested together
        float px[KS + 1];
#pragma unroll
        for (int j = 0; j <= KS; j++) px[j] = row(j);
#pragma unroll
        for (int j = 0; j <= KS; j++) taps.add(acc, taps.tap(j), j, px[j]);
    } else {
#pragma unroll 8
        for (int j = 0; j <= ksize; j++) taps.add(acc, taps.tap(j), j, row(j));
    }
    return fmaf(Taps::b1(acc), f, Taps::b0(acc) * (1.f - f));
}
// Vertical pass at destination row (s0, f): row(y) = the horizontal pass's value at source row y of this thread's column.
template <typename RowFn>
static __device__ __forceinline__ float blur_v1(RowFn row, int H, int s0, float f, const BlurParams& bp)
{
    const int r = bp.ksize >> 1;
    if (s0 - r >= 0 && s0 + 1 + r < H) {
        const TapsScalar taps{bp.g};
        auto at = [&](int j) { return row(s0 - r + j); };
        return bp.ksize == 5 ? blur_v1_run<5>(at, taps, 5, f) : blur_v1_run<0>(at, taps, bp.ksize, f);
    }
    // border: the rows of B[s0] and of B[s0 + 1] reflect separately
    const int s1 = s0 + 1 < H ? s0 + 1 : s0;
    float b0 = 0.f, b1 = 0.f;
    for (int t = 0; t < bp.ksize; t++) {
        const float g = bp.g[t];
        b0 = fmaf(g, row(reflect101d(s0 - r + t, H)), b0);
        b1 = fmaf(g, row(reflect101d(s1 - r + t, H)), b1);
    }
    return fmaf(b1, f, b0 * (1.f - f));
}

// direct form (no LDS): every thread walks its own bytes in global memory.  Fallback for scales whose staged rows would not fit LDS.
template <typename T>
__global__ __launch_bounds__(256) void k_blur_resize_h_direct(const T* __restrict__ img, const T* __restrict__ img2, int split,
                                                              size_t img_stride, int W, int H, int w, BlurParams bp,
                                                              float* __restrict__ tmp, size_t tmp_stride)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 4;
    if (dx >= w || y0 >= H) return;
    const T* base = image_of(img, img2, split, img_stride, blockIdx.z);
    int s0; float f;
    resize_coord(dx, W, w, bp.scale_x, &s0, &f);
    float o[4];
    blur_h4(base, W, H, y0, s0, f, bp, o);
    float* dst = tmp + (size_t)blockIdx.z * tmp_stride + dx;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (y0 + k < H) dst[(size_t)(y0 + k) * w] = o[k];
}
// Staged form: a workgroup owns 64 destination columns x rows_blk source rows; the u8 bytes those need go through LDS once
// (coalesced dword loads; a thread of the direct form issues (ksize + 1) / 4 dependent dword loads per row from an address of its
// own -- 24 round trips for the 95-tap layer of the 4K preset -- and neighbouring lanes re-read each other's bytes).
template <typename T>
__global__ __launch_bounds__(256) void k_blur_resize_h(const T* __restrict__ img, const T* __restrict__ img2, int split,
                                                       size_t img_stride, int W, int H, int w, BlurParams bp,
                                                       float* __restrict__ tmp, size_t tmp_stride, int rows_blk, int pitch_w, int dword_ok)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t srows[];         // [rows_blk][pitch_w] quads, then the tap pairs (stage_tap_pairs)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int dx0 = blockIdx.x * 64;
    const T* base = image_of(img, img2, split, img_stride, blockIdx.z);
    const int dx = dx0 + lane;
    mav_f2* G2 = (mav_f2*)(srows + ((rows_blk * pitch_w * (int)sizeof(T) + 1) & ~1));
    stage_tap_pairs(bp, G2);                                                 // (visible after the first barrier below)
    int s0; float f;
    if (bp.xs) { s0 = bp.xs[min(dx, w - 1)]; f = bp.xf[min(dx, w - 1)]; }
    else resize_coord(min(dx, w - 1), W, w, bp.scale_x, &s0, &f);
    int xb, words;
    tile_columns(s0, bp, &xb, &words);
    const int off = s0 - (bp.ksize >> 1) - xb;
    float* dst = tmp + (size_t)blockIdx.z * tmp_stride + dx;
    // a workgroup walks every gridDim.y-th block of rows (the launcher gives every block its own workgroup)
    for (int yb = blockIdx.y; yb * rows_blk < H; yb += gridDim.y) {
        const int y0 = yb * rows_blk;
        const int n_rows = min(rows_blk, H - y0);
        if (yb != (int)blockIdx.y) __syncthreads();             // everybody has finished reading the previous block's rows
        // (24 instead of 8 staging loads in flight per thread: 161 / 175 vs 129 / 169 us per launch -- the registers cost occupancy)
        stage_rows(base, W, H, y0, n_rows, xb, min(words, pitch_w), dword_ok != 0, srows, pitch_w);
        __syncthreads();
        for (int i = wv * 4; i < n_rows; i += 16) {
            float o[4];
            // (rows past n_rows clamp to the last one; their results are not stored)
            if constexpr (sizeof(T) == 1)
                blur_h4_run<0>(px_staged_bytes([&](int k) { return srows + min(i + k, n_rows - 1) * pitch_w; }, off), taps_lds_pairs(G2),
                               bp.ksize, f, o);
            else
                blur_h4_run<0>(px_elems([&](int k, int j) { return (float)((const T*)srows)[(min(i + k, n_rows - 1) * pitch_w) * 4 + off + j]; }),
                               taps_lds_pairs(G2), bp.ksize, f, o);
            if (dx < w) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i + k < n_rows) dst[(size_t)(y0 + i + k) * w] = o[k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_blur_resize_v(const float* __restrict__ tmp, size_t tmp_stride, int H, int w, int h,
                                                       BlurParams bp, float* __restrict__ out, size_t out_stride)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= w || dy >= h) return;
    const float* src = tmp + (size_t)blockIdx.z * tmp_stride + dx;
    int s0; float f;
    resize_coord(dy, H, h, bp.scale_y, &s0, &f);
    out[(size_t)blockIdx.z * out_stride + (size_t)dy * w + dx] = blur_v1([&](int y) { return src[(size_t)y * w]; }, H, s0, f, bp);
}

// Both passes in ONE kernel for the layers whose Gaussian is short (ksize <= 13: layer 1 of the reference's preset, layers 1 - 2
// of the 4K / 5-layer one): a workgroup owns a 64 x FB_TH tile of the layer, runs the horizontal pass over the source rows the
// tile's vertical pass will read -- [s0(first row) - r, s0(last row) + 1 + r] clamped to the image; a reflected row index always
// falls inside that range -- into LDS (rows x 64 f32), and filters / resamples vertically from there.  The H x w f32 scratch of
// the two-pass form (written once, read ~(ksize + 1) h / H times: 2.95x the stage's algorithmic bytes) never exists.  Same
// functions, same tap order: bit-identical to the two-pass form (tests/test_gpu_flow.py).  The rows two vertically adjacent
// tiles share (2r + 1 of ~40 at scale 0.4) are filtered twice.
#define FB_TH 16
// pitch_w > 0: the tile's u8 source region (rows [ylo, yhi], the columns its 64 destination columns need) goes through LDS first
// (stage_rows: ~7 coalesced dword loads per thread instead of ~70 single-byte loads) and the horizontal pass reads it from there;
// pitch_w == 0 (regions too large for LDS): every thread reads its bytes from global memory.
// one 64 x FB_TH tile of one image: base = the u8 frame, out = the layer image of that frame
template <typename T>
static __device__ __forceinline__ void blur_fused_tile(const T* __restrict__ base, float* __restrict__ out, int W, int H, int w, int h,
                                                       const BlurParams& bp, int rows_cap, int pitch_w, int dword_ok, int tile_x, int tile_y,
                                                       float* __restrict__ hrows)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // (Measured and not kept: a 1-D grid in tile_of_block's XCD-aware order, so that the 128-byte lines horizontally adjacent tiles
    // share are re-read from one XCD's L2 -- 72.0 vs 69.6 us per launch; workgroups that walk 4 - 8 tiles -- 104 vs 72 us.  PMC says
    // why: the kernel issues ~1000 VALU instructions per wave, index arithmetic and double-precision resize coordinates as much as
    // filter taps, so it is instruction-bound.  Hence: the tile's first / last source column come from lanes 0 / 63 of the wave's own
    // coordinates, and the 16 destination rows' source coordinates are evaluated once per wave, by lanes 0 - 15.)
    const int dx0 = tile_x * 64;
    const int dx = dx0 + lane, dxc = min(dx, w - 1);
    const int r = bp.ksize >> 1;
    int s0; float f;
    resize_coord(dxc, W, w, bp.scale_x, &s0, &f);
    int xb, words;
    tile_columns(s0, bp, &xb, &words);
    const int off = s0 - r - xb;
    uint32_t* sw = (uint32_t*)(hrows + rows_cap * 64);
    const int dy0 = tile_y * FB_TH, dy1 = min(dy0 + FB_TH, h) - 1;
    int row_s; float row_f;                                              // lane L < 16: source row / weight of destination row dy0 + L
    resize_coord(min(dy0 + (lane & (FB_TH - 1)), h - 1), H, h, bp.scale_y, &row_s, &row_f);
    const int sa = __builtin_amdgcn_readlane(row_s, 0), sb = __builtin_amdgcn_readlane(row_s, FB_TH - 1);    // (rows past h - 1 clamp to it)
    const int ylo = max(sa - r, 0), yhi = min(sb + 1 + r, H - 1);
    const int n_rows = min(yhi - ylo + 1, rows_cap);                      // (the host sized rows_cap for the worst tile)
    if (pitch_w > 0) {
        stage_rows(base, W, H, ylo, n_rows, xb, min(words, pitch_w), dword_ok != 0, sw, pitch_w);
        __syncthreads();
        for (int i = wv * 4; i < n_rows; i += 16) {
            float o[4];
            if constexpr (sizeof(T) == 1)
                blur_h4_scalar(px_staged_bytes([&](int k) { return sw + min(i + k, n_rows - 1) * pitch_w; }, off), f, bp, o);
            else
                blur_h4_scalar(px_elems([&](int k, int j) { return (float)((const T*)sw)[(min(i + k, n_rows - 1) * pitch_w) * 4 + off + j]; }), f, bp, o);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k < n_rows) hrows[(i + k) * 64 + lane] = o[k];
        }
    } else {
        for (int i = wv * 4; i < n_rows; i += 16) {
            float o[4];
            blur_h4(base, W, H, ylo + i, s0, f, bp, o);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k < n_rows) hrows[(i + k) * 64 + lane] = o[k];
        }
    }
    __syncthreads();
    const float* col = hrows + lane - ylo * 64;
#pragma unroll
    for (int j = 0; j < FB_TH / 4; j++) {
        const int dy = dy0 + j * 4 + wv;                                  // wave-uniform
        if (dy > dy1) break;
        const int t0 = __builtin_amdgcn_readlane(row_s, j * 4 + wv);
        const float tf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row_f), j * 4 + wv));
        const float v = blur_v1([&](int y) { return col[y * 64]; }, H, t0, tf, bp);
        if (dx < w) out[(size_t)dy * w + dx] = v;
    }
}

// The fused tile again, for the cases that carry the load (ksize 5 and 13 -- layer 1 of the reference's preset, layers 1 - 2 of the
// 4K / 5-layer one; dword-addressable frames; coordinate tables present): same H-pass / V-pass functions on the same values as
// blur_fused_tile, hence the same bits, with the bookkeeping around them cut down -- round 3's form issued ~1000 VALU + ~520 SALU
// instructions per wave for ~190 filter FMAs per thread:
//   * the resize coordinates come from the layer's tables (bp.xs / xf / ys / yf) instead of double-precision arithmetic per thread;
//   * KS is a template argument of the WHOLE tile (no run-time dispatch inside the loops; the V pass unrolls for 13 taps too);
//   * staging: a wave owns rows wv, wv + 4, ...; row addresses are wave-uniform (scalar), a lane adds its word offset; six rows'
//     loads in flight; every staged row lies inside the image (ylo + row <= yhi <= H - 1), so no clamping;
//   * the H pass does not clamp its row index: rows past n_rows (at most 3, LDS the launch allocates) are computed and not stored;
//   * interior tiles (every row's taps inside the image) take a V pass without the reflect-101 tests.
// Taps: scalar for 5, register pairs for 13 -- the pair form pays for 13 taps (184 vs 194 us per launch for layer 2 of the 4K preset)
// and costs for 5 (64 vs 53 us per launch for layer 1 at 1080p, where the compiler's own mix of scalar-tap FMAs is shorter).
// 13 taps: u8 frames only (fused_fast_ok).
template <typename T, int KS, int TH>
static __device__ __forceinline__ void blur_fused_tile_fast(const T* __restrict__ base, float* __restrict__ out, int W, int H, int w, int h,
                                                            const BlurParams& bp, int rows_cap, int pitch_w, int tile_x, int tile_y,
                                                            float* __restrict__ hrows)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int r = KS >> 1;
    static_assert(KS == 5 || (KS == 13 && sizeof(T) == 1), "the fast tiles the dispatch selects");
    TapPairs<KS> tp;
    if constexpr (KS >= 13) tp.load(bp);
    const auto taps = [&] { if constexpr (KS >= 13) return tp.taps(); else return TapsScalar{bp.g}; }();
    const int dx = tile_x * 64 + lane, dxc = min(dx, w - 1);
    const int dy0 = tile_y * TH, dy1 = min(dy0 + TH, h) - 1;
    const int dyc = min(dy0 + (lane & (TH - 1)), h - 1);
    const int s0 = bp.xs[dxc];
    const float f = bp.xf[dxc];
    const int row_s = bp.ys[dyc];                                           // lane L < TH: source row / weight of destination row dy0 + L
    const float row_f = bp.yf[dyc];
    int xb, words;
    tile_columns(s0, bp, &xb, &words);
    words = min(words, pitch_w);
    const int off = s0 - r - xb;
    uint32_t* sw = (uint32_t*)(hrows + rows_cap * 64);
    const int sa = __builtin_amdgcn_readlane(row_s, 0), sb = __builtin_amdgcn_readlane(row_s, TH - 1);
    const int ylo = max(sa - r, 0), yhi = min(sb + 1 + r, H - 1);
    const int n_rows = min(yhi - ylo + 1, rows_cap);
    // ---- stage the source rows [ylo, ylo + n_rows), pixel columns [xb, xb + 4 words)
    {
        typedef typename QuadOf<T>::type Q;
        const int wlo = xb < 0 ? (-xb) >> 2 : 0, whi = min(words, (W - xb) >> 2);
        const int nw = whi - wlo;                                            // quads of a row that lie inside the image
        const T* g0 = base + (size_t)ylo * W + (xb + 4 * wlo);               // wave-uniform
        Q* s00 = (Q*)sw + wlo;
        for (int c0 = 0; c0 < nw; c0 += 64) {
            const int wd = c0 + lane;
            const bool ok = wd < nw;
            const unsigned lo = 4u * (unsigned)(ok ? wd : 0);
            for (int row0 = wv; row0 < n_rows; row0 += 24) {
                Q v[6];
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    const int row = min(row0 + 4 * u, n_rows - 1);           // (wave-uniform)
                    v[u] = *(const Q*)(g0 + ((unsigned)(row * W) + lo));
                }
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    const int row = row0 + 4 * u;
                    if (ok && row < n_rows) s00[row * pitch_w + wd] = v[u];
                }
            }
        }
        const int n_left = 4 * wlo, n_out = n_left + 4 * max(words - whi, 0);
        if (n_out > 0) {                                                     // the few columns outside the image, reflected, pixel by pixel
            T* sb8 = (T*)sw;
            for (int row = wv; row < n_rows; row += 4) {
                const T* p = base + (size_t)(ylo + row) * W;
                for (int j = lane; j < n_out; j += 64) {
                    const int col = j < n_left ? j : 4 * whi + (j - n_left);
                    sb8[row * pitch_w * 4 + col] = p[reflect101d(xb + col, W)];
                }
            }
        }
    }
    __syncthreads();
    // ---- horizontal pass: staged bytes -> hrows (n_rows x 64 f32)
    for (int i = wv * 4; i < n_rows; i += 16) {
        float o[4];
        if constexpr (sizeof(T) > 1) {
            const T* re = (const T*)sw + i * pitch_w * 4 + off;
            blur_h4_run<KS>(px_elems([&](int k, int j) { return (float)re[k * pitch_w * 4 + j]; }), taps, KS, f, o);
        } else {
            const uint32_t* rw = sw + i * pitch_w;
            blur_h4_run<KS>(px_staged_bytes([&](int k) { return rw + k * pitch_w; }, off), taps, KS, f, o);
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k < n_rows) hrows[(i + k) * 64 + lane] = o[k];
    }
    __syncthreads();
    // ---- vertical pass
    const float* col = hrows + lane - ylo * 64;
    const bool interior = sa - r >= 0 && sb + 1 + r < H;                    // wave-uniform: no row of the tile touches the border
#pragma unroll
    for (int j = 0; j < TH / 4; j++) {
        const int dy = dy0 + j * 4 + wv;                                     // wave-uniform
        if (dy > dy1) break;
        const int t0 = __builtin_amdgcn_readlane(row_s, j * 4 + wv);
        const float tf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row_f), j * 4 + wv));
        const float v = interior ? blur_v1_run<KS>([&](int t) { return col[(t0 - r + t) * 64]; }, taps, KS, tf)
                                 : blur_v1([&](int y) { return col[y * 64]; }, H, t0, tf, bp);
        if (dx < w) out[(size_t)dy * w + dx] = v;
    }
}
// does a fused layer take the fast tile?  Quad-addressable frames, staged form, tables, and 5 taps (any depth) or 13 taps (u8 only:
// blur_resize_is_fused refuses every 13-tap layer of wider pixels, whose staged 64 x 16 region is past 64 KB from 1 / scale = 5.6 on)
static __host__ __device__ __forceinline__ bool fused_fast_ok(const BlurParams& bp, int pitch_w, int dword_ok, int esize)
{
    return dword_ok && pitch_w > 0 && bp.xs != nullptr && (bp.ksize == 5 || (bp.ksize == 13 && esize == 1));
}
// Which tile code a fused launch carries.  One kernel per PATH: the paths differ a lot in registers (the generic tile and the 13-tap
// pair form want ~80 VGPRs, the 5-tap fast tile 44), and a kernel that contained them all ran the 5-tap layers at the occupancy of
// the hungriest (66 vs 53 us per launch for layer 1 at 1080p).
enum { FP_GENERIC = 0, FP_FAST5 = 1, FP_FAST13 = 2, FP_ANY = 3 };
static int fused_path_of(const BlurParams& bp, int pitch_w, int dword_ok, int esize)
{
    return !fused_fast_ok(bp, pitch_w, dword_ok, esize) ? FP_GENERIC : (bp.ksize == 5 ? FP_FAST5 : FP_FAST13);
}
// go(integral_constant<int, PATH>) for a run-time path: the one place that turns a path into a kernel instantiation.  FP_FAST13
// exists for u8 frames only (fused_path_of never names it for another depth); path < 0 (a launch without a fused job): any kernel.
template <typename T, typename Go>
static void with_fused_path(int path, Go go)
{
    switch (path) {
    case FP_GENERIC: go(std::integral_constant<int, FP_GENERIC>()); break;
    case FP_ANY: go(std::integral_constant<int, FP_ANY>()); break;
    case FP_FAST13:
        if constexpr (sizeof(T) == 1) go(std::integral_constant<int, FP_FAST13>());
        break;
    default: go(std::integral_constant<int, FP_FAST5>()); break;
    }
}
template <typename T, int PATH>
static __device__ __forceinline__ void blur_fused_any(const T* __restrict__ base, float* __restrict__ out, int W, int H, int w, int h,
                                                      const BlurParams& bp, int rows_cap, int pitch_w, int dword_ok, int th, int tile_x, int tile_y,
                                                      float* __restrict__ hrows)
{
    // th = tile height chosen by the host (fused_plan): 16, or 8 where 16 rows' source region does not fit LDS (13 taps only)
    static_assert(PATH != FP_FAST13 || sizeof(T) == 1, "the 13-tap fast tile is a u8 form");
    const bool fast = PATH == FP_FAST5 || PATH == FP_FAST13 || (PATH == FP_ANY && fused_fast_ok(bp, pitch_w, dword_ok, (int)sizeof(T)));
    if ((PATH == FP_FAST5 || PATH == FP_ANY) && fast && bp.ksize == 5) {
        blur_fused_tile_fast<T, 5, 16>(base, out, W, H, w, h, bp, rows_cap, pitch_w, tile_x, tile_y, hrows);
        return;
    }
    if constexpr (sizeof(T) == 1 && (PATH == FP_FAST13 || PATH == FP_ANY)) {
        if (fast && bp.ksize == 13) {
            if (th == 16) blur_fused_tile_fast<T, 13, 16>(base, out, W, H, w, h, bp, rows_cap, pitch_w, tile_x, tile_y, hrows);
            else blur_fused_tile_fast<T, 13, 8>(base, out, W, H, w, h, bp, rows_cap, pitch_w, tile_x, tile_y, hrows);
            return;
        }
    }
    if (PATH == FP_GENERIC || PATH == FP_ANY)
        blur_fused_tile(base, out, W, H, w, h, bp, rows_cap, pitch_w, dword_ok, tile_x, tile_y, hrows);
}
template <typename T, int PATH>
__global__ __launch_bounds__(256) void k_blur_resize_fused(const T* __restrict__ img, const T* __restrict__ img2, int split,
                                                           size_t img_stride, int W, int H, int w, int h, BlurParams bp,
                                                           float* __restrict__ out, size_t out_stride, int rows_cap, int pitch_w, int dword_ok, int th)
{
    extern __shared__ __attribute__((aligned(16))) float hrows[];       // [rows_cap][64] f32, then [rows_cap + 3][pitch_w] quads of T
    blur_fused_any<T, PATH>(image_of(img, img2, split, img_stride, blockIdx.z), out + (size_t)blockIdx.z * out_stride, W, H, w, h, bp, rows_cap,
                         pitch_w, dword_ok, th, blockIdx.x, blockIdx.y, hrows);
}

static int fused_blur_rows(int H, int h, int ksize, int th = FB_TH) { return (int)((th - 1) * ((double)H / h)) + (ksize | 1) + 4; }
// LDS of a fused tile: rows x 64 f32 of horizontal-pass results, then the staged rows of esize-byte pixels (three rows of slack: the
// fast tile's horizontal pass works on whole groups of four rows)
static size_t fused_lds_bytes(int rows, int pitch_w, int esize = 1) { return (size_t)rows * 256 + (size_t)(rows + 3) * 4 * pitch_w * esize; }
// quads per staged source row: the columns 64 destination pixels need (63 scale + 1 + ksize), the 4-alignment slack and the quad
// PxBytes reads ahead
static int staged_pitch_words(int W, int w, int ksize) { return ((int)(63 * ((double)W / w)) + (ksize | 1) + 2 + 3) / 4 + 3; }
// How a fused layer's tiles are cut: 64 x 16 with the source region staged in LDS when that fits 64 KB; else, for the 13-tap fast
// tile, 64 x 8 staged (layer 2 of the 4K / 5-layer preset: 13 taps at scale 6.25 -- 110 source rows of 420 bytes for 16 destination
// rows); else 64 x 16 unstaged (every thread reads its bytes from global memory).  Only u8 frames get past the first plan: a 5-tap
// layer (1 / scale < 3.2) fits it, and wider pixels (esize 2 / 4) take the fused form only where it fits (blur_resize_is_fused).
struct FusedPlan { int th, rows, pitch_w; size_t lds; };
static FusedPlan fused_plan(int W, int H, int w, int h, const BlurParams& bp, int dword_ok, int esize = 1)
{
    const int pitch = staged_pitch_words(W, w, bp.ksize);
    FusedPlan p{FB_TH, fused_blur_rows(H, h, bp.ksize), pitch, 0};
    if (fused_lds_bytes(p.rows, pitch, esize) > 64 * 1024) {
        const int rows8 = fused_blur_rows(H, h, bp.ksize, 8);
        if (bp.ksize == 13 && fused_fast_ok(bp, pitch, dword_ok, esize) && fused_lds_bytes(rows8, pitch, esize) <= 64 * 1024) { p.th = 8; p.rows = rows8; }
        else p.pitch_w = 0;
    }
    p.lds = fused_lds_bytes(p.rows, p.pitch_w, esize);
    return p;
}
bool blur_resize_is_fused(int W, int H, int w, int h, int ksize, int esize)
{
    if (!(!(w == W && h == H) && ksize <= 13 && H > 2 * ksize && W > 2 * ksize && (size_t)fused_blur_rows(H, h, ksize) * 256 <= 48 * 1024))
        return false;
    // u8: fused_plan falls back to 64 x 8 staged tiles or to the unstaged tile.  Wider pixels: fused only where the staged region of a
    // 64 x 16 tile (2x / 4x the bytes of u8) fits the 64 KB default dynamic LDS, whichever tile code the frames' alignment picks; else
    // the two-pass form, whose staged row block shrinks to fit 48 KB (or reads global memory directly)
    if (esize == 1) return true;
    const int pitch = staged_pitch_words(W, w, ksize);
    return fused_lds_bytes(fused_blur_rows(H, h, ksize), pitch, esize) <= 64 * 1024;
}

// Layer 0 (scale 1, sigma 0 -> fixed kernel [1/4, 1/2, 1/4], BORDER_REFLECT_101): every product is exact in f32,
// so this is bit-identical to OpenCV's row-then-column filter.  One thread = 4 consecutive pixels x 4 rows:
// six aligned quad row loads (u8: a dword) + the two neighbour pixels per row, float4 stores.
template <typename T>
static __device__ __forceinline__ void blur3_block(const T* __restrict__ src, float* __restrict__ dst, int W, int H, int bx, int by)
{
    typedef typename QuadOf<T>::type Q;
    const int x = (bx * 64 + (threadIdx.x & 63)) * 4;
    const int y0 = (by * 4 + (threadIdx.x >> 6)) * 4;
    if (x >= W || y0 >= H) return;
    const int xl = x == 0 ? 1 : x - 1;                    // reflect101
    const int xr = x + 4 >= W ? W - 2 : x + 4;
    // all 18 loads of the thread first (six rows x {left pixel, aligned quad, right pixel}); the outputs below are computed
    // unconditionally and only the stores are predicated, so no load is deferred behind a branch
    Q qs[6];
    T ls[6], rs[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        int yy = y0 - 1 + r;
        yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
        yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);         // rows past the image (tail of the last group): any valid row
        const T* p = src + (size_t)yy * W;
        qs[r] = *(const Q*)(p + x);
        ls[r] = p[xl];
        rs[r] = p[xr];
    }
    float hrow[6][4];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t q = qs[r];
            const float a = (float)ls[r], b0 = (float)(q & 255u), b1 = (float)((q >> 8) & 255u), b2 = (float)((q >> 16) & 255u),
                        b3 = (float)(q >> 24), c = (float)rs[r];
            hrow[r][0] = 0.5f * b0 + 0.25f * (a + b1);
            hrow[r][1] = 0.5f * b1 + 0.25f * (b0 + b2);
            hrow[r][2] = 0.5f * b2 + 0.25f * (b1 + b3);
            hrow[r][3] = 0.5f * b3 + 0.25f * (b2 + c);
        } else {                                            // the same four lines on the quad's converted pixels
            float b[4];
            quad_px<T>(qs[r], b);
            const float a = (float)ls[r], c = (float)rs[r];
            hrow[r][0] = 0.5f * b[0] + 0.25f * (a + b[1]);
            hrow[r][1] = 0.5f * b[1] + 0.25f * (b[0] + b[2]);
            hrow[r][2] = 0.5f * b[2] + 0.25f * (b[1] + b[3]);
            hrow[r][3] = 0.5f * b[3] + 0.25f * (b[2] + c);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float4 o;
        o.x = 0.5f * hrow[r + 1][0] + 0.25f * (hrow[r][0] + hrow[r + 2][0]);
        o.y = 0.5f * hrow[r + 1][1] + 0.25f * (hrow[r][1] + hrow[r + 2][1]);
        o.z = 0.5f * hrow[r + 1][2] + 0.25f * (hrow[r][2] + hrow[r + 2][2]);
        o.w = 0.5f * hrow[r + 1][3] + 0.25f * (hrow[r][3] + hrow[r + 2][3]);
        if (y0 + r < H) *(float4*)(dst + (size_t)(y0 + r) * W + x) = o;
    }
}

// The layer images of SEVERAL layers in one launch (a small group's pyramid: launch_blur_multi): job 0.. = layers whose blur is the
// 3x3 form (layer 0) or the fused form; workgroup b belongs to the last job whose first_block is <= b.
template <typename T, int PATH>      // the tile code its fused jobs need (FP_ANY when they differ)
__global__ __launch_bounds__(256) void k_blur_multi(const T* __restrict__ img, const T* __restrict__ img2, int split, size_t img_stride,
                                                    int W, int H, int dword_ok, BlurJobs jobs)
{
    extern __shared__ __attribute__((aligned(16))) float hrows[];
    int k = 0;
    for (int i = 1; i < jobs.n; i++) k = (int)blockIdx.x >= jobs.j[i].first_block ? i : k;
    const BlurJob J = jobs.j[k];
    const int b = (int)blockIdx.x - J.first_block;
    const int z = b / (J.gx * J.gy), rem = b - z * J.gx * J.gy;
    const int by = rem / J.gx, bx = rem - by * J.gx;
    const T* base = image_of(img, img2, split, img_stride, z);
    float* out = J.out + (size_t)z * J.out_stride;
    if (J.fused) blur_fused_any<T, PATH>(base, out, W, H, J.w, J.h, J.bp, J.rows_cap, J.pitch_w, dword_ok, J.th, bx, by, hrows);
    else blur3_block(base, out, W, H, bx, by);
}
// rows are quad-addressable (aligned dword / dwordx2 / dwordx4 loads) when W, the image stride (pixels) and both bases are multiples of
// four pixels
template <typename T>
static int quad_ok(const FrameRun<T>& f)
{
    const uintptr_t m = 4 * sizeof(T) - 1;
    return (f.W % 4 == 0 && f.img_stride % 4 == 0 && ((uintptr_t)f.img & m) == 0 && ((uintptr_t)f.img2 & m) == 0) ? 1 : 0;
}
// does the layer take the 3x3 form (blur3_block)?  f: two runs spelled out (FrameRun::runs)
template <typename T>
static bool blur3_fast_ok(const FrameRun<T>& f, const LayerTarget& t)
{
    return t.w == f.W && t.h == f.H && t.bp.fixed3 && f.W >= 8 && f.H >= 2 && quad_ok(f) && t.out_stride % 4 == 0 &&
           ((uintptr_t)t.out & 15) == 0;
}
// Layer images of several layers of G frames in ONE launch.  jobs[i]: the LayerTarget filled by the caller; a layer qualifies when
// blur_multi_ok says so (3x3 form or fused form).  Grid bookkeeping and the LDS size are filled here.
template <typename T>
bool blur_multi_ok(const FrameRun<T>& f, const LayerTarget& t)
{
    return blur3_fast_ok(f.runs(), t) || blur_resize_is_fused(f.W, f.H, t.w, t.h, t.bp.ksize, (int)sizeof(T));
}
// one launch for all jobs; f: two runs spelled out
template <typename T>
static void blur_multi_launch(hipStream_t st, const FrameRun<T>& f, int dword_ok, BlurJobs jobs)
{
    const int esize = (int)sizeof(T), W = f.W, H = f.H;
    int blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < jobs.n; i++) {
        BlurJob& J = jobs.j[i];
        J.fused = !(J.w == W && J.h == H);
        if (J.fused) {
            const FusedPlan fp = fused_plan(W, H, J.w, J.h, J.bp, dword_ok, esize);
            J.rows_cap = fp.rows; J.pitch_w = fp.pitch_w; J.th = fp.th;
            J.gx = (J.w + 63) / 64; J.gy = (J.h + fp.th - 1) / fp.th;
            lds = std::max(lds, fp.lds);
        } else {
            J.rows_cap = J.pitch_w = 0;
            J.gx = (W / 4 + 63) / 64; J.gy = ((H + 3) / 4 + 3) / 4;
        }
        J.first_block = blocks;
        blocks += J.gx * J.gy * f.G;
    }
    int path = -1;                                                          // one tile code for all fused jobs, or FP_ANY
    for (int i = 0; i < jobs.n; i++)
        if (jobs.j[i].fused) {
            const int p = fused_path_of(jobs.j[i].bp, jobs.j[i].pitch_w, dword_ok, esize);
            path = path < 0 ? p : (path == p ? p : FP_ANY);
        }
    with_fused_path<T>(path, [&](auto P) {
        hipLaunchKernelGGL((k_blur_multi<T, decltype(P)::value>), dim3(blocks), dim3(256), lds, st, f.img, f.img2, f.split, f.img_stride, W, H,
                           dword_ok, jobs);
    });
}
template <typename T>
void launch_blur_multi(hipStream_t st, const FrameRun<T>& frames, BlurJobs jobs)
{
    const FrameRun<T> f = frames.runs();
    const int dword_ok = quad_ok(f);
    const int esize = (int)sizeof(T);
    if (f.G <= 8) return blur_multi_launch(st, f, dword_ok, jobs);
    // many frames per layer (the deep layers of a whole call): one launch per tile code -- a launch that mixes them runs every layer at
    // the occupancy of the hungriest path -- instead of one launch in all
    bool done[MAV_MAX_JOBS] = {false};
    for (int i = 0; i < jobs.n; i++) {
        if (done[i]) continue;
        auto path_of = [&](const BlurJob& J) {
            if (J.w == f.W && J.h == f.H) return -1;
            const FusedPlan fp = fused_plan(f.W, f.H, J.w, J.h, J.bp, dword_ok, esize);
            return fused_path_of(J.bp, fp.pitch_w, dword_ok, esize);
        };
        const int p = path_of(jobs.j[i]);
        BlurJobs sub{0, 0, {}};
        for (int k = i; k < jobs.n; k++)
            if (!done[k] && path_of(jobs.j[k]) == p) { sub.j[sub.n++] = jobs.j[k]; done[k] = true; }
        blur_multi_launch(st, f, dword_ok, sub);
    }
}

// G images: the first `split` from run img, the rest from run img2 (both with stride img_stride); split >= G: one run.
template <typename T>
__global__ __launch_bounds__(256) void k_blur3(const T* __restrict__ img, const T* __restrict__ img2, int split,
                                               size_t img_stride, int W, int H, float* __restrict__ out, size_t out_stride)
{
    blur3_block(image_of(img, img2, split, img_stride, blockIdx.z), out + (size_t)blockIdx.z * out_stride, W, H, blockIdx.x, blockIdx.y);
}

// true when launch_blur_resize (scratch.two_pass = false) will go through the tmp scratch for these operands
template <typename T>
bool blur_resize_needs_tmp(const FrameRun<T>& f, const LayerTarget& t)
{
    return !blur3_fast_ok(f.runs(), t) && !blur_resize_is_fused(f.W, f.H, t.w, t.h, t.bp.ksize, (int)sizeof(T));
}
template <typename T>
void launch_blur_resize(hipStream_t st, const FrameRun<T>& frames, const LayerTarget& t, const BlurScratch& scratch)
{
    const FrameRun<T> f = frames.runs();
    const int G = f.G, W = f.W, H = f.H, w = t.w, h = t.h;
    const BlurParams& bp = t.bp;
    if (blur3_fast_ok(f, t)) {
        dim3 grid((W / 4 + 63) / 64, ((H + 3) / 4 + 3) / 4, G);
        hipLaunchKernelGGL(k_blur3<T>, grid, dim3(256), 0, st, f.img, f.img2, f.split, f.img_stride, W, H, t.out, t.out_stride);
        return;
    }
    const int dword_ok = quad_ok(f);     // else the staging goes pixel by pixel
    const int esize = (int)sizeof(T);
    const int pitch_w = staged_pitch_words(W, w, bp.ksize);
    if (!scratch.two_pass && blur_resize_is_fused(W, H, w, h, bp.ksize, esize)) {
        const FusedPlan fp = fused_plan(W, H, w, h, bp, dword_ok, esize);
        const dim3 grid((w + 63) / 64, (h + fp.th - 1) / fp.th, G);
        with_fused_path<T>(fused_path_of(bp, fp.pitch_w, dword_ok, esize), [&](auto P) {
            if constexpr (decltype(P)::value != FP_ANY)                     // (one layer has one tile code)
                hipLaunchKernelGGL((k_blur_resize_fused<T, decltype(P)::value>), grid, dim3(256), fp.lds, st, f.img, f.img2, f.split, f.img_stride,
                                   W, H, w, h, bp, t.out, t.out_stride, fp.rows, fp.pitch_w, dword_ok, fp.th);
        });
        return;
    }
    // the staged row block: rows_blk rows of pitch_w quads of esize-byte pixels
    int rows_blk = 16;
    while (rows_blk > 4 && (size_t)rows_blk * pitch_w * 4 * esize > 48 * 1024) rows_blk >>= 1;
    if ((size_t)rows_blk * pitch_w * 4 * esize <= 48 * 1024)
    {
        const int gx = (w + 63) / 64, nby = (H + rows_blk - 1) / rows_blk;
        const int gy = nby;                                               // one row block per workgroup (walking several measured slower: 69 vs 47 us)
        const size_t lds_h = (size_t)((rows_blk * pitch_w * esize + 1) & ~1) * 4 + (size_t)((bp.ksize + 4) & ~3) * 8;    // staged rows + tap pairs
        hipLaunchKernelGGL(k_blur_resize_h<T>, dim3(gx, gy, G), dim3(256), lds_h, st, f.img, f.img2, f.split, f.img_stride, W, H, w, bp,
                           scratch.tmp, scratch.stride, rows_blk, pitch_w, dword_ok);
    }
    else
        hipLaunchKernelGGL(k_blur_resize_h_direct<T>, dim3((w + 63) / 64, ((H + 3) / 4 + 3) / 4, G), dim3(256), 0, st, f.img, f.img2, f.split,
                           f.img_stride, W, H, w, bp, scratch.tmp, scratch.stride);
    hipLaunchKernelGGL(k_blur_resize_v, dim3((w + 63) / 64, (h + 3) / 4, G), dim3(256), 0, st, (const float*)scratch.tmp, scratch.stride, H, w,
                       h, bp, t.out, t.out_stride);
}
// the three source depths (mavflow_internal.h)
#define MAV_BLUR_DEPTH(T)                                                                                     \
    template bool blur_multi_ok<T>(const FrameRun<T>&, const LayerTarget&);                                   \
    template void launch_blur_multi<T>(hipStream_t, const FrameRun<T>&, BlurJobs);                            \
    template bool blur_resize_needs_tmp<T>(const FrameRun<T>&, const LayerTarget&);                           \
    template void launch_blur_resize<T>(hipStream_t, const FrameRun<T>&, const LayerTarget&, const BlurScratch&);
MAV_BLUR_DEPTH(uint8_t)
MAV_BLUR_DEPTH(uint16_t)
MAV_BLUR_DEPTH(float)
#undef MAV_BLUR_DEPTH

// ------------------------------------------------------------------------------------------------------------
// FarnebackPolyExp (A.4).  64x16 output tile per workgroup; the (64+2n) x (16+2n) source tile (edge-clamped,
// which is exactly OpenCV's row clamp + edge-triple replication) is staged in LDS, the vertical pass leaves
// three (64+2n) x 16 planes in LDS and the horizontal pass reads those.  Coefficients sit in kernel arguments
// (scalar loads).  Output: (h, w, 5), a wave's row of 64 pixels is 1 280 contiguous bytes.
// ------------------------------------------------------------------------------------------------------------
#define PX 64
#define PY 16
// An expansion is (h, w, 5): the five values of a pixel lie together, 20 bytes at 4-byte alignment.  A pixel is
// 16 + 4 bytes; the gather's row of two adjacent pixels is 16 + 16 + 8.
struct __attribute__((packed, aligned(4))) F2U { float x, y; };           // two / four adjacent floats at 4-byte alignment
struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };
static __device__ __forceinline__ void load5(const float* __restrict__ p, float v[5])
{
    const F4U a = *(const F4U*)p;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = p[4];
}
static __device__ __forceinline__ void store5(float* __restrict__ p, const float v[5])
{
    *(F4U*)p = F4U{v[0], v[1], v[2], v[3]};
    p[4] = v[4];
}
// one 64 x 16 tile of one image: src / dst = the image's layer plane and its expansion.  This is the RELAXED form: any width, any
// alignment, any poly_n (N_T == 0: n from the arguments).  polyexp_tile_fast below is the aligned form of the same arithmetic; the
// launch chooses (polyexp_vec_ok), and tests/test_gpu_polyexp_forms.py holds the two to the same bits.
template <int N_T>
static __device__ __forceinline__ void polyexp_tile(const float* __restrict__ src, float* __restrict__ dst, int w, int h, const PolyCoef& pc,
                                                    int tile_x, int tile_y, float* __restrict__ smem)
{
    const int n = N_T > 0 ? N_T : pc.n;
    const int EX = PX + 2 * n, EY = PY + 2 * n;
    float* tile = smem;
    float* v0 = tile + EX * EY;
    float* v1 = v0 + PY * EX;
    float* v2 = v1 + PY * EX;
    const int tid = threadIdx.x;
    const int x0 = tile_x * PX, y0 = tile_y * PY;

    if constexpr (N_T > 0) {
        // all of a thread's loads are issued before the first one is consumed (a load -> LDS-store loop would serialise
        // ten memory round trips per workgroup)
        constexpr int TOT = (PX + 2 * N_T) * (PY + 2 * N_T), CNT = (TOT + 255) / 256;
        float v[CNT];
#pragma unroll
        for (int j = 0; j < CNT; j++) {
            const int i = tid + 256 * j;
            if (i < TOT) {
                const int ly = i / EX, lx = i - ly * EX;
                const int gx = clampi(x0 - n + lx, 0, w - 1), gy = clampi(y0 - n + ly, 0, h - 1);
                v[j] = src[(size_t)gy * w + gx];
            }
        }
#pragma unroll
        for (int j = 0; j < CNT; j++)
            if (tid + 256 * j < TOT) tile[tid + 256 * j] = v[j];
    } else {
        for (int i = tid; i < EX * EY; i += 256) {
            const int ly = i / EX, lx = i - ly * EX;
            const int gx = clampi(x0 - n + lx, 0, w - 1), gy = clampi(y0 - n + ly, 0, h - 1);
            tile[i] = src[(size_t)gy * w + gx];
        }
    }
    __syncthreads();
    for (int i = tid; i < PY * EX; i += 256) {
        const int ly = i / EX, lx = i - ly * EX;
        const float* c = tile + (ly + n) * EX + lx;
        float t0 = c[0] * pc.g[0], t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 1; k <= n; k++) {               // (explicit fmaf: the bits must not depend on which kernel this is inlined into)
            const float a = c[-k * EX], b = c[k * EX];
            const float p = a + b;
            t0 = fmaf(pc.g[k], p, t0);
            t1 = fmaf(pc.xg[k], b - a, t1);
            t2 = fmaf(pc.xxg[k], p, t2);
        }
        v0[i] = t0; v1[i] = t1; v2[i] = t2;
    }
    __syncthreads();
    for (int i = tid; i < PY * PX; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= w || gy >= h) continue;
        const float* p0 = v0 + ly * EX + lx + n;
        const float* p1 = v1 + ly * EX + lx + n;
        const float* p2 = v2 + ly * EX + lx + n;
        float b1 = p0[0] * pc.g[0], b2 = 0.f, b3 = p1[0] * pc.g[0], b4 = 0.f, b5 = p2[0] * pc.g[0], b6 = 0.f;
#pragma unroll
        for (int k = 1; k <= n; k++) {
            const float a0 = p0[-k], c0 = p0[k], a1 = p1[-k], c1 = p1[k], a2 = p2[-k], c2 = p2[k];
            const float tg = c0 + a0;
            b1 = fmaf(tg, pc.g[k], b1);
            b4 = fmaf(tg, pc.xxg[k], b4);
            b2 = fmaf(c0 - a0, pc.xg[k], b2);
            b3 = fmaf(c1 + a1, pc.g[k], b3);
            b6 = fmaf(c1 - a1, pc.xg[k], b6);
            b5 = fmaf(c2 + a2, pc.g[k], b5);
        }
        // the pixel's five values as 16 + 4 bytes, a wave's row 1 280 contiguous bytes.  (Measured, not kept: the row staged through LDS
        // and stored as 16 bytes per consecutive lane -- k_polyexp<8> 231 us per launch against 217; HISTORY.md, "Expansion layout".)
        const float r[5] = {b3 * pc.ig11, b2 * pc.ig11, fmaf(b5, pc.ig33, b1 * pc.ig03), fmaf(b4, pc.ig33, b1 * pc.ig03), b6 * pc.ig55};
        store5(dst + 5 * ((size_t)gy * w + gx), r);
    }
}

// The aligned fast form of the same tile (N_T > 0, polyexp_vec_ok: width a multiple of 4, 16-byte aligned planes): the same values
// bit for bit -- every output is the relaxed form's expression in the relaxed form's order, two adjacent pixels per packed
// instruction -- with the taps carried in registers instead of re-read from LDS for every output.
//   staging     the source tile as 16-byte quads, 20 per row: columns x0 - 8 .. x0 + 71 whatever n is, so that every quad is aligned;
//               with w % 4 == 0 a quad lies wholly inside the image or wholly outside, where it is the edge pixel replicated
//   vertical    one thread per (column pair, block of 4 rows): its 4 + 2n float2 values are read once and slide through registers
//               for the 4 x 2 outputs of the three planes (plane column = tile column + 8)
//   horizontal  one thread per 4 consecutive pixels of a row, lanes laid out by the hardware's ds_read_b128 lane groups as in the sweep
//               kernel's phase B (16 consecutive quads of one row per group: every bank once at any pitch); per plane five 16-byte
//               reads
//   stores      a thread's 4 pixels are 80 contiguous bytes of the expansion, but stored from there a wave's store instruction would
//               touch 40 cache lines at 16 bytes in every 80 (measured: 257 us per launch of k_polyexp<8> against the relaxed form's
//               217).  The 16 lanes of a row exchange their quads through LDS that nobody reads any more -- the wave's own rows of
//               the three planes and a row of the tile region -- and lane p stores quads p, 16 + p, .. 64 + p of the row's 80: 256
//               contiguous bytes per row and instruction (169 us).  Same wave, LDS operations in program order: no barrier.
// LDS: (16 + 2n) x 84 + 3 x 16 x 80 floats = 25.5 KB at n = 8.  The tile pitch of 84 puts the two row blocks that one half-wave of the
// vertical pass can straddle (4 rows apart) on disjoint banks.  HISTORY.md, "Polynomial expansion: the aligned fast form".
typedef float pk2 __attribute__((ext_vector_type(2)));
#define PF_QX 20                // quads per staged row
#define PF_TP 84                // tile pitch (floats)
#define PF_PP 80                // plane pitch
static __device__ __forceinline__ pk2 pk_fma(float s, pk2 x, pk2 acc) { return __builtin_elementwise_fma(pk2{s, s}, x, acc); }
// A thread's 20 floats of one plane row as five 16-byte reads.  n < 8 leaves the outer 8 - n floats unused, and the compiler would then
// re-form the reads from the pairs the arithmetic takes, at 4-byte alignment (ds_read2_b32 at a 16-byte lane stride: 4-way bank
// conflicts, and floats read several times): there the quads pass through an empty asm statement, which it cannot look through.
template <int N_T>
static __device__ __forceinline__ void load_quads5(const float* __restrict__ p, float f[20])
{
    typedef float pk4 __attribute__((ext_vector_type(4)));
    pk4 t[5];
#pragma unroll
    for (int k = 0; k < 5; k++) t[k] = ((const pk4*)p)[k];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        if constexpr (N_T < 8) asm volatile("" : "+v"(t[k]));
        f[4 * k] = t[k].x; f[4 * k + 1] = t[k].y; f[4 * k + 2] = t[k].z; f[4 * k + 3] = t[k].w;
    }
}
template <int N_T>
static __device__ __forceinline__ void polyexp_tile_fast(const float* __restrict__ src, float* __restrict__ dst, int w, int h, const PolyCoef& pc,
                                                         int tile_x, int tile_y, float* __restrict__ smem)
{
    constexpr int n = N_T, EY = PY + 2 * n, NV = 4 + 2 * n;
    float* tile = smem;
    float* v0 = tile + EY * PF_TP;
    float* v1 = v0 + PY * PF_PP;
    float* v2 = v1 + PY * PF_PP;
    const int tid = threadIdx.x;
    const int x0 = tile_x * PX, y0 = tile_y * PY;
    {
        // all of a thread's loads are issued before the first LDS store, as in the relaxed form
        constexpr int TOT = PF_QX * EY, CNT = (TOT + 255) / 256;
        // (straight-line loads -- a thread past the last quad re-reads that quad -- and selects afterwards: with the load or the edge
        // replication under a branch the compiler splits the load and waits for its first part before it issues the next)
        float4 q[CNT];
#pragma unroll
        for (int j = 0; j < CNT; j++) {
            const int i = min(tid + 256 * j, TOT - 1);
            const int ly = i / PF_QX, qx = i - ly * PF_QX;
            const int gx = x0 - 8 + 4 * qx, gy = clampi(y0 - n + ly, 0, h - 1);
            q[j] = *(const float4*)(src + (size_t)gy * w + clampi(gx, 0, w - 4));
        }
#pragma unroll
        for (int j = 0; j < CNT; j++) {
            const int i = tid + 256 * j;
            const int ly = i / PF_QX, qx = i - ly * PF_QX;
            const int gx = x0 - 8 + 4 * qx;
            const bool lo = gx < 0, hi = gx >= w, out = lo || hi;
            const float4 t = q[j];
            const float e = lo ? t.x : t.w;
            if (i < TOT) *(float4*)(tile + ly * PF_TP + 4 * qx) = make_float4(hi ? e : t.x, out ? e : t.y, out ? e : t.z, lo ? e : t.w);
        }
    }
    __syncthreads();
    if (tid < (PY / 4) * (PF_PP / 2)) {
        const int rb = tid / (PF_PP / 2), cp = tid - rb * (PF_PP / 2);
        const float* c = tile + rb * 4 * PF_TP + 2 * cp;
        pk2 v[NV];
#pragma unroll
        for (int i = 0; i < NV; i++) v[i] = *(const pk2*)(c + i * PF_TP);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            pk2 t0 = v[j + n] * pc.g[0], t1 = pk2{0.f, 0.f}, t2 = pk2{0.f, 0.f};
#pragma unroll
            for (int k = 1; k <= n; k++) {
                const pk2 a = v[j + n - k], b = v[j + n + k];
                const pk2 p = a + b;
                t0 = pk_fma(pc.g[k], p, t0);
                t1 = pk_fma(pc.xg[k], b - a, t1);
                t2 = pk_fma(pc.xxg[k], p, t2);
            }
            const int o = (rb * 4 + j) * PF_PP + 2 * cp;
            *(pk2*)(v0 + o) = t0; *(pk2*)(v1 + o) = t1; *(pk2*)(v2 + o) = t2;
        }
    }
    __syncthreads();
    {
        // hardware b128 lane group -> tile row, position inside the group -> the row's quad (k_blur_iter_fast, phase B)
        const int lane = tid & 63, wv = tid >> 6;
        const int quad = (lane & 31) >> 2;
        const int grp = (lane >> 5) * 2 + ((quad == 1 || quad == 2 || quad == 4 || quad == 7) ? 1 : 0);
        const int qpos = (quad == 0 || quad == 1) ? 0 : ((quad == 3 || quad == 2) ? 1 : ((quad == 5 || quad == 4) ? 2 : 3));
        const int ly = wv * 4 + grp, lx0 = (qpos * 4 + (lane & 3)) * 4;
        const int gy = y0 + ly;
        const int o = ly * PF_PP + lx0;       // f[i] = plane column lx0 + i; pixel j of the thread sits at f[8 + j]
        float f[20];
        pk2 b1[2], b2[2], b3[2], b4[2], b5[2], b6[2];
        load_quads5<N_T>(v0 + o, f);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int m = 8 + 2 * j;
            b1[j] = pk2{f[m], f[m + 1]} * pc.g[0]; b2[j] = pk2{0.f, 0.f}; b4[j] = pk2{0.f, 0.f};
#pragma unroll
            for (int k = 1; k <= n; k++) {
                const pk2 a0 = pk2{f[m - k], f[m + 1 - k]}, c0 = pk2{f[m + k], f[m + 1 + k]};
                const pk2 tg = c0 + a0;
                b1[j] = pk_fma(pc.g[k], tg, b1[j]);
                b4[j] = pk_fma(pc.xxg[k], tg, b4[j]);
                b2[j] = pk_fma(pc.xg[k], c0 - a0, b2[j]);
            }
        }
        load_quads5<N_T>(v1 + o, f);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int m = 8 + 2 * j;
            b3[j] = pk2{f[m], f[m + 1]} * pc.g[0]; b6[j] = pk2{0.f, 0.f};
#pragma unroll
            for (int k = 1; k <= n; k++) {
                const pk2 a1 = pk2{f[m - k], f[m + 1 - k]}, c1 = pk2{f[m + k], f[m + 1 + k]};
                b3[j] = pk_fma(pc.g[k], c1 + a1, b3[j]);
                b6[j] = pk_fma(pc.xg[k], c1 - a1, b6[j]);
            }
        }
        load_quads5<N_T>(v2 + o, f);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int m = 8 + 2 * j;
            b5[j] = pk2{f[m], f[m + 1]} * pc.g[0];
#pragma unroll
            for (int k = 1; k <= n; k++) {
                const pk2 a2 = pk2{f[m - k], f[m + 1 - k]}, c2 = pk2{f[m + k], f[m + 1 + k]};
                b5[j] = pk_fma(pc.g[k], c2 + a2, b5[j]);
            }
        }
        float r[20];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const pk2 r0 = b3[j] * pc.ig11, r1 = b2[j] * pc.ig11, e = b1[j] * pc.ig03;
            const pk2 r2 = pk_fma(pc.ig33, b5[j], e), r3 = pk_fma(pc.ig33, b4[j], e), r4 = b6[j] * pc.ig55;
            float* q = r + 10 * j;
            q[0] = r0.x; q[1] = r1.x; q[2] = r2.x; q[3] = r3.x; q[4] = r4.x;
            q[5] = r0.y; q[6] = r1.y; q[7] = r2.y; q[8] = r3.y; q[9] = r4.y;
        }
        // the row's 80 quads through LDS (this wave's own rows of the three planes + a row of the tile region, 20 quads each): lane pos
        // leaves quads 5 pos .. 5 pos + 4 and takes quads 16 k + pos, so that a store instruction covers 256 contiguous bytes per row
        {
            const int pos = lx0 >> 2;
            auto chunk = [&](int c) { return smem + (c < 3 ? EY * PF_TP + c * PY * PF_PP : 0) + ly * PF_PP; };
            float* wr = chunk(pos >> 2) + 4 * (5 * (pos & 3));
#pragma unroll
            for (int k = 0; k < 5; k++) *(float4*)(wr + 4 * k) = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
            const int vq = 5 * (min(PX, w - x0) >> 2);          // valid quads of the row
            float4* out = (float4*)(dst + 5 * ((size_t)gy * w + x0));
            float4 t[5];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const int idx = 16 * k + pos, c = idx / 20;
                t[k] = *(const float4*)(chunk(c) + 4 * (idx - 20 * c));
            }
            if (gy < h) {
#pragma unroll
                for (int k = 0; k < 5; k++)
                    if (16 * k + pos < vq) out[16 * k + pos] = t[k];
            }
        }
    }
}
// one tile in the form the launch chose (`fast`: polyexp_vec_ok held on the host; uniform over the workgroup)
template <int N_T>
static __device__ __forceinline__ void polyexp_tile_any(bool fast, const float* __restrict__ src, float* __restrict__ dst, int w, int h,
                                                        const PolyCoef& pc, int tile_x, int tile_y, float* __restrict__ smem)
{
    if constexpr (N_T > 0) {
        if (fast) { polyexp_tile_fast<N_T>(src, dst, w, h, pc, tile_x, tile_y, smem); return; }
    }
    polyexp_tile<N_T>(src, dst, w, h, pc, tile_x, tile_y, smem);
}

template <int N_T>
__global__ __launch_bounds__(256) void k_polyexp(const float* __restrict__ I, size_t I_stride, int w, int h, PolyCoef pc, TileMap tm,
                                                 float* __restrict__ R, size_t R_stride, int fast)
{
    int img_s, tile_x, tile_y;
    if (!tile_of_block(tm, &img_s, &tile_x, &tile_y)) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    polyexp_tile_any<N_T>(fast != 0, I + (size_t)img_s * I_stride, R + (size_t)img_s * R_stride, w, h, pc, tile_x, tile_y, smem);
}

// The expansions of SEVERAL layers in one launch (a small group's whole pyramid: launch_polyexp_multi): workgroup b belongs to the
// last job whose first_block is <= b and takes that job's tile b - first_block (plain row-major order, image by image).
template <int N_T>
__global__ __launch_bounds__(256) void k_polyexp_multi(PolyJobs jobs, PolyCoef pc)
{
    int k = 0;
    for (int i = 1; i < jobs.n; i++) k = (int)blockIdx.x >= jobs.j[i].first_block ? i : k;
    const PolyJob J = jobs.j[k];
    const int tile = (int)blockIdx.x - J.first_block;
    const int img_s = tile / J.per_img, rem = tile - img_s * J.per_img;
    const int tile_y = rem / J.tiles_x, tile_x = rem - tile_y * J.tiles_x;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    polyexp_tile_any<N_T>(J.fast != 0, J.I + (size_t)img_s * J.I_stride, J.R + (size_t)img_s * J.R_stride, J.w, J.h, pc, tile_x, tile_y, smem);
}
// The fast form's predicate (the same kind as blur_iter_vec_ok): every quad of a row, of the source and of the expansion, is 16-byte
// aligned in every slot.  poly_n 8, 7 and 5 have the form; every other n takes the relaxed one.
static bool polyexp_vec_ok(const float* I, size_t I_stride, const float* R, size_t R_stride, int w, int n)
{
    return (n == 8 || n == 7 || n == 5) && w >= 4 && w % 4 == 0 && I_stride % 4 == 0 && R_stride % 4 == 0 && ((uintptr_t)I & 15) == 0 &&
           ((uintptr_t)R & 15) == 0;
}
// dynamic LDS of a launch: the relaxed form's, or the larger of the two when a job takes the fast form
static size_t polyexp_lds_bytes(int n, bool fast)
{
    const size_t relaxed = sizeof(float) * ((size_t)(PX + 2 * n) * (PY + 2 * n) + 3 * (size_t)PY * (PX + 2 * n));
    const size_t vec = sizeof(float) * ((size_t)(PY + 2 * n) * PF_TP + 3 * (size_t)PY * PF_PP);
    return fast && vec > relaxed ? vec : relaxed;
}
// jobs[i]: G images of a (w x h) layer at I (slot stride I_stride) -> R (slot stride R_stride); first_block / tiles_x / per_img / fast are
// filled here
void launch_polyexp_multi(hipStream_t st, PolyJobs jobs, int G, const PolyCoef& pc)
{
    const int n = pc.n;
    int blocks = 0;
    bool any_fast = false;
    for (int i = 0; i < jobs.n; i++) {
        PolyJob& J = jobs.j[i];
        J.tiles_x = (J.w + PX - 1) / PX;
        J.per_img = J.tiles_x * ((J.h + PY - 1) / PY);
        J.first_block = blocks;
        J.fast = polyexp_vec_ok(J.I, J.I_stride, J.R, J.R_stride, J.w, n);
        any_fast |= J.fast != 0;
        blocks += J.per_img * G;
    }
    const size_t lds = polyexp_lds_bytes(n, any_fast);
    if (n == 8) hipLaunchKernelGGL(k_polyexp_multi<8>, dim3(blocks), dim3(256), lds, st, jobs, pc);
    else if (n == 7) hipLaunchKernelGGL(k_polyexp_multi<7>, dim3(blocks), dim3(256), lds, st, jobs, pc);
    else if (n == 5) hipLaunchKernelGGL(k_polyexp_multi<5>, dim3(blocks), dim3(256), lds, st, jobs, pc);
    else hipLaunchKernelGGL(k_polyexp_multi<0>, dim3(blocks), dim3(256), lds, st, jobs, pc);
}

void launch_polyexp(hipStream_t st, const float* I, size_t I_stride, int G, int w, int h, const PolyCoef& pc, float* R,
                    size_t R_stride)
{
    const int n = pc.n;
    const int fast = polyexp_vec_ok(I, I_stride, R, R_stride, w, n);
    const size_t lds = polyexp_lds_bytes(n, fast != 0);
    TileMap tm = make_tile_map(w, h, G, PX, PY);
    tm.xcd = 0;        // plain row-major order: measured 3 % faster here than the XCD-banded order (the halo re-reads that miss
                       // L2 hit the Infinity Cache, which all XCDs share; the kernel is VALU / write bound, not read bound)
    const dim3 grid(tile_grid(tm));
    if (n == 8)
        hipLaunchKernelGGL(k_polyexp<8>, grid, dim3(256), lds, st, I, I_stride, w, h, pc, tm, R, R_stride, fast);
    else if (n == 7)
        hipLaunchKernelGGL(k_polyexp<7>, grid, dim3(256), lds, st, I, I_stride, w, h, pc, tm, R, R_stride, fast);
    else if (n == 5)
        hipLaunchKernelGGL(k_polyexp<5>, grid, dim3(256), lds, st, I, I_stride, w, h, pc, tm, R, R_stride, fast);
    else
        hipLaunchKernelGGL(k_polyexp<0>, grid, dim3(256), lds, st, I, I_stride, w, h, pc, tm, R, R_stride, fast);
}

// ------------------------------------------------------------------------------------------------------------
// FarnebackUpdateMatrices for one pixel (A.5): a GATHER of the 2x2 neighbourhood of R1 around (x + dx, y + dy), then ONE
// body, update_finish, that turns (q[] = the 5 R0 values at (x, y), the taps, the flow) into the 5 M values.  Every kernel that builds
// M calls that body; they differ only in how the taps arrive.
struct GatherPx {
    float p00[5], p01[5], p10[5], p11[5];
    float fx, fy;
    bool inside;
};
// one row of the neighbourhood: the pixels at p and p + 5, ten adjacent floats, as 16 + 16 + 8 bytes
static __device__ __forceinline__ void gather_row(const float* __restrict__ p, float a[5], float b[5])
{
    const F4U t0 = *(const F4U*)p, t1 = *(const F4U*)(p + 4);
    const F2U t2 = *(const F2U*)(p + 8);
    a[0] = t0.x; a[1] = t0.y; a[2] = t0.z; a[3] = t0.w; a[4] = t1.x;
    b[0] = t1.y; b[1] = t1.z; b[2] = t1.w; b[3] = t2.x; b[4] = t2.y;
}
// the sweep's fast form: the loads are issued unconditionally, so that two pixels' gathers are in flight together; a neighbourhood that
// is not inside the image reads the one at (0, 0) instead and discards it.  On a layer of one row or one column no neighbourhood is
// inside, and the second row of that read is the first one again: it stays inside the expansion (DESIGN.md has the one exception, 1 x 1)
static __device__ __forceinline__ void gather_issue(const float* __restrict__ R1p, int w, int h, int x, int y, float dx, float dy, GatherPx& g)
{
    float fx = x + dx, fy = y + dy;
    const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    g.fx = fx - x1; g.fy = fy - y1;
    g.inside = (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
    const int xc = g.inside ? x1 : 0, yc = g.inside ? y1 : 0;
    const float* p = R1p + 5 * ((size_t)yc * w + xc);
    const size_t row = (w > 1 && h > 1) ? 5 * (size_t)w : 0;             // uniform
    gather_row(p, g.p00, g.p01);
    gather_row(p + row, g.p10, g.p11);
}
// the memory form's gather: the taps are read only when the neighbourhood is inside the image
static __device__ __forceinline__ void gather_inside(const float* __restrict__ R1p, int w, int h, int x, int y, float dx, float dy, GatherPx& g)
{
    float fx = x + dx, fy = y + dy;
    const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    g.fx = fx - x1; g.fy = fy - y1;
    g.inside = (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
    if (!g.inside) return;
    const float* p = R1p + 5 * ((size_t)y1 * w + x1);
    gather_row(p, g.p00, g.p01);
    gather_row(p + 5 * (size_t)w, g.p10, g.p11);
}
static __device__ __forceinline__ void update_finish(const float q[5], const GatherPx& g, int w, int h, int x, int y, float dx,
                                                     float dy, float out[5])
{
    // Every multiply-add below is spelled out (fmaf) and contraction is off for the rest: the bits must not depend on which kernel
    // (or which template instantiation of one) the function is inlined into -- under -ffp-contract=fast (this file's setting until round 3) two
    // instantiations of the sweep kernel that differed in a store instruction fused `a*b + c*d` differently and their flows drifted
    // apart by up to 8e-4 px over twenty sweeps.
#pragma clang fp contract(off)
    float r2, r3, r4, r5, r6;
    if (g.inside) {
        const float gx = 1.f - g.fx, gy = 1.f - g.fy;
        const float a00 = gx * gy, a01 = g.fx * gy, a10 = gx * g.fy, a11 = g.fx * g.fy;
        r2 = fmaf(a11, g.p11[0], fmaf(a10, g.p10[0], fmaf(a01, g.p01[0], a00 * g.p00[0])));
        r3 = fmaf(a11, g.p11[1], fmaf(a10, g.p10[1], fmaf(a01, g.p01[1], a00 * g.p00[1])));
        r4 = fmaf(a11, g.p11[2], fmaf(a10, g.p10[2], fmaf(a01, g.p01[2], a00 * g.p00[2])));
        r5 = fmaf(a11, g.p11[3], fmaf(a10, g.p10[3], fmaf(a01, g.p01[3], a00 * g.p00[3])));
        r6 = fmaf(a11, g.p11[4], fmaf(a10, g.p10[4], fmaf(a01, g.p01[4], a00 * g.p00[4])));
        r4 = (q[2] + r4) * 0.5f;
        r5 = (q[3] + r5) * 0.5f;
        r6 = (q[4] + r6) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = q[2]; r5 = q[3]; r6 = q[4] * 0.5f;
    }
    r2 = (q[0] - r2) * 0.5f;
    r3 = (q[1] - r3) * 0.5f;
    r2 += fmaf(r4, dy, r6 * dx);
    r3 += fmaf(r6, dy, r5 * dx);
    const int BORDER = 5;
    if ((unsigned)(x - BORDER) >= (unsigned)(w - BORDER * 2) || (unsigned)(y - BORDER) >= (unsigned)(h - BORDER * 2)) {
        // border[] = {0.14, 0.14, 0.4472, 0.4472, 0.4472}
        auto bw = [](int d) { return d < 2 ? 0.14f : 0.4472f; };
        const float scale = (x < BORDER ? bw(x) : 1.f) * (x >= w - BORDER ? bw(w - x - 1) : 1.f) *
                            (y < BORDER ? bw(y) : 1.f) * (y >= h - BORDER ? bw(h - y - 1) : 1.f);
        r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    }
    out[0] = fmaf(r4, r4, r6 * r6);
    out[1] = (r4 + r5) * r6;
    out[2] = fmaf(r5, r5, r6 * r6);
    out[3] = fmaf(r4, r2, r6 * r3);
    out[4] = fmaf(r6, r2, r5 * r3);
}

// memory form: R0p/R1p point at the pair's two expansions (h, w, 5); Mp at plane 0 of its M, planes are npx apart.
static __device__ __forceinline__ void update_px(const float* __restrict__ R0p, const float* __restrict__ R1p, size_t npx,
                                                 int w, int h, int x, int y, float dx, float dy, float* __restrict__ Mp)
{
    const size_t idx = (size_t)y * w + x;
    float q[5], o[5];
    load5(R0p + 5 * idx, q);
    GatherPx g;
    gather_inside(R1p, w, h, x, y, dx, dy, g);
    update_finish(q, g, w, h, x, y, dx, dy, o);
#pragma unroll
    for (int c = 0; c < 5; c++) Mp[c * npx + idx] = o[c];
}

// 2x2 solve of the blurred system (A.6).  Differences of products with one fused rounding each (Kahan): the CPU path
// does this step in double.
static __device__ __forceinline__ void solve_px(float g11, float g12, float g22, float h1, float h2, float* u, float* v)
{
    const float p = g12 * g12, pe = fmaf(g12, g12, -p);
    const float det = (fmaf(g11, g22, -p) - pe) + 1e-3f;
    const float idet = 1.f / det;
    const float qa = g12 * h1, qae = fmaf(g12, h1, -qa);
    const float qb = g12 * h2, qbe = fmaf(g12, h2, -qb);
    *u = (fmaf(g11, h2, -qa) - qae) * idet;
    *v = (fmaf(g22, h1, -qb) - qbe) * idet;
}

// resize(prevFlow -> layer size, INTER_LINEAR) * mul at one pixel (A.2): half-pixel centres, clamped, f32 weights.
static __device__ __forceinline__ float2 upsample_flow(const float* __restrict__ pf, int pw, int ph, float mul, double scale_x,
                                                       double scale_y, int x, int y)
{
#pragma clang fp contract(off)                       // products and sums rounded one by one, as resize()'s host code does
    float fy = (float)((y + 0.5) * scale_y - 0.5);
    int sy = (int)floorf(fy);
    fy -= sy;
    if (sy < 0) { fy = 0.f; sy = 0; }
    if (sy >= ph - 1) { fy = 0.f; sy = ph - 1; }
    const int sy1 = sy + 1 < ph ? sy + 1 : sy;
    float fx = (float)((x + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= pw - 1) { fx = 0.f; sx = pw - 1; }
    const int sx1 = sx + 1 < pw ? sx + 1 : sx;
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
    const float2 p00 = *(const float2*)(pf + ((size_t)sy * pw + sx) * 2);
    const float2 p01 = *(const float2*)(pf + ((size_t)sy * pw + sx1) * 2);
    const float2 p10 = *(const float2*)(pf + ((size_t)sy1 * pw + sx) * 2);
    const float2 p11 = *(const float2*)(pf + ((size_t)sy1 * pw + sx1) * 2);
    return make_float2(((p00.x * a0 + p01.x * a1) * b0 + (p10.x * a0 + p11.x * a1) * b1) * mul,
                       ((p00.y * a0 + p01.y * a1) * b0 + (p10.y * a0 + p11.y * a1) * b1) * mul);
}

// Initial M of a layer.  flow = 0 (top layer), resize(prevFlow)*mul evaluated inline (lower layers), or an
// explicit flow field (stage hook; the top layer of a call with an initial flow).  The upsampled flow is never written: the first blur sweep overwrites it.
// One thread per pixel, 64 x 4 pixels per workgroup on a plain 2-D grid.  (Measured alternative, not kept: 64 x 16 tiles in the
// XCD-aware order with two gathers in flight per thread -- L2 absorbed the gather rows, the kernel ran 5 % slower: its reads
// that miss L2 are served by the Infinity Cache anyway, and the taller tile halves the number of workgroups in flight.  And with the
// expansions interleaved: 64 x 8 per workgroup, a wave on two adjacent rows with both gathers in flight, fetched 8 % less than 64 x 4
// (2 x FETCH_SIZE 6.36 vs 6.89 GB per step) and ran no faster: 3.69 vs 3.65 ms of class time; HISTORY.md, "Expansion layout".)
template <int MODE>  // 0 zero, 1 upsample, 2 explicit
__global__ __launch_bounds__(256) void k_update_matrices(const float* __restrict__ R0, const float* __restrict__ R1,
                                                         size_t R_stride, const float* __restrict__ fsrc, size_t f_stride,
                                                         int pw, int ph, float mul, double scale_x, double scale_y, int w,
                                                         int h, float* __restrict__ M, size_t M_stride, int y_begin, int y_end)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = y_begin + blockIdx.y * 4 + (threadIdx.x >> 6);          // rows [y_begin, y_end) of the layer only
    if (x >= w || y >= y_end) return;
    const int s = blockIdx.z;
    float dx = 0.f, dy = 0.f;
    if (MODE == 1) {
        const float2 f = upsample_flow(fsrc + (size_t)s * f_stride, pw, ph, mul, scale_x, scale_y, x, y);
        dx = f.x; dy = f.y;
    } else if (MODE == 2) {
        const float2 f = *(const float2*)(fsrc + (size_t)s * f_stride + ((size_t)y * w + x) * 2);
        dx = f.x; dy = f.y;
    }
    update_px(R0 + (size_t)s * R_stride, R1 + (size_t)s * R_stride, (size_t)w * h, w, h, x, y, dx, dy,
              M + (size_t)s * M_stride);
}

void launch_initial_m(hipStream_t st, const InitialMArgs& a, const FlowSource& src)
{
    const int y_begin = a.y_begin < 0 ? 0 : a.y_begin, y_end = (a.y_end < 0 || a.y_end > a.h) ? a.h : a.y_end;
    if (y_end <= y_begin) return;
    const auto k = src.kind == FlowSource::COARSER ? k_update_matrices<1> : src.kind == FlowSource::FIELD ? k_update_matrices<2> : k_update_matrices<0>;
    hipLaunchKernelGGL(k, dim3((a.w + 63) / 64, (y_end - y_begin + 3) / 4, a.G), dim3(256), 0, st, a.R0, a.R1, a.R_stride, src.flow, src.stride,
                       src.pw, src.ph, src.mul, (double)src.pw / a.w, (double)src.ph / a.h, a.w, a.h, a.M, a.M_stride, y_begin, y_end);
}

// ------------------------------------------------------------------------------------------------------------
// The sweep's window: a compile-time policy of the two sweep kernels below (box: FarnebackUpdateFlow_Blur; Gaussian:
// OPTFLOW_FARNEBACK_GAUSSIAN, FarnebackUpdateFlow_GaussianBlur).  Tiles, halo, LDS layout, launch geometry and the bytes moved are the
// same for both; a policy holds what differs: the kernel argument, how a run of N + 2m values becomes N windowed sums, the 2x2 solve.
//   sums<M_T, N, REGS>(m_rt, in, out)   in(i), i = 0 .. N + 2m - 1, reads input i; out(j, s), j = 0 .. N - 1, takes sum j, the one over
//       inputs j .. j + 2m.  Whatever sum j + 1 needs of input j is read before out(j, ...) runs, so out(j) may overwrite input j (the
//       generic form sums in place in LDS).  m = M_T when M_T > 0 (the loops over the taps unroll), else m_rt.  REGS: inputs and
//       outputs are registers, so the loop over the outputs unrolls fully; otherwise they are LDS and it unrolls in part.  A value is
//       whatever in() returns: a float, or the float2 of a column pair (the fast form's phase A; each half has the float's arithmetic).
//   solve(g11, g12, g22, h1, h2, &u, &v)   the flow of one pixel from its five sums.
// Every pass of both kernel forms takes its sums from sums() and its flow from solve(); nothing else in them knows the window.
// Box: the sum of the first 2m + 1 values, then slide; the 1 / winsize^2 scale goes in front of the solve.
// Gaussian: everything in float32, nothing fused, one fixed order per value (tests/gauss_window_ref.py restates it in numpy; the kernels
// equal it bit for bit) -- vertically, then horizontally on the result, with edge-clamped coordinates:
//   V(y, x) = M(y, x) k0;  for i = 1..m:  V += (M(max(y - i, 0), x) + M(min(y + i, h - 1), x)) k_i
//   S(y, x) = V(y, x) k0;  for i = 1..m:  S += (V(y, max(x - i, 0)) + V(y, min(x + i, w - 1))) k_i
// The taps do not sum to 1 and there is no 1 / winsize^2 scale: 19 operations per output and plane at m = 6 against the box's 2.
// ------------------------------------------------------------------------------------------------------------
struct BoxWindow {
    float scale;                                       // 1 / winsize^2
    template <int M_T, int N, bool REGS, typename In, typename Out>
    __device__ __forceinline__ void sums(int m_rt, In in, Out out) const
    {
        const int win = 2 * (M_T > 0 ? M_T : m_rt) + 1;
        constexpr int UNROLL = REGS ? N : 8;
        decltype(in(0)) sum{};
#pragma unroll
        for (int k = 0; k < win; k++) sum += in(k);
#pragma unroll UNROLL
        for (int j = 0; j < N; j++) {
            const auto s = sum;
            if (j < N - 1) sum += in(j + win) - in(j);
            out(j, s);
        }
    }
    __device__ __forceinline__ void solve(float g11, float g12, float g22, float h1, float h2, float* u, float* v) const
    {
        solve_px(g11 * scale, g12 * scale, g22 * scale, h1 * scale, h2 * scale, u, v);
    }
};

void gauss_taps(int winsize, GaussTaps* out)
{
    const int m = winsize / 2;
    const double sigma = m * 0.3;
    float t[MAV_MAX_WIN_HALF + 1];
    double s = 1.;                                     // as the CPU code has it: starts at 1, and the centre tap counts twice too
    for (int i = 0; i <= m; i++) {
        t[i] = (float)exp(-i * i / (2 * sigma * sigma));
        s += t[i] * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= MAV_MAX_WIN_HALF; i++) out->k[i] = i <= m ? (float)(t[i] * s) : 0.f;
}

// the 2x2 solve as the Gaussian CPU path has it: products and differences in float32, the regularised reciprocal and the final
// product in double.  (solve_px above is the box path's, which sums in double on the CPU.)
static __device__ __forceinline__ void solve_gauss_px(float g11, float g12, float g22, float h1, float h2, float* u, float* v)
{
#pragma clang fp contract(off)
    const float d = g11 * g22 - g12 * g12;
    const double idet = 1.0 / ((double)d + 1e-3);
    *u = (float)((double)(g11 * h2 - g12 * h1) * idet);
    *v = (float)((double)(g22 * h1 - g12 * h2) * idet);
}

struct GaussWindow {
    GaussTaps gt;
    template <int M_T, int N, bool REGS, typename In, typename Out>
    __device__ __forceinline__ void sums(int m_rt, In in, Out out) const
    {
#pragma clang fp contract(off)
        const int m = M_T > 0 ? M_T : m_rt;
        constexpr int UNROLL = REGS ? N : 2;           // LDS forms: 2 outputs in flight (8, as the box has it, halves the generic form's occupancy)
#pragma unroll UNROLL
        for (int j = 0; j < N; j++) {                  // centre j + m, then the taps' pairs at -+ i: the order every form uses
            auto a = in(j + m) * gt.k[0];
            if (M_T > 0) {
#pragma unroll
                for (int i = 1; i <= M_T; i++) a += (in(j + m - i) + in(j + m + i)) * gt.k[i];
            } else {
                for (int i = 1; i <= m; i++) a += (in(j + m - i) + in(j + m + i)) * gt.k[i];
            }
            out(j, a);
        }
    }
    __device__ __forceinline__ void solve(float g11, float g12, float g22, float h1, float h2, float* u, float* v) const
    {
        solve_gauss_px(g11, g12, g22, h1, h2, u, v);
    }
};

// ------------------------------------------------------------------------------------------------------------
// One FarnebackUpdateFlow_Blur sweep (A.6), fused: (2m+1)^2 windowed sum of the 5 M planes -> 2x2 solve -> flow, and
// (all sweeps but the last) UpdateMatrices with the new flow -> M'.  32x32 pixel tile per 256-thread workgroup.
//   phase 1  M tile + m-pixel halo (edge-clamped = replicate border) -> LDS, 5 planes, odd row pitch
//   phase 2  vertical windowed sums, one thread per (plane, column), written back in place
//   phase 3  horizontal windowed sums, one thread per (plane, row), in place
//   phase 4  per pixel: solve, store flow; gather R1, store M'
// LDS for winsize 12: 5 x 1996 floats = 39.9 KB -> 4 workgroups (16 waves) per CU.
// ------------------------------------------------------------------------------------------------------------
static inline void iter_geometry(int m, int* ext, int* pitch, int* plane)
{
    *ext = MAV_TILE + 2 * m;
    *pitch = (*ext & 1) ? *ext : *ext + 1;          // odd pitch: phase 3 lanes (rows) hit distinct banks
    int p = *ext * *pitch;
    while ((p - *ext) % 32 != 0) p++;               // plane = ext (mod 32): phase 2 lanes stay on distinct banks across planes
    *plane = p;
}

size_t blur_iter_lds_bytes(int winsize)
{
    int ext, pitch, plane;
    iter_geometry(winsize / 2, &ext, &pitch, &plane);
    return sizeof(float) * 5 * (size_t)plane;
}

template <typename Win, int M_T>
__global__ __launch_bounds__(256) void k_blur_iter_generic(const float* __restrict__ M_in, float* __restrict__ M_out, size_t M_stride,
                                                   const float* __restrict__ R0, const float* __restrict__ R1, size_t R_stride,
                                                   int w, int h, int m_rt, int pitch, int plane, Win win, int do_update,
                                                   float* __restrict__ flow, size_t f_stride)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int m = M_T > 0 ? M_T : m_rt;
    const int ext = MAV_TILE + 2 * m;
    const int tid = threadIdx.x;
    const int s = blockIdx.z;
    const int x0 = blockIdx.x * MAV_TILE, y0 = blockIdx.y * MAV_TILE;
    const size_t npx = (size_t)w * h;
    const float* Min = M_in + (size_t)s * M_stride;

    for (int c = 0; c < 5; c++) {
        const float* P = Min + c * npx;
        float* L = lds + c * plane;
        for (int i = tid; i < ext * ext; i += 256) {
            const int ly = i / ext, lx = i - ly * ext;
            const int gx = clampi(x0 - m + lx, 0, w - 1), gy = clampi(y0 - m + ly, 0, h - 1);
            L[ly * pitch + lx] = P[(size_t)gy * w + gx];
        }
    }
    __syncthreads();
    for (int t = tid; t < 5 * ext; t += 256) {
        const int c = t / ext, lx = t - c * ext;
        float* col = lds + c * plane + lx;
        win.template sums<M_T, MAV_TILE, false>(m, [&](int i) { return col[i * pitch]; }, [&](int y, float a) { col[y * pitch] = a; });
    }
    __syncthreads();
    for (int t = tid; t < 5 * MAV_TILE; t += 256) {
        const int c = t >> 5, y = t & 31;
        float* row = lds + c * plane + y * pitch;
        win.template sums<M_T, MAV_TILE, false>(m, [&](int i) { return row[i]; }, [&](int x, float a) { row[x] = a; });
    }
    __syncthreads();
    const float* R0p = R0 + (size_t)s * R_stride;
    const float* R1p = R1 + (size_t)s * R_stride;
    float* Mo = M_out + (size_t)s * M_stride;
    float* fo = flow + (size_t)s * f_stride;
    const int lx = tid & 31;
    const int gx = x0 + lx;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ly = (tid >> 5) + 8 * j;
        const int gy = y0 + ly;
        if (gx >= w || gy >= h) continue;
        const float* L = lds + ly * pitch + lx;
        float u, v;
        win.solve(L[0], L[plane], L[2 * plane], L[3 * plane], L[4 * plane], &u, &v);
        *(float2*)(fo + ((size_t)gy * w + gx) * 2) = make_float2(u, v);
        if (do_update) update_px(R0p, R1p, npx, w, h, gx, gy, u, v, Mo);
    }
}

// ------------------------------------------------------------------------------------------------------------
// Fast form of the sweep for a compile-time half-window M_T (winsize 12 -> 6), image width a multiple of 4.
// Tile = 64 x 16 pixels per 256-thread workgroup; tiles are numbered so that the workgroups one XCD receives
// (blockIdx % 8, round-robin dispatch) walk one contiguous band of the image: halo rows are re-read from that XCD's L2.
// The kernel is built around memory latency (the v1-v3 profiles showed ~7 serialized round trips per tile):
//   entry    the R0 values phase C will need are requested first (they depend on nothing)
//   phase A  one thread per (plane, PAIR of tile columns): the 16+2m rows of its two columns arrive as float2 loads, all
//            independent and in flight together; vertical windowed sums in registers; only the 16 sums go to LDS
//   barrier  (the only one)
//   phase B  one thread per 4 consecutive pixels of a row.  Lanes are assigned by the hardware's ds_read_b128 lane
//            groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32): each group reads 16 consecutive float4 of ONE row =
//            all 64 banks once, conflict-free at any pitch.  Horizontal windowed sums, 2x2 solve.  Wave v owns tile rows
//            4v..4v+3 in phases B and C, and nobody else reads those LDS rows, so it parks its flow in the rows of planes
//            0/1 it has just finished reading: no second barrier, no extra LDS.
//   phase C  UpdateMatrices with lane = pixel column (64 consecutive pixels per wave): the R1 gathers of two pixels
//            are in flight together; R0 loads, gathers and M' stores are all row-contiguous across the wave.
// flow is stored to HBM only by a layer's last sweep (earlier sweeps' flow is consumed inside the kernel).
// LDS: 5 x (16 x 76 + 12) floats = 24.6 KB -> 6 workgroups (24 waves) per CU.  Raw M never touches LDS.
// ------------------------------------------------------------------------------------------------------------
#define FT_X 64
#define FT_Y 16

// AL = true: width a multiple of 4 and 16-byte aligned planes (vector loads / stores as written); AL = false: any width -- the
// column pairs are read as two floats at 4-byte alignment and the flow is stored pixel by pixel.
// WT = true: M' leaves the kernel through write-through (agent-scope, sc1) stores instead of staying dirty in the XCD's L2 until the
// end-of-kernel write-back.  With two launches in flight on two streams (the batch schedules) that is worth 2 % of a step -- 1080p,
// 64 pairs: 2 532 -> 2 577 pairs/s over three alternating runs, 4K / 5 layers, 16 pairs: 571 -> 583 (profiles/r03/ab_write_through.log) --
// the lines M' would occupy in L2 stay free for the M / R0 / R1 reads and no launch ends in a burst of write-backs that its
// neighbour on the other stream has to share; alone on one stream (one pair per call) the same stores cost 3 % (0.305 vs 0.297 ms
// per 1280x720 pair), so launch_blur_iter's callers ask for it in the two-stream schedules only.  Write-through for the initial M
// (k_update_matrices) and for the expansions (k_polyexp) was measured too: -0.7 % and +-0.
template <typename Win, int M_T, bool AL, bool WT>
__global__ __launch_bounds__(256) void k_blur_iter_fast(const float* __restrict__ M_in, float* __restrict__ M_out,
                                                        size_t M_stride, const float* __restrict__ R0,
                                                        const float* __restrict__ R1, size_t R_stride, int w, int h,
                                                        TileMap tm, Win win,
                                                        int do_update, int store_flow, float* __restrict__ flow, size_t f_stride)
{
    constexpr int EXT_X = FT_X + 2 * M_T;              // 76
    constexpr int EXT_Y = FT_Y + 2 * M_T;              // 28
    constexpr int PITCH = (EXT_X + 3) & ~3;            // 76
    constexpr int PLANE = FT_Y * PITCH + (EXT_X - (FT_Y * PITCH) % 32 + 64) % 32;   // = EXT_X (mod 32): phase-A lanes stay on distinct banks across planes
    static_assert(PLANE % 4 == 0 && EXT_X % 2 == 0, "plane must keep 16-byte alignment");
    __shared__ __attribute__((aligned(16))) float vs[5 * PLANE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    int s, tx, ty;                                       // XCD-aware tile order, see tile_of_block()
    if (!tile_of_block(tm, &s, &tx, &ty)) return;
    const int x0 = tx * FT_X, y0 = ty * FT_Y;
    const size_t npx = (size_t)w * h;
    const float* Min = M_in + (size_t)s * M_stride;
    const float* R0p = R0 + (size_t)s * R_stride;
    const float* R1p = R1 + (size_t)s * R_stride;

    STAMP(ts0);
    // entry: R0 of this thread's four phase-C pixels (rows 4*wv + j, column lane)
    float q[4][5];
    int gys[4];
    const int gxc = min(x0 + lane, w - 1);
    if (do_update) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            gys[j] = min(y0 + wv * 4 + j, h - 1);
            load5(R0p + 5 * ((size_t)gys[j] * w + gxc), q[j]);
        }
    }

    if (x0 >= M_T && x0 + FT_X + M_T <= w) {           // all 76 columns inside the image: float2 columns, one pass
        constexpr int NP = EXT_X / 2;                  // 38 column pairs per plane, 190 threads busy
        for (int t = tid; t < 5 * NP; t += 256) {
            const int c = t / NP, pr = t - c * NP;
            const float* col = Min + c * npx + (x0 - M_T + 2 * pr);
            float2 v[EXT_Y];
#pragma unroll
            for (int i = 0; i < EXT_Y; i++) {
                const float* pp = col + (size_t)clampi(y0 - M_T + i, 0, h - 1) * w;
                if (AL) v[i] = *(const float2*)pp;
                else { const F2U t = *(const F2U*)pp; v[i] = make_float2(t.x, t.y); }
            }
            float* out = vs + c * PLANE + 2 * pr;
            win.template sums<M_T, FT_Y, true>(M_T, [&](int i) { return v[i]; }, [&](int y, float2 a) { *(float2*)(out + y * PITCH) = a; });
        }
    } else {                                           // tiles touching the left/right image edge: clamped scalar columns
        for (int t = tid; t < 5 * EXT_X; t += 256) {
            const int c = t / EXT_X, lx = t - c * EXT_X;
            const int gx = clampi(x0 - M_T + lx, 0, w - 1);
            const float* col = Min + c * npx + gx;
            float v[EXT_Y];
#pragma unroll
            for (int i = 0; i < EXT_Y; i++) v[i] = col[(size_t)clampi(y0 - M_T + i, 0, h - 1) * w];
            float* out = vs + c * PLANE + lx;
            win.template sums<M_T, FT_Y, true>(M_T, [&](int i) { return v[i]; }, [&](int y, float a) { out[y * PITCH] = a; });
        }
    }
    STAMP(ts1);
    __syncthreads();
    STAMP(ts2);

    {
        // hardware b128 lane group (quads of 4 lanes: g0 = quads {0,3,5,6}, g1 = quads {1,2,4,7}, +2 for lanes 32..63)
        const int quad = (lane & 31) >> 2;
        const int grp = (lane >> 5) * 2 + ((quad == 1 || quad == 2 || quad == 4 || quad == 7) ? 1 : 0);
        const int qpos = (quad == 0 || quad == 1) ? 0 : ((quad == 3 || quad == 2) ? 1 : ((quad == 5 || quad == 4) ? 2 : 3));
        const int pos = qpos * 4 + (lane & 3);          // 0..15 inside the group
        const int ly = wv * 4 + grp;                     // tile row 0..15
        const int lx0 = pos * 4;
        const int gx = x0 + lx0, gy = y0 + ly;
        float S[5][4];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const float4* p = (const float4*)(vs + c * PLANE + ly * PITCH + lx0);
            constexpr int NV = (4 + 2 * M_T + 3) / 4;
            float f[4 * NV];
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const float4 t4 = p[k];
                f[4 * k] = t4.x; f[4 * k + 1] = t4.y; f[4 * k + 2] = t4.z; f[4 * k + 3] = t4.w;
            }
            win.template sums<M_T, 4, true>(M_T, [&](int i) { return f[i]; }, [&](int j, float a) { S[c][j] = a; });
        }
        float u[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) win.solve(S[0][j], S[1][j], S[2][j], S[3][j], S[4][j], &u[j], &v[j]);
        if (store_flow && gx < w && gy < h) {
            float* fo = flow + (size_t)s * f_stride + ((size_t)gy * w + gx) * 2;
            if (AL) {                                        // w % 4 == 0: the 4 pixels are all inside or all outside
                *(float4*)fo = make_float4(u[0], v[0], u[1], v[1]);
                *(float4*)(fo + 4) = make_float4(u[2], v[2], u[3], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (gx + j < w) *(float2*)(fo + 2 * j) = make_float2(u[j], v[j]);
            }
        }
        if (!do_update) return;
        // park the flow in this wave's own rows of planes 0 (u) and 1 (v); every read of those rows by this wave is
        // older in program order, and no other wave touches them
        *(float4*)(vs + ly * PITCH + lx0) = make_float4(u[0], u[1], u[2], u[3]);
        *(float4*)(vs + PLANE + ly * PITCH + lx0) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    STAMP(ts3);

    float* Mo = M_out + (size_t)s * M_stride;
    const bool colok = x0 + lane < w;
#pragma unroll
    for (int jb = 0; jb < 4; jb += 2) {
        GatherPx g[2];
        float fu[2], fv[2];
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const int ly = wv * 4 + jb + jj;
            fu[jj] = vs[ly * PITCH + lane];
            fv[jj] = vs[PLANE + ly * PITCH + lane];
            gather_issue(R1p, w, h, gxc, gys[jb + jj], fu[jj], fv[jj], g[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            float o[5];
            update_finish(q[jb + jj], g[jj], w, h, gxc, gys[jb + jj], fu[jj], fv[jj], o);
            if (colok && y0 + wv * 4 + jb + jj < h) {
                const size_t idx = (size_t)gys[jb + jj] * w + gxc;
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    if constexpr (WT) __hip_atomic_store((unsigned*)(Mo + c * npx + idx), __float_as_uint(o[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else Mo[c * npx + idx] = o[c];
                }
            }
        }
#ifdef MAV_STAMPS
        if (jb == 0) { STAMP(tsm); STAMP_ADD(3, ts3, tsm); STAMP_ADD(5, tsm, tsm); }
#endif
    }
    STAMP(ts4);
    STAMP_ADD(0, ts0, ts1); STAMP_ADD(1, ts1, ts2); STAMP_ADD(2, ts2, ts3); STAMP_ADD(4, ts3, ts4); STAMP_ADD(6, ts0, ts4); STAMP_ADD(7, 0ull, 1ull);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int blur_iter_tile_rows(int h) { return (h + FT_Y - 1) / FT_Y; }
static bool blur_iter_vec_ok(const SweepArgs& a)
{
    return (a.w % 4 == 0) && (a.M_stride % 4 == 0) && (a.R_stride % 4 == 0) && (a.f_stride % 4 == 0) && aligned16(a.M_in) && aligned16(a.M_out) &&
           aligned16(a.R0) && aligned16(a.R1) && aligned16(a.flow);
}
bool blur_iter_bands_ok(const SweepArgs& a) { return a.winsize / 2 == 6 && blur_iter_vec_ok(a); }

// the fast form's launch
template <typename Win, bool AL>
static void launch_sweep_fast(hipStream_t st, const TileMap& tm, const SweepArgs& a, const Win& win)
{
    const bool wt = a.write_through && a.do_update;      // M' through write-through stores
    const auto k = wt ? k_blur_iter_fast<Win, 6, AL, true> : k_blur_iter_fast<Win, 6, AL, false>;
    hipLaunchKernelGGL(k, dim3(tile_grid(tm)), dim3(256), 0, st, a.M_in, a.M_out, a.M_stride, a.R0, a.R1, a.R_stride, a.w, a.h, tm, win,
                       a.do_update, a.store_flow, a.flow, a.f_stride);
}

// One sweep launch of either window, three tiers: the fast form as written (AL), its relaxed form for any width / alignment, the
// generic form.
template <typename Win>
static void launch_sweep(hipStream_t st, const SweepArgs& a, const Win& win)
{
    const int m = a.winsize / 2;
    if (m == 6 && blur_iter_vec_ok(a)) {
        const TileMap tm = make_tile_map(a.w, a.h, a.G, FT_X, FT_Y, a.ty0, a.ty1, a.strip);
        if (tm.n_tiles == 0) return;
        return launch_sweep_fast<Win, true>(st, tm, a, win);
    }
    if (m == 6 && a.f_stride % 2 == 0 && ((uintptr_t)a.flow & 7) == 0)      // any width / alignment: relaxed form of the same kernel
        return launch_sweep_fast<Win, false>(st, make_tile_map(a.w, a.h, a.G, FT_X, FT_Y, 0, -1, a.strip), a, win);
    int ext, pitch, plane;
    iter_geometry(m, &ext, &pitch, &plane);
    const size_t lds = sizeof(float) * 5 * (size_t)plane;
    const dim3 grid((a.w + MAV_TILE - 1) / MAV_TILE, (a.h + MAV_TILE - 1) / MAV_TILE, a.G);
    // m != 6: dynamic LDS above the default limit was granted by blur_iter_prepare() when the context was created
    const auto k = m == 6 ? k_blur_iter_generic<Win, 6> : k_blur_iter_generic<Win, 0>;
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, a.M_in, a.M_out, a.M_stride, a.R0, a.R1, a.R_stride, a.w, a.h, m, pitch, plane, win,
                       a.do_update, a.flow, a.f_stride);
}

// tile rows [a.ty0, a.ty1) only (ty1 < 0: the whole layer).  Band launches exist for the fast form only (blur_iter_bands_ok).
void launch_blur_iter(hipStream_t st, const SweepArgs& a)
{
    if (a.gauss) launch_sweep(st, a, GaussWindow{*a.gauss});
    else launch_sweep(st, a, BoxWindow{(float)(1.0 / ((double)a.winsize * a.winsize))});
}

// The general-winsize sweep needs 5 x (32 + 2m)^2 floats of dynamic LDS; above the 64 KB default a kernel must be granted
// the size on every device it runs on.  Called by mav_create on the context's device; returns an error text or nullptr.
const char* blur_iter_prepare(int winsize)
{
    const size_t lds = blur_iter_lds_bytes(winsize);
    if (lds <= (size_t)64 * 1024) return nullptr;
    hipError_t e = hipFuncSetAttribute((const void*)k_blur_iter_generic<BoxWindow, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_blur_iter_generic<GaussWindow, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ------------------------------------------------------------------------------------------------------------
// Calibration (mav_membw_probe, bench.py's `measured_ceiling`): what the memory system delivers to a plain streaming kernel with
// the sweeps' mix of 3 reads : 1 write (M, R0, R1 in; M' out), one float4 per thread and step, grid-stride.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_probe_r3w1(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ c,
                                                    float4* __restrict__ d, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float4 x = a[i], y = b[i], z = c[i];
        d[i] = make_float4(x.x + y.x + z.x, x.y + y.y + z.y, x.z + y.z + z.z, x.w + y.w + z.w);
    }
}
void launch_probe_r3w1(hipStream_t st, const float* a, const float* b, const float* c, float* d, size_t n_float4)
{
    hipLaunchKernelGGL(k_probe_r3w1, dim3(256 * 8), dim3(256), 0, st, (const float4*)a, (const float4*)b, (const float4*)c, (float4*)d, n_float4);
}

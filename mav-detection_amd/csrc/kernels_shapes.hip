// Shapes on the device (include/mavflow_shapes.h, whose text is the definition): a table of lines, rectangles and filled circles drawn in
// table order, cv2.add, blob records -> rectangles, and the tile mosaic.  gfx950, wave64.  Compiled with -ffp-contract=off: the thick
// line's half-width is float64 arithmetic in a fixed order (correctly rounded '/' and sqrt), everything else is integer arithmetic.
// This unit holds its own host side: the entry points of the header, at the end.
//
// Every record is a set of row spans that are a closed form of the row, so rows are independent work.  ONE WAVE takes a (record, part)
// item (k_shapes_rows: a rectangle outline's four lines, or a quarter of another record's rows) and walks its rows: short spans one row
// per lane, long spans one row per wave with the span's pixels on consecutive lanes.  Waves stride over the items of the grid.
// ORDERED: a lane's "draw" is atomicMax(plane[pixel], index + 1) and a second pass over the
// pixels writes the colour of the recorded index; DIRECT: it stores the colour.  Every index is range-checked before it is used: a span
// is clipped to 0 .. W - 1, a row to 0 .. H - 1, a record's image is checked against the batch, and the plane's words are <= the count
// pass A ran with.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mavflow_internal.h"
#include "../../include/mavflow_shapes.h"

#define SH_WG 256
#define SH_WAVES (SH_WG / 64)
#define SH_ONE 65536ll
#define SH_HALF 32768ll

static_assert(sizeof(mav_shape) == 32, "mav_shape");

struct ShapeDraw { uint8_t* img; const mav_shape* shapes; const int32_t* n_dev; int32_t* plane; int n_max, W, H, B, C; };

// the records the header says are skipped
__host__ __device__ inline bool sh_coord_ok(int v) { return v >= -MAV_SHAPE_MAX_COORD && v <= MAV_SHAPE_MAX_COORD; }
__host__ __device__ inline bool sh_valid(const mav_shape& s, int batch)
{
    if (s.image < 0 || s.image >= batch) return false;
    if (!sh_coord_ok(s.x0) || !sh_coord_ok(s.y0) || !sh_coord_ok(s.x1) || !sh_coord_ok(s.y1)) return false;
    const bool thick = s.thickness >= 1 && s.thickness <= MAV_SHAPE_MAX_THICKNESS;
    switch (s.kind) {
    case MAV_SHAPE_LINE: return thick;
    case MAV_SHAPE_RECT: return thick || s.thickness == MAV_SHAPE_FILLED;
    case MAV_SHAPE_CIRCLE: return s.thickness == MAV_SHAPE_FILLED && s.x1 >= 0;
    default: return false;
    }
}
__device__ __forceinline__ int sh_count(const ShapeDraw& k)
{
    if (!k.n_dev) return k.n_max;
    const int n = *k.n_dev;
    return n < 0 || n > k.n_max ? 0 : n;
}
// What a lane does with the pixels of a span
template <bool ORDERED>
struct ShapeSink {
    uint8_t* row;          // the image row (DIRECT)
    int32_t* prow;         // the plane's row (ORDERED)
    int W, C, first, step, tag;    // a span's pixels first, first + step, ...: (lane, 64) across a wave, (0, 1) for a lane alone
    uint32_t colour;
    __device__ __forceinline__ void span(long long xa, long long xb) const
    {
        if (xa < 0) xa = 0;
        if (xb > W - 1) xb = W - 1;
        for (long long x = xa + first; x <= xb; x += step) {
            if constexpr (ORDERED) atomicMax(prow + x, tag);
            else {
                uint8_t* q = row + (size_t)x * C;
                q[0] = (uint8_t)colour;
                if (C == 3) { q[1] = (uint8_t)(colour >> 8); q[2] = (uint8_t)(colour >> 16); }
            }
        }
    }
};

// cv::clipLine on int64 points (mavflow_vis.h); false: nothing of the segment is inside
__device__ __forceinline__ bool sh_clip_line(long long W, long long H, long long& x1, long long& y1, long long& x2, long long& y2)
{
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}
// row y of the thickness-1 line: the LineIterator's pixels by rows
template <typename Sink>
__device__ __forceinline__ void sh_thin_line(const Sink& sk, int W, int H, long long x1, long long y1, long long x2, long long y2, int y)
{
    if (!sh_clip_line(W, H, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
    const long long sy = dy < 0 ? -1 : 1;
    if (dy < 0) dy = -dy;
    if (dy > dx) {                                                       // one pixel per row
        const long long i = (y - y1) * sy;
        if (i < 0 || i > dy) return;
        const long long x = x1 + (2 * dx * i + dy - 1) / (2 * dy);       // dy > dx >= 0: dy >= 1, the numerator is >= 0
        sk.span(x, x);
    } else {
        const long long d = (y - y1) * sy;
        if (d < 0 || d > dy) return;
        if (dy == 0) { sk.span(x1, x1 + dx); return; }
        const long long lo = d == 0 ? 0 : (2 * dx * (d - 1) + dx) / (2 * dy) + 1;
        long long hi = (2 * dx * d + dx) / (2 * dy);
        if (hi > dx) hi = dx;
        if (lo <= hi) sk.span(x1 + lo, x1 + hi);
    }
}
// the half-width of row offset k of the filled circle of radius r (0 <= k <= r).  The midpoint walk of the header keeps
// err = dx^2 + dy^2 - r^2 and lowers dx by one exactly when that is positive, and in the octant dx >= dy one step is always enough: so
// dx at row dy is floor(sqrt(r^2 - dy^2)), every row's widest span is floor(sqrt(r^2 - k^2)), and no row is left empty.
// (tests/test_shapes_cases_cpu.py holds this closed form to the walk.)  r <= 2^20: r^2 - k^2 is exact in int64 and in double.
__device__ __forceinline__ long long sh_disc_half_width(long long r, long long k)
{
    const long long v = r * r - k * k;
    long long h = (long long)sqrt((double)v);
    while (h * h > v) h--;
    while ((h + 1) * (h + 1) <= v) h++;
    return h;
}
template <typename Sink>
__device__ __forceinline__ void sh_disc(const Sink& sk, long long cx, long long cy, int r, int y)
{
    const long long k = y < cy ? cy - y : y - cy;
    if (k > r) return;
    const long long h = sh_disc_half_width(r, k);
    sk.span(cx - h, cx + h);
}
// one chain's x at row y of the convex fill: vx, vy the vertices, rw their rows, m the start, di = 1 or 3
__device__ __forceinline__ long long sh_chain_x(const long long* vx, const long long* rw, int m, int di, long long ymin, long long y)
{
    long long X = -SH_ONE, D = 0, Y = ymin, ys = ymin;
    int c = 0;
    for (;;) {
        int k = c + 1;
        while (k <= 3 && rw[(m + k * di) & 3] <= ys) k++;
        if (k > 3) break;
        const long long ty = rw[(m + k * di) & 3], xs = vx[(m + (k - 1) * di) & 3], xe = vx[(m + k * di) & 3];
        D = ((xe - xs) * 2 + (ty - ys)) / (2 * (ty - ys));              // truncated toward zero
        X = xs; Y = ys; c = k;
        if (y < ty) break;
        ys = ty;
    }
    return X + (y - Y) * D;
}
// row y of the line (x0, y0) - (x1, y1) of thickness t
template <typename Sink>
__device__ void sh_line(const Sink& sk, int W, int H, long long x0, long long y0, long long x1, long long y1, int t, int y)
{
    if (t <= 1) { sh_thin_line(sk, W, H, x0, y0, x1, y1, y); return; }
    const int cap = (int)(((long long)t * SH_HALF + SH_HALF) >> 16);
    if (y < (y0 < y1 ? y0 : y1) - t - 2 || y > (y0 > y1 ? y0 : y1) + t + 2) return;      // beyond the half-width (< t / 2 + 1) and the caps
    const double dx = (double)(x0 - x1), dy = (double)(y1 - y0);
    const double r = dx * dx + dy * dy;
    if (r > DBL_EPSILON) {
        const double s = ((double)((long long)t << 15) + (double)((long long)(t & 1) << 15)) / sqrt(r);
        const long long dpx = (long long)rint(dy * s), dpy = (long long)rint(dx * s);
        const long long X0 = x0 * SH_ONE, Y0 = y0 * SH_ONE, X1 = x1 * SH_ONE, Y1 = y1 * SH_ONE;
        const long long vx[4] = {X0 + dpx, X0 - dpx, X1 - dpx, X1 + dpx};
        const long long vy[4] = {Y0 + dpy, Y0 - dpy, Y1 - dpy, Y1 + dpy};
        long long rw[4], ymax;
        int m = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { rw[i] = (vy[i] + SH_HALF) >> 16; if (vy[i] < vy[m]) m = i; }
        ymax = rw[0];
#pragma unroll
        for (int i = 1; i < 4; i++) if (rw[i] > ymax) ymax = rw[i];
        const long long ymin = rw[m];
        if (y >= ymin && y <= ymax) {
            long long xa = sh_chain_x(vx, rw, m, 1, ymin, y), xb = sh_chain_x(vx, rw, m, 3, ymin, y);
            if (xa > xb) { const long long q = xa; xa = xb; xb = q; }
            sk.span((xa + SH_HALF) >> 16, (xb + SH_HALF) >> 16);
        }
    }
    sh_disc(sk, x0, y0, cap, y);
    sh_disc(sk, x1, y1, cap, y);
}
// row y of one primitive: a LINE, a filled RECT or a CIRCLE
template <typename Sink>
__device__ void sh_record_row(const Sink& sk, const mav_shape& s, int W, int H, int y)
{
    switch (s.kind) {
    case MAV_SHAPE_LINE:
        sh_line(sk, W, H, s.x0, s.y0, s.x1, s.y1, s.thickness, y);
        break;
    case MAV_SHAPE_RECT:
        {                                                               // filled: k_shapes_rows hands an outline over as its four lines
            const int ya = min(s.y0, s.y1), yb = max(s.y0, s.y1);
            if (y >= ya && y <= yb) sk.span(min(s.x0, s.x1), max(s.x0, s.x1));
        }
        break;
    case MAV_SHAPE_CIRCLE:
        sh_disc(sk, s.x0, s.y0, s.x1, y);
        break;
    }
}

// The clipped rows a primitive (a LINE, a filled RECT or a CIRCLE) can reach; empty when *ya > *yb
__device__ __forceinline__ void sh_prim_rows(const mav_shape& q, int H, int* ya, int* yb)
{
    long long a, b;
    if (q.kind == MAV_SHAPE_CIRCLE) { a = (long long)q.y0 - q.x1; b = (long long)q.y0 + q.x1; }
    else {
        const long long ext = q.kind == MAV_SHAPE_LINE && q.thickness > 1 ? (q.thickness + 1) / 2 + 2 : 0;      // half-width, rounding, caps
        a = min(q.y0, q.y1) - ext; b = max(q.y0, q.y1) + ext;
    }
    *ya = (int)(a < 0 ? 0 : a);
    *yb = (int)(b > H - 1 ? H - 1 : b);
}
// pass A (ORDERED) or the whole drawing (DIRECT).  The work item is (record, part), part 0 .. 3, one WAVE each, waves striding over the
// items: a rectangle's outline is its four lines, one per part; every other record is one primitive whose rows are dealt to the four
// parts in quarters.  A primitive whose spans are short (a line that is neither thick nor shallow) gives each LANE a row, and the lane
// stores its few pixels itself; any other gives the wave one row at a time and a span's pixels go to consecutive lanes.  The pixels
// are the same either way.
template <bool ORDERED>
__global__ __launch_bounds__(SH_WG) void k_shapes_rows(const ShapeDraw k)
{
    const int n = sh_count(k), lane = threadIdx.x & 63;
    const unsigned long long items = (unsigned long long)n * 4;
    const unsigned long long stride = (unsigned long long)gridDim.x * SH_WAVES;
    const size_t n0 = (size_t)k.W * k.H;
    for (unsigned long long it = (unsigned long long)blockIdx.x * SH_WAVES + (threadIdx.x >> 6); it < items; it += stride) {
        const int i = (int)(it >> 2), part = (int)(it & 3);             // i < n <= n_max
        const mav_shape s = k.shapes[i];
        if (!sh_valid(s, k.B)) continue;
        mav_shape q = s;                                                // the part's primitive
        const bool outline = s.kind == MAV_SHAPE_RECT && s.thickness != MAV_SHAPE_FILLED;
        if (outline) {
            q.kind = MAV_SHAPE_LINE;
            q.x0 = part == 0 || part == 3 ? (part == 0 ? s.x0 : s.x1) : (part == 1 ? s.x0 : s.x1);
            q.y0 = part == 0 || part == 3 ? s.y1 : s.y0;
            q.x1 = part == 0 || part == 1 ? (part == 0 ? s.x0 : s.x1) : (part == 2 ? s.x1 : s.x0);
            q.y1 = part == 0 || part == 1 ? s.y0 : s.y1;
        }
        int ya, yb;
        sh_prim_rows(q, k.H, &ya, &yb);
        if (!outline) {                                                 // this part's quarter of the rows
            const int per = (yb - ya + 1 + 3) / 4;
            ya += part * per;
            yb = min(yb, ya + per - 1);
        }
        if (ya > yb) continue;
        const long long adx = q.x0 < q.x1 ? (long long)q.x1 - q.x0 : (long long)q.x0 - q.x1;
        const long long ady = q.y0 < q.y1 ? (long long)q.y1 - q.y0 : (long long)q.y0 - q.y1;
        const bool by_rows = q.kind == MAV_SHAPE_LINE && q.thickness <= 16 && q.thickness + 3 + adx / (ady > 1 ? ady : 1) <= 32;
        ShapeSink<ORDERED> sk;
        sk.W = k.W; sk.C = k.C; sk.tag = i + 1;
        sk.first = by_rows ? 0 : lane; sk.step = by_rows ? 1 : 64;
        sk.colour = (uint32_t)s.colour[0] | ((uint32_t)s.colour[1] << 8) | ((uint32_t)s.colour[2] << 16);
        const size_t image = n0 * (size_t)s.image;
        for (int base = ya; base <= yb; base += by_rows ? 64 : 1) {
            const int y = by_rows ? base + lane : base;                 // ya >= 0, yb <= H - 1
            if (y > yb) continue;
            const size_t row = image + (size_t)y * k.W;
            sk.row = ORDERED ? nullptr : k.img + row * k.C;
            sk.prow = ORDERED ? k.plane + row : nullptr;
            sh_record_row(sk, q, k.W, k.H, y);
        }
    }
}
// pass B: the colour of the recorded record, where there is one
__global__ __launch_bounds__(SH_WG) void k_shapes_resolve(const ShapeDraw k)
{
    const int n = sh_count(k);
    const size_t N = (size_t)k.W * k.H * k.B, stride = (size_t)gridDim.x * SH_WG;
    for (size_t p = (size_t)blockIdx.x * SH_WG + threadIdx.x; p < N; p += stride) {
        const int v = k.plane[p];
        if (v < 1 || v > n) continue;                                    // pass A wrote nothing else; checked all the same
        const mav_shape* s = k.shapes + (v - 1);
        uint8_t* q = k.img + p * k.C;
        q[0] = s->colour[0];
        if (k.C == 3) { q[1] = s->colour[1]; q[2] = s->colour[2]; }
    }
}

// ---- cv2.add ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sh_add4(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const uint32_t s = ((a >> i) & 255u) + ((b >> i) & 255u);
        r |= (s > 255u ? 255u : s) << i;
    }
    return r;
}
// threads 0 .. G - 1 own 16 bytes, threads G .. G + (n - 16 G) - 1 one of the last bytes (G = 0: the BYTES form)
__global__ __launch_bounds__(SH_WG) void k_add_saturate(const uint8_t* a, const uint8_t* b, uint8_t* dst, size_t n, size_t G)
{
    const size_t t = (size_t)blockIdx.x * SH_WG + threadIdx.x;
    if (t < G) {
        const uint4 x = ((const uint4*)a)[t], y = ((const uint4*)b)[t];
        ((uint4*)dst)[t] = make_uint4(sh_add4(x.x, y.x), sh_add4(x.y, y.y), sh_add4(x.z, y.z), sh_add4(x.w, y.w));
    } else {
        const size_t p = 16 * G + (t - G);
        if (p >= n) return;
        const unsigned s = (unsigned)a[p] + b[p];
        dst[p] = (uint8_t)(s > 255u ? 255u : s);
    }
}

// ---- blob records -> rectangles ---------------------------------------------------------------------------------------------------------
__global__ void k_shapes_from_blobs(const mav_blob* blobs, const mav_cc_counts* counts, int B, int max_blobs, int thickness, uint32_t colour,
                                    mav_shape* out, int32_t* n_out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * max_blobs) return;
    const int b = t / max_blobs, j = t - b * max_blobs;
    int first = 0, mine = 0;
    for (int i = 0; i < B; i++) {                                       // images in front of this one; the last thread's sum is the total
        const int c = min(max(counts[i].n_blobs, 0), max_blobs);
        if (i < b) first += c;
        if (i == b) mine = c;
    }
    if (t == 0) {
        int total = 0;
        for (int i = 0; i < B; i++) total += min(max(counts[i].n_blobs, 0), max_blobs);
        *n_out = total;
    }
    if (j >= mine) return;
    const mav_blob q = blobs[(size_t)b * max_blobs + j];
    mav_shape s;
    s.kind = MAV_SHAPE_RECT; s.image = b; s.x0 = q.x; s.y0 = q.y; s.x1 = q.x + q.w - 1; s.y1 = q.y + q.h - 1; s.thickness = thickness;
    s.colour[0] = (uint8_t)colour; s.colour[1] = (uint8_t)(colour >> 8); s.colour[2] = (uint8_t)(colour >> 16); s.colour[3] = (uint8_t)(colour >> 24);
    out[first + j] = s;                                                 // first + j < B * max_blobs
}

// ---- mosaic -------------------------------------------------------------------------------------------------------------------------------
struct Mosaic { const uint8_t* tile[MAV_MOSAIC_MAX_TILES]; int ch[MAV_MOSAIC_MAX_TILES]; int rows, cols, W, H, B; uint8_t* out; };
__device__ __forceinline__ uint8_t sh_mosaic_byte(const Mosaic& m, size_t o)          // byte o of out
{
    const size_t rowb = (size_t)m.cols * m.W * 3, imgb = rowb * m.rows * m.H;
    const size_t b = o / imgb, r0 = o - b * imgb, Y = r0 / rowb, xb = r0 - Y * rowb, X = xb / 3, c = xb - X * 3;
    const size_t tr = Y / m.H, y = Y - tr * m.H, tc = X / m.W, x = X - tc * m.W;
    const int ti = (int)(tr * m.cols + tc);                             // < rows * cols
    const uint8_t* src = m.tile[ti];
    if (!src) return 0;
    const size_t px = (b * m.H + y) * m.W + x;
    return m.ch[ti] == 1 ? src[px] : src[px * 3 + c];
}
__global__ __launch_bounds__(SH_WG) void k_mosaic(const Mosaic m, size_t n, size_t G)
{
    const size_t t = (size_t)blockIdx.x * SH_WG + threadIdx.x;
    if (t < G) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const size_t o = 16 * t + 4 * i;
            w[i] = (uint32_t)sh_mosaic_byte(m, o) | ((uint32_t)sh_mosaic_byte(m, o + 1) << 8) | ((uint32_t)sh_mosaic_byte(m, o + 2) << 16) |
                   ((uint32_t)sh_mosaic_byte(m, o + 3) << 24);
        }
        ((uint4*)m.out)[t] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const size_t p = 16 * G + (t - G);
        if (p < n) m.out[p] = sh_mosaic_byte(m, p);
    }
}

// ---- n bytes of one value in the caller's memory (mav_motion_pictures_dev's mode bytes) ----------------------------------------------------
__global__ void k_fill_bytes(uint8_t* p, uint8_t value, size_t n)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = value;
}
void launch_fill_bytes(hipStream_t st, uint8_t* p, uint8_t value, size_t n)
{
    if (n) hipLaunchKernelGGL(k_fill_bytes, dim3((unsigned)((n + SH_WG - 1) / SH_WG)), dim3(SH_WG), 0, st, p, value, n);
}

// ---- host side: the entry points of include/mavflow_shapes.h ----------------------------------------------------------------------------
#define SCHK(call) do { const int rc_ = (call); if (rc_ != MAV_OK) return rc_; } while (0)

static unsigned sh_grid(size_t threads, size_t cap)
{
    size_t g = (threads + SH_WG - 1) / SH_WG;
    if (g > cap) g = cap;
    return (unsigned)(g ? g : 1);
}
extern "C" size_t mav_shapes_scratch_bytes(int W, int H, int batch)
{
    return W < 1 || H < 1 || batch < 1 ? 0 : sizeof(int32_t) * (size_t)W * H * batch;
}
extern "C" int mav_shapes_form(const mav_shape* shapes, int n, int channels)
{
    if (n < 0 || (n > 0 && !shapes) || (channels != 1 && channels != 3)) return -1;
    for (int i = 1; i < n; i++)
        for (int c = 0; c < channels; c++)
            if (shapes[i].colour[c] != shapes[0].colour[c]) return MAV_SHAPES_FORM_ORDERED;
    return MAV_SHAPES_FORM_DIRECT;
}
extern "C" int mav_bytes_form(size_t n, const void* a, const void* b, const void* dst)
{
    if (n < 1) return -1;
    return n >= 16 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)dst) % 16 == 0 ? MAV_SHAPES_FORM_WORDS : MAV_SHAPES_FORM_BYTES;
}

// what both forms of mav_draw_shapes are refused for before the context's device is looked at (the batch is check_dev_call's)
static int draw_shapes_checked(mav_ctx* c, const void* img, int channels, const void* shapes, int n, const char* fn)
{
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!img) return ctx_fail(MAV_ERR_ARG, "%s: NULL img", fn);
    if (channels != 1 && channels != 3) return ctx_fail(MAV_ERR_ARG, "%s: channels %d is neither 1 nor 3", fn, channels);
    if (n < 0) return ctx_fail(MAV_ERR_ARG, "%s: %d records", fn, n);
    if (n > 0 && !shapes) return ctx_fail(MAV_ERR_ARG, "%s: NULL shapes", fn);
    return MAV_OK;
}
static int sh_pixels_checked(const CtxView& v, int batch, const char* fn)
{
    if ((uint64_t)v.W * v.H * (uint64_t)batch > 0x7FFFFFFFull)
        return ctx_fail(MAV_ERR_ARG, "%s: %d images of %d x %d are more than 2^31 - 1 pixels", fn, batch, v.W, v.H);
    return MAV_OK;
}
// the launches of one drawing; plane == NULL: DIRECT
static int draw_shapes_launch(mav_ctx* c, const CtxView& v, uint8_t* img, int channels, int batch, const mav_shape* shapes, int n_max,
                              const int32_t* n_dev, int32_t* plane, const char* fn)
{
    if (n_max == 0) return MAV_OK;
    const ShapeDraw k = {img, shapes, n_dev, plane, n_max, v.W, v.H, batch, channels};
    const size_t N = (size_t)v.W * v.H * batch;
    const unsigned rows_grid = sh_grid((size_t)n_max * 4 * 64, 8192);
    MiscScope ps(c);
    if (plane) {
        const hipError_t e = hipMemsetAsync(plane, 0, sizeof(int32_t) * N, v.stream);
        if (e != hipSuccess) return ctx_fail(MAV_ERR_HIP, "%s: clearing the plane failed: %s", fn, hipGetErrorString(e));
        hipLaunchKernelGGL(k_shapes_rows<true>, dim3(rows_grid), dim3(SH_WG), 0, v.stream, k);
        hipLaunchKernelGGL(k_shapes_resolve, dim3(sh_grid(N, 4096)), dim3(SH_WG), 0, v.stream, k);
    } else {
        hipLaunchKernelGGL(k_shapes_rows<false>, dim3(rows_grid), dim3(SH_WG), 0, v.stream, k);
    }
    return ctx_check_launch("draw_shapes");
}
extern "C" int mav_draw_shapes_dev(mav_ctx* c, uint8_t* img, int channels, int batch, const mav_shape* shapes, int n_max, const int32_t* n_dev,
                                   void* scratch)
{
    const char* fn = "mav_draw_shapes_dev";
    SCHK(draw_shapes_checked(c, img, channels, shapes, n_max, fn));
    if ((uintptr_t)shapes % 4 || (uintptr_t)n_dev % 4 || (uintptr_t)scratch % 4)
        return ctx_fail(MAV_ERR_ARG, "%s: shapes, n_dev and scratch must be aligned to 4", fn);
    CtxView v;
    SCHK(ctx_enter(c, batch, fn, &v));
    SCHK(sh_pixels_checked(v, batch, fn));
    return draw_shapes_launch(c, v, img, channels, batch, shapes, n_max, n_dev, (int32_t*)scratch, fn);
}
extern "C" int mav_draw_shapes(mav_ctx* c, uint8_t* img, int channels, int batch, const mav_shape* shapes, int n)
{
    const char* fn = "mav_draw_shapes";
    SCHK(draw_shapes_checked(c, img, channels, shapes, n, fn));
    StagedCall h(c, fn);
    CtxView v;
    SCHK(h.begin(batch, &v));
    SCHK(sh_pixels_checked(v, batch, fn));
    for (int i = 0; i < n; i++)
        if (!sh_valid(shapes[i], batch))
            return ctx_fail(MAV_ERR_ARG, "%s: record %d (kind %d, image %d, (%d, %d) - (%d, %d), thickness %d) is not one this call draws", fn, i,
                            shapes[i].kind, shapes[i].image, shapes[i].x0, shapes[i].y0, shapes[i].x1, shapes[i].y1, shapes[i].thickness);
    if (n == 0) return MAV_OK;
    const size_t bytes = (size_t)v.W * v.H * batch * channels;
    uint8_t* di = (uint8_t*)h.inout(img, bytes);
    const mav_shape* ds = (const mav_shape*)h.in(shapes, sizeof(mav_shape) * (size_t)n);
    int32_t* plane = mav_shapes_form(shapes, n, channels) == MAV_SHAPES_FORM_ORDERED ? (int32_t*)h.scratch(mav_shapes_scratch_bytes(v.W, v.H, batch)) : nullptr;
    SCHK(h.staged());
    SCHK(draw_shapes_launch(c, v, di, channels, batch, ds, n, nullptr, plane, fn));
    return h.finish();
}

static int add_checked(mav_ctx* c, const void* a, const void* b, int channels, const void* dst, const char* fn)
{
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!a || !b || !dst) return ctx_fail(MAV_ERR_ARG, "%s: NULL %s", fn, !a ? "a" : !b ? "b" : "dst");
    if (channels < 1 || channels > 4) return ctx_fail(MAV_ERR_ARG, "%s: channels %d outside [1, 4]", fn, channels);
    return MAV_OK;
}
static int add_launch(mav_ctx* c, const CtxView& v, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* dst)
{
    const size_t G = mav_bytes_form(n, a, b, dst) == MAV_SHAPES_FORM_WORDS ? n / 16 : 0, T = G + (n - 16 * G);
    MiscScope ps(c);
    hipLaunchKernelGGL(k_add_saturate, dim3((unsigned)((T + SH_WG - 1) / SH_WG)), dim3(SH_WG), 0, v.stream, a, b, dst, n, G);
    return ctx_check_launch("add_saturate");
}
extern "C" int mav_add_saturate_dev(mav_ctx* c, const uint8_t* a, const uint8_t* b, int channels, int batch, uint8_t* dst)
{
    const char* fn = "mav_add_saturate_dev";
    SCHK(add_checked(c, a, b, channels, dst, fn));
    CtxView v;
    SCHK(ctx_enter(c, batch, fn, &v));
    SCHK(sh_pixels_checked(v, batch, fn));
    return add_launch(c, v, a, b, (size_t)v.W * v.H * batch * channels, dst);
}
extern "C" int mav_add_saturate(mav_ctx* c, const uint8_t* a, const uint8_t* b, int channels, int batch, uint8_t* dst)
{
    const char* fn = "mav_add_saturate";
    SCHK(add_checked(c, a, b, channels, dst, fn));
    StagedCall h(c, fn);
    CtxView v;
    SCHK(h.begin(batch, &v));
    SCHK(sh_pixels_checked(v, batch, fn));
    const size_t n = (size_t)v.W * v.H * batch * channels;
    const uint8_t* da = (const uint8_t*)h.in(a, n);
    const uint8_t* db = (const uint8_t*)h.in(b, n);
    uint8_t* dd = (uint8_t*)h.out(dst, n);
    SCHK(h.staged());
    SCHK(add_launch(c, v, da, db, n, dd));
    return h.finish();
}

extern "C" int mav_shapes_from_blobs_dev(mav_ctx* c, const mav_blob* blobs, const mav_cc_counts* counts, int batch, int max_blobs, int thickness,
                                         const uint8_t* colour, mav_shape* out, int32_t* n_out)
{
    const char* fn = "mav_shapes_from_blobs_dev";
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!blobs || !counts || !colour || !out || !n_out) return ctx_fail(MAV_ERR_ARG, "%s: NULL argument", fn);
    if (max_blobs < 1 || max_blobs > (1 << 20)) return ctx_fail(MAV_ERR_ARG, "%s: max_blobs %d outside [1, 2^20]", fn, max_blobs);
    if (thickness != MAV_SHAPE_FILLED && (thickness < 1 || thickness > MAV_SHAPE_MAX_THICKNESS))
        return ctx_fail(MAV_ERR_ARG, "%s: thickness %d is neither MAV_SHAPE_FILLED nor in [1, %d]", fn, thickness, MAV_SHAPE_MAX_THICKNESS);
    if ((uintptr_t)blobs % 8 || (uintptr_t)counts % 4 || (uintptr_t)out % 4 || (uintptr_t)n_out % 4)
        return ctx_fail(MAV_ERR_ARG, "%s: a pointer is not aligned to its elements", fn);
    CtxView v;
    SCHK(ctx_enter(c, batch, fn, &v));
    const size_t T = (size_t)batch * max_blobs;
    if (T > 0x7FFFFFFFull) return ctx_fail(MAV_ERR_ARG, "%s: batch * max_blobs above 2^31 - 1", fn);
    const uint32_t col = (uint32_t)colour[0] | ((uint32_t)colour[1] << 8) | ((uint32_t)colour[2] << 16) | ((uint32_t)colour[3] << 24);
    MiscScope ps(c);
    hipLaunchKernelGGL(k_shapes_from_blobs, dim3((unsigned)((T + SH_WG - 1) / SH_WG)), dim3(SH_WG), 0, v.stream, blobs, counts, batch, max_blobs,
                       thickness, col, out, n_out);
    return ctx_check_launch("shapes_from_blobs");
}

static int mosaic_checked(mav_ctx* c, const uint8_t* const* tiles, const int* ch, int rows, int cols, const void* out, const char* fn)
{
    if (!c) return ctx_fail(MAV_ERR_ARG, "%s: NULL context", fn);
    if (!tiles || !ch || !out) return ctx_fail(MAV_ERR_ARG, "%s: NULL %s", fn, !tiles ? "tiles" : !ch ? "tile_channels" : "out");
    if (rows < 1 || cols < 1 || (long long)rows * cols > MAV_MOSAIC_MAX_TILES)
        return ctx_fail(MAV_ERR_ARG, "%s: %d x %d tiles; at least 1 x 1, at most %d in all", fn, rows, cols, MAV_MOSAIC_MAX_TILES);
    for (int i = 0; i < rows * cols; i++)
        if (tiles[i] && ch[i] != 1 && ch[i] != 3) return ctx_fail(MAV_ERR_ARG, "%s: tile %d has %d channels, neither 1 nor 3", fn, i, ch[i]);
    return MAV_OK;
}
static int mosaic_size_checked(const CtxView& v, int rows, int cols, int batch, const char* fn)
{
    if ((uint64_t)v.W * v.H * (uint64_t)batch * rows * cols > 0x7FFFFFFFull) return ctx_fail(MAV_ERR_ARG, "%s: the mosaic has more than 2^31 - 1 pixels", fn);
    return MAV_OK;
}
static int mosaic_launch(mav_ctx* c, const CtxView& v, const uint8_t* const* tiles, const int* ch, int rows, int cols, int batch, uint8_t* out,
                         const char* fn)
{
    const uint64_t n64 = (uint64_t)v.W * v.H * 3 * (uint64_t)batch * rows * cols;
    Mosaic m = {};
    for (int i = 0; i < rows * cols; i++) { m.tile[i] = tiles[i]; m.ch[i] = tiles[i] ? ch[i] : 3; }
    m.rows = rows; m.cols = cols; m.W = v.W; m.H = v.H; m.B = batch; m.out = out;
    const size_t n = (size_t)n64, G = mav_bytes_form(n, out, nullptr, nullptr) == MAV_SHAPES_FORM_WORDS ? n / 16 : 0, T = G + (n - 16 * G);
    MiscScope ps(c);
    hipLaunchKernelGGL(k_mosaic, dim3((unsigned)((T + SH_WG - 1) / SH_WG)), dim3(SH_WG), 0, v.stream, m, n, G);
    return ctx_check_launch("mosaic");
}
extern "C" int mav_mosaic_dev(mav_ctx* c, const uint8_t* const* tiles, const int* tile_channels, int rows, int cols, int batch, uint8_t* out)
{
    const char* fn = "mav_mosaic_dev";
    SCHK(mosaic_checked(c, tiles, tile_channels, rows, cols, out, fn));
    CtxView v;
    SCHK(ctx_enter(c, batch, fn, &v));
    SCHK(mosaic_size_checked(v, rows, cols, batch, fn));
    return mosaic_launch(c, v, tiles, tile_channels, rows, cols, batch, out, fn);
}
extern "C" int mav_mosaic(mav_ctx* c, const uint8_t* const* tiles, const int* tile_channels, int rows, int cols, int batch, uint8_t* out)
{
    const char* fn = "mav_mosaic";
    SCHK(mosaic_checked(c, tiles, tile_channels, rows, cols, out, fn));
    StagedCall h(c, fn);
    CtxView v;
    SCHK(h.begin(batch, &v));
    SCHK(mosaic_size_checked(v, rows, cols, batch, fn));
    const size_t px = (size_t)v.W * v.H * batch;
    const uint8_t* dt[MAV_MOSAIC_MAX_TILES] = {};
    for (int i = 0; i < rows * cols; i++) dt[i] = (const uint8_t*)h.in(tiles[i], px * (tile_channels[i] == 1 ? 1 : 3));
    uint8_t* dout = (uint8_t*)h.out(out, px * 3 * rows * cols);
    SCHK(h.staged());
    SCHK(mosaic_launch(c, v, dt, tile_channels, rows, cols, batch, dout, fn));
    return h.finish();
}

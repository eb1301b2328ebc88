// Baseline JPEG (ITU T.81, SOF0 / Huffman) as libjpeg-turbo decodes it, one source for host and device: integer arithmetic only, no
// inline assembly.  include/mavflow_jpeg.h states what is accepted and what the verdicts mean.
//
//   jc_parse              host only: the segments up to SOS into a mav_jpeg_info, with a reason for a file it refuses.
//   jc_info_ok            what the decoder trusts of an info before it reads a byte through it (the device runs it too).
//   jc_geometry           MCU grid, per-component block grids and plane sizes of an image, and where they lie in the scratch.
//   JcBits                the bit reader: FF 00 un-stuffing, FF fill bytes, marker detection.  It never advances past a marker and
//                         never reads at or behind the entropy segment's end.
//   jc_build_tables       per Huffman table a first-level lookup of JC_FAST bits and the canonical max-code walk for longer codes.
//   jc_decode_interval    the MCUs of one restart interval into int16 coefficients in natural order.  Policies, as inflate_core.h's:
//                             Src   uint32_t byte(uint32_t pos): byte `pos` of the entropy segment; called for pos < size alone.
//                             Par   lane() / lanes() / sync(): the strides of the table-filling loops (host: 0, 1, nothing).
//                             Sink  begin() / coef(natural index, value) / end(int16_t* block): all 64 coefficients are written.
//                         Everything else runs on values that are the same in every lane.
//   jc_idct_pass          the 8-point pass of jidctint.c ("islow"); columns descale by 11, rows by 18.
//   jc_upsample           none / h2v1 / h2v2 "fancy" (triangle) from the component planes, with libjpeg's rule that a component of
//                         downsampled width <= 2 is replicated, and its edges taken at the REAL downsampled width and height.
//   jc_pixel              upsample + YCbCr -> RGB + the output format of one pixel.
//   jc_decode_host        all of these, serially.
//
// TERMINATION.  Every symbol consumes at least one bit or ends the interval with a verdict; bits consumed beyond those fetched end it
// with TRUNCATED (or RESTART before an RSTn); the bytes fetched are bounded by the segment's size.  A block's AC loop runs at most 63
// times, an interval has a fixed number of MCUs.
#ifndef MAV_JPEG_CORE_H
#define MAV_JPEG_CORE_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/mavflow_jpeg.h"

#if defined(__HIPCC__)
#define JC_HD __host__ __device__ inline
#else
#define JC_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define JC_U32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))       // a value every lane holds alike, kept on the scalar side
#define JC_TABLE static __device__ const
#define JC_ADD(p, v) atomicAdd((p), (v))
#define JC_MAX(p, v) atomicMax((p), (v))
#define JC_MIN(p, v) atomicMin((p), (v))
#else
#define JC_U32(x) ((uint32_t)(x))
#define JC_TABLE static const
#define JC_ADD(p, v) (void)(*(p) += (v))
#define JC_MAX(p, v) (void)(*(p) = *(p) > (v) ? *(p) : (v))
#define JC_MIN(p, v) (void)(*(p) = *(p) < (v) ? *(p) : (v))
#endif
// the one gray value of a BGR pixel; the library passes the context's own function in (mavflow_internal.h's bgr2gray_px)
#ifndef JC_GRAY_PX
#define JC_GRAY_PX(b, g, r) ((uint8_t)(((b) * 1868u + (g) * 9617u + (r) * 4899u + 8192u) >> 14))
#endif

#define JC_FAST 9                    // first-level bits of a Huffman table
#define JC_NO_ERR 0xFFFFFFFFu
#define JC_END 0x100                 // JcBits::marker: the segment's end

JC_TABLE uint8_t jc_zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- geometry and scratch layout -------------------------------------------------------------------------------------------------------
struct JcGeom {
    int comps, hmax, vmax, mcux, mcuy, mcus, intervals, ri;
    int h[3], v[3], bw[3], bh[3], dw[3], dh[3];      // blocks of the padded grid; the real downsampled size
    uint32_t block0[3];                              // the component's first block among the image's
};
// blocks of one component at full resolution on a grid of whole 16 x 16 MCUs: the unit of the scratch formula
JC_HD uint64_t jc_full_blocks(int W, int H) { return (uint64_t)(2 * ((W + 15) / 16)) * (uint64_t)(2 * ((H + 15) / 16)); }
JC_HD bool jc_shape_ok(int W, int H, int comps, int count)
{
    return W >= 1 && H >= 1 && W <= 65535 && H <= 65535 && (comps == 1 || comps == 3) && count >= 1 && count <= MAV_JPEG_MAX_COUNT;
}
// per image: coefficients, planes, a header (error word, markers found, unsupported, spare), the interval table (offset, first MCU, end, spare)
JC_HD uint64_t jc_coef_bytes(int W, int H, int comps) { return jc_full_blocks(W, H) * 128u * (uint64_t)comps; }
JC_HD uint64_t jc_plane_bytes(int W, int H, int comps) { return jc_full_blocks(W, H) * 64u * (uint64_t)comps; }
JC_HD uint64_t jc_image_scratch(int W, int H, int comps) { return jc_coef_bytes(W, H, comps) + jc_plane_bytes(W, H, comps) + 16u + jc_full_blocks(W, H) * 16u; }
struct JcScratch { int16_t* coef; uint8_t* planes; uint32_t* hdr; uint32_t* table; };
JC_HD JcScratch jc_scratch_of(void* scratch, int W, int H, int comps, uint32_t image)
{
    uint8_t* p = (uint8_t*)scratch + jc_image_scratch(W, H, comps) * image;
    JcScratch s;
    s.coef = (int16_t*)p;
    s.planes = p + jc_coef_bytes(W, H, comps);
    s.hdr = (uint32_t*)(s.planes + jc_plane_bytes(W, H, comps));
    s.table = s.hdr + 4;
    return s;
}

JC_HD bool jc_huffman_ok(const mav_jpeg_huffman* t, bool dc)
{
    int left = 1, sum = 0;
    for (int l = 0; l < 16; l++) {
        left = (left << 1) - t->counts[l];
        if (left < 0) return false;                  // over-subscribed
        sum += t->counts[l];
    }
    if (sum > 256) return false;
    if (dc)
        for (int i = 0; i < sum; i++)
            if (t->values[i] > 11) return false;     // a DC category 8-bit samples cannot have
    return true;
}
// what the decoder trusts: an info jc_parse would have produced for a file of `file_size` bytes holding an image of the call's sizes
JC_HD bool jc_info_ok(const mav_jpeg_info* I, int W, int H, int comps, uint64_t file_size)
{
    if (!jc_shape_ok(W, H, comps, 1) || I->W != W || I->H != H || I->components != comps) return false;
    if (I->restart_interval < 0 || I->restart_interval > 65535) return false;
    if (I->entropy_offset > file_size || I->entropy_bytes > file_size - I->entropy_offset || I->entropy_bytes > 0x7FFFFFFFull) return false;
    for (int c = 0; c < comps; c++) {
        const mav_jpeg_component* k = &I->comp[c];
        if (k->tq > 3 || k->td > 3 || k->ta > 3 || !I->quant_defined[k->tq] || !I->dc_defined[k->td] || !I->ac_defined[k->ta]) return false;
        if (!jc_huffman_ok(&I->dc[k->td], true) || !jc_huffman_ok(&I->ac[k->ta], false)) return false;
        if (k->h < 1 || k->h > 4 || k->v < 1 || k->v > 4) return false;
    }
    if (comps == 3) {
        if (I->comp[1].h != 1 || I->comp[1].v != 1 || I->comp[2].h != 1 || I->comp[2].v != 1) return false;
        const int h = I->comp[0].h, v = I->comp[0].v;
        if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return false;
    }
    return true;
}
// of an info that jc_info_ok accepted.  A one-component scan is not interleaved: its MCU is one block whatever its sampling factors say.
JC_HD void jc_geometry(const mav_jpeg_info* I, JcGeom* g)
{
    g->comps = I->components;
    g->hmax = g->comps == 1 ? 1 : I->comp[0].h;
    g->vmax = g->comps == 1 ? 1 : I->comp[0].v;
    g->mcux = (I->W + 8 * g->hmax - 1) / (8 * g->hmax);
    g->mcuy = (I->H + 8 * g->vmax - 1) / (8 * g->vmax);
    g->mcus = g->mcux * g->mcuy;
    g->ri = I->restart_interval;
    g->intervals = g->ri ? (g->mcus + g->ri - 1) / g->ri : 1;
    uint32_t at = 0;
    for (int c = 0; c < g->comps; c++) {
        g->h[c] = g->comps == 1 ? 1 : I->comp[c].h;
        g->v[c] = g->comps == 1 ? 1 : I->comp[c].v;
        g->bw[c] = g->mcux * g->h[c];
        g->bh[c] = g->mcuy * g->v[c];
        g->dw[c] = (I->W * g->h[c] + g->hmax - 1) / g->hmax;
        g->dh[c] = (I->H * g->v[c] + g->vmax - 1) / g->vmax;
        g->block0[c] = at;
        at += (uint32_t)(g->bw[c] * g->bh[c]);
    }
    for (int c = g->comps; c < 3; c++) g->h[c] = g->v[c] = g->bw[c] = g->bh[c] = g->dw[c] = g->dh[c] = 0, g->block0[c] = at;
}
JC_HD uint32_t jc_total_blocks(const JcGeom& g) { return g.block0[g.comps - 1] + (uint32_t)(g.bw[g.comps - 1] * g.bh[g.comps - 1]); }
JC_HD bool jc_is_rst(uint32_t b0, uint32_t b1) { return b0 == 0xFF && b1 >= 0xD0 && b1 <= 0xD7; }

// ---- the parser (host only) --------------------------------------------------------------------------------------------------------------
// a refused file leaves an all-zero info, which jc_info_ok accepts for no call
#define JC_REFUSE(code, ...) do { snprintf(why, why_n, __VA_ARGS__); memset(I, 0, sizeof *I); return (code); } while (0)
// 0, MAV_JPEG_E_UNSUPPORTED or MAV_JPEG_E_TRUNCATED; `why` names the marker
static inline int jc_parse(const uint8_t* f, size_t n, mav_jpeg_info* I, char* why, size_t why_n)
{
    memset(I, 0, sizeof *I);
    if (why_n) why[0] = 0;
    if (n < 2 || f[0] != 0xFF || f[1] != 0xD8) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "no SOI marker (FF D8) at the file's start");
    size_t pos = 2;
    bool sof = false;
    int adobe = -1;
    for (;;) {
        if (pos >= n) JC_REFUSE(MAV_JPEG_E_TRUNCATED, "the file ends before SOS");
        if (f[pos] != 0xFF) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "byte %02X at offset %zu where a marker is due", f[pos], pos);
        while (pos < n && f[pos] == 0xFF) pos++;
        if (pos >= n) JC_REFUSE(MAV_JPEG_E_TRUNCATED, "the file ends before SOS");
        const unsigned m = f[pos++];
        if (m == 0xD9) JC_REFUSE(MAV_JPEG_E_TRUNCATED, "EOI before SOS");
        if (m == 0x00 || m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "marker FF %02X before SOS", m);
        if (pos + 2 > n) JC_REFUSE(MAV_JPEG_E_TRUNCATED, "the file ends inside segment FF %02X", m);
        const size_t L = ((size_t)f[pos] << 8) | f[pos + 1];
        if (L < 2 || pos + L > n) JC_REFUSE(MAV_JPEG_E_TRUNCATED, "segment FF %02X of length %zu passes the file's end", m, L);
        const uint8_t* b = f + pos + 2;
        size_t bl = L - 2;
        if (m == 0xC0) {
            if (sof) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "a second SOF0");
            if (bl < 6) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 of %zu bytes", bl);
            if (b[0] != 8) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with %d-bit samples", b[0]);
            I->H = (b[1] << 8) | b[2];
            I->W = (b[3] << 8) | b[4];
            I->components = b[5];
            if (I->W < 1 || I->H < 1) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with an image of %d x %d (DNL is not read)", I->W, I->H);
            if (I->components != 1 && I->components != 3) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with %d components", I->components);
            if (bl != 6 + 3 * (size_t)I->components) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 of %zu bytes for %d components", bl, I->components);
            for (int c = 0; c < I->components; c++) {
                mav_jpeg_component* k = &I->comp[c];
                k->id = b[6 + 3 * c];
                k->h = b[7 + 3 * c] >> 4;
                k->v = b[7 + 3 * c] & 15;
                k->tq = b[8 + 3 * c];
                if (k->tq > 3) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 names quantisation table %d", k->tq);
                if (k->h < 1 || k->h > 4 || k->v < 1 || k->v > 4) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with sampling factors %d x %d", k->h, k->v);
            }
            sof = true;
        } else if (m == 0xC4) {
            while (bl > 0) {
                if (bl < 17) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT ends inside a table");
                const int tc = b[0] >> 4, th = b[0] & 15;
                if (tc > 1 || th > 3) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT with class %d, table %d", tc, th);
                mav_jpeg_huffman* t = tc ? &I->ac[th] : &I->dc[th];
                size_t sum = 0;
                int left = 1;
                for (int l = 0; l < 16; l++) {
                    sum += b[1 + l];
                    left = (left << 1) - b[1 + l];
                    if (left < 0) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT %s table %d is over-subscribed at length %d", tc ? "AC" : "DC", th, l + 1);
                }
                if (sum > 256) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT %s table %d counts %zu symbols", tc ? "AC" : "DC", th, sum);
                if (bl < 17 + sum) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT ends inside a table");
                memset(t, 0, sizeof *t);
                memcpy(t->counts, b + 1, 16);
                memcpy(t->values, b + 17, sum);
                (tc ? I->ac_defined : I->dc_defined)[th] = 1;
                b += 17 + sum;
                bl -= 17 + sum;
            }
        } else if (m == 0xDB) {
            while (bl > 0) {
                const int pq = b[0] >> 4, tq = b[0] & 15;
                if (pq != 0) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DQT with a %s table", pq == 1 ? "16-bit" : "malformed");
                if (tq > 3) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DQT defines table %d", tq);
                if (bl < 65) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DQT ends inside a table");
                for (int i = 0; i < 64; i++) I->quant[tq][jc_zz[i]] = b[1 + i];
                I->quant_defined[tq] = 1;
                b += 65;
                bl -= 65;
            }
        } else if (m == 0xDD) {
            if (bl != 2) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DRI of %zu bytes", bl);
            I->restart_interval = (b[0] << 8) | b[1];
        } else if (m == 0xDA) {
            if (!sof) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS before SOF0");
            if (bl < 1 || b[0] != I->components)
                JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS with %d of the frame's %d components (more than one scan)", bl ? b[0] : 0, I->components);
            if (bl != 4 + 2 * (size_t)I->components) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS of %zu bytes for %d components", bl, I->components);
            for (int c = 0; c < I->components; c++) {
                mav_jpeg_component* k = &I->comp[c];
                if (b[1 + 2 * c] != k->id) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS lists component %d where the frame has %d", b[1 + 2 * c], k->id);
                k->td = b[2 + 2 * c] >> 4;
                k->ta = b[2 + 2 * c] & 15;
                if (k->td > 3 || !I->dc_defined[k->td]) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS names DC table %d, which no DHT defined", k->td);
                if (k->ta > 3 || !I->ac_defined[k->ta]) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS names AC table %d, which no DHT defined", k->ta);
                if (!I->quant_defined[k->tq]) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 names quantisation table %d, which no DQT defined", k->tq);
                if (!jc_huffman_ok(&I->dc[k->td], true)) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DHT DC table %d holds a category above 11", k->td);
            }
            const uint8_t* e = b + 1 + 2 * I->components;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0)
                JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS with Ss, Se, Ah/Al = %d, %d, %02X (not 0, 63, 0)", e[0], e[1], e[2]);
            if (I->components == 3) {
                if (adobe == 0) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "APP14 Adobe segment with transform 0 (RGB samples)");
                if (I->comp[0].id == 'R' && I->comp[1].id == 'G' && I->comp[2].id == 'B')
                    JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with component ids R, G, B (RGB samples)");
                const int h = I->comp[0].h, v = I->comp[0].v;
                if (I->comp[1].h != 1 || I->comp[1].v != 1 || I->comp[2].h != 1 || I->comp[2].v != 1 ||
                    !((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)))
                    JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF0 with sampling %dx%d, %dx%d, %dx%d", h, v, I->comp[1].h, I->comp[1].v, I->comp[2].h, I->comp[2].v);
            }
            I->entropy_offset = pos + L;
            I->entropy_bytes = n - (pos + L);
            if (I->entropy_bytes > 0x7FFFFFFFull) JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOS with an entropy segment of 2^31 bytes or more");
            return 0;
        } else if (m == 0xEE) {
            if (bl >= 12 && memcmp(b, "Adobe", 5) == 0) adobe = b[11];
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            // APPn, COM: skipped
        } else if (m == 0xCC) {
            JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "DAC (arithmetic coding)");
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8) {
            JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "SOF%d (%s)", m - 0xC0, m == 0xC2 ? "progressive" : m == 0xC1 ? "extended sequential" : m >= 0xC9 ? "arithmetic coding" : "not baseline");
        } else {
            JC_REFUSE(MAV_JPEG_E_UNSUPPORTED, "marker FF %02X before SOS", m);
        }
        pos += L;
    }
}

// ---- the bit reader ----------------------------------------------------------------------------------------------------------------------
template <class Src> struct JcBits {
    Src& src;
    uint32_t n, pos;                 // the segment's size; the next byte to fetch
    uint32_t buf = 0, stuffed = 0;   // the bits in hand, the next one highest of the low `cnt`
    int cnt = 0, marker = -1;        // marker: -1 none met, JC_END, or the byte behind the FF the reader stands at
    JC_HD JcBits(Src& s, uint32_t size, uint32_t start) : src(s), n(size), pos(start) {}
    // the next data byte, or -1 with `marker` set
    JC_HD int next()
    {
        while (marker < 0) {
            if (pos >= n) { marker = JC_END; break; }
            const uint32_t b = src.byte(pos);
            if (b != 0xFF) { pos += 1; return (int)b; }
            if (pos + 1 >= n) { marker = JC_END; break; }
            const uint32_t b2 = src.byte(pos + 1);
            if (b2 == 0) { pos += 2; stuffed += 1; return 0xFF; }
            if (b2 == 0xFF) { pos += 1; continue; }                // a fill byte
            marker = (int)b2;
        }
        return -1;
    }
    JC_HD void fill()
    {
        while (cnt <= 24) {
            const int b = next();
            if (b < 0) break;
            buf = (buf << 8) | (uint32_t)b;
            cnt += 8;
        }
    }
    // the next k <= 16 bits, zeros where the segment has none
    JC_HD uint32_t peek(int k) const
    {
        const uint32_t mask = (1u << k) - 1u;
        return cnt >= k ? (buf >> (cnt - k)) & mask : (buf << (k - cnt)) & mask;
    }
    JC_HD bool skip(int k)
    {
        if (k > cnt) return false;
        cnt -= k;
        return true;
    }
};

// ---- Huffman tables -----------------------------------------------------------------------------------------------------------------------
struct JcHuff {
    uint16_t lut[1 << JC_FAST];      // (symbol << 4) | length for codes of up to JC_FAST bits, 0 otherwise
    int32_t maxcode[17], valoff[17]; // per length: the largest code (-1: none); index of its first symbol minus its first code
    uint8_t vals[256];
};
struct JcTables { JcHuff dc[4], ac[4]; };         // 11328 bytes (LDS on the device)

template <class Par> JC_HD void jc_build_huff(Par& par, const mav_jpeg_huffman* t, JcHuff* h)
{
    for (int i = par.lane(); i < (1 << JC_FAST); i += par.lanes()) h->lut[i] = 0;
    for (int i = par.lane(); i < 256; i += par.lanes()) h->vals[i] = t->values[i];
    par.sync();
    uint32_t code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        const uint32_t c = JC_U32(t->counts[l - 1]);
        if (par.lane() == 0) {
            h->valoff[l] = (int32_t)p - (int32_t)code;
            h->maxcode[l] = c ? (int32_t)(code + c - 1) : -1;
        }
        if (l <= JC_FAST)
            for (uint32_t s = 0; s < c; s++) {
                const uint32_t lo = (code + s) << (JC_FAST - l), span = 1u << (JC_FAST - l);
                const uint16_t e = (uint16_t)((JC_U32(t->values[p + s]) << 4) | (uint32_t)l);
                for (uint32_t k = (uint32_t)par.lane(); k < span; k += (uint32_t)par.lanes()) h->lut[lo + k] = e;
            }
        p += c;
        code = (code + c) << 1;
    }
    par.sync();
}
// the tables the scan's components name, each built once
template <class Par> JC_HD void jc_build_tables(Par& par, const mav_jpeg_info* I, JcTables* T)
{
    uint32_t built = 0;
    for (int c = 0; c < I->components; c++) {
        const uint32_t td = JC_U32(I->comp[c].td), ta = JC_U32(I->comp[c].ta);
        if (!(built & (1u << td))) jc_build_huff(par, &I->dc[td], &T->dc[td]);
        if (!(built & (16u << ta))) jc_build_huff(par, &I->ac[ta], &T->ac[ta]);
        built |= (1u << td) | (16u << ta);
    }
}

// ---- one restart interval -----------------------------------------------------------------------------------------------------------------
struct JcUnit { uint32_t code, mcus, nonzero, zrl, stuffed, max_len, end; };

// a symbol of table h, or -1: no code in 16 bits of the segment (CODE), -2: the segment's bits ran out
template <class Src> JC_HD int jc_symbol(JcBits<Src>& br, const JcHuff* h, JcUnit* u)
{
    br.fill();
    const uint32_t e = JC_U32(h->lut[br.peek(JC_FAST)]);
    int len, sym;
    if (e) {
        len = (int)(e & 15u);
        sym = (int)(e >> 4);
    } else {
        len = JC_FAST + 1;
        for (; len <= 16; len++)
            if ((int32_t)br.peek(len) <= (int32_t)JC_U32(h->maxcode[len])) break;
        if (len > 16) return br.cnt >= 16 ? -1 : -2;
        sym = (int)JC_U32(h->vals[((int32_t)br.peek(len) + (int32_t)JC_U32(h->valoff[len])) & 255]);
    }
    if (!br.skip(len)) return -2;
    if ((uint32_t)len > u->max_len) u->max_len = (uint32_t)len;
    return sym;
}
JC_HD int jc_extend(uint32_t v, int t) { return t == 0 || v >= (1u << (t - 1)) ? (int)v : (int)v - (1 << t) + 1; }
// t <= 15 bits as a value; false: the segment's bits ran out
template <class Src> JC_HD bool jc_receive(JcBits<Src>& br, int t, int* out)
{
    br.fill();
    const uint32_t v = br.peek(t);
    if (!br.skip(t)) return false;
    *out = jc_extend(v, t);
    return true;
}

// MCUs first_mcu .. first_mcu + n_mcus - 1 from byte `start` of the segment.  `last`: no RSTn is due behind this interval.
template <class Src, class Sink>
JC_HD void jc_decode_interval(Src& src, uint32_t size, uint32_t start, const mav_jpeg_info* I, const JcGeom& g, const JcTables* T, Sink& sink,
                              int16_t* coef, uint32_t interval, uint32_t first_mcu, uint32_t n_mcus, bool last, JcUnit* u)
{
    JcBits<Src> br(src, size, start);
    uint32_t pred[3] = {0, 0, 0};
    int code = 0;
    u->code = u->mcus = u->nonzero = u->zrl = u->stuffed = u->max_len = 0;
    for (uint32_t m = 0; m < n_mcus && !code; m++) {
        const uint32_t mx = (first_mcu + m) % (uint32_t)g.mcux, my = (first_mcu + m) / (uint32_t)g.mcux;
        for (int c = 0; c < g.comps && !code; c++) {
            const JcHuff* hd = &T->dc[JC_U32(I->comp[c].td)];
            const JcHuff* ha = &T->ac[JC_U32(I->comp[c].ta)];
            for (int b = 0; b < g.h[c] * g.v[c] && !code; b++) {
                const uint32_t bx = mx * (uint32_t)g.h[c] + (uint32_t)(b % g.h[c]), by = my * (uint32_t)g.v[c] + (uint32_t)(b / g.h[c]);
                sink.begin();
                const int t = jc_symbol(br, hd, u);
                int diff = 0;
                if (t < 0) code = t;
                else if (t > 0) {
                    if (!jc_receive(br, t, &diff)) code = -2;
                    else u->nonzero++;
                }
                if (!code) {
                    pred[c] += (uint32_t)diff;
                    sink.coef(0, (int16_t)(uint16_t)pred[c]);
                }
                int k = 1;
                while (k < 64 && !code) {
                    const int rs = jc_symbol(br, ha, u);
                    if (rs < 0) { code = rs; break; }
                    const int r = rs >> 4, s = rs & 15;
                    if (s == 0) {
                        if (r != 15) break;                        // end of block
                        u->zrl++;
                        k += 16;
                        if (k > 64) code = MAV_JPEG_E_COEF_INDEX;
                        continue;
                    }
                    k += r;
                    if (k > 63) { code = MAV_JPEG_E_COEF_INDEX; break; }
                    int v;
                    if (!jc_receive(br, s, &v)) { code = -2; break; }
                    sink.coef(JC_U32(jc_zz[k]), (int16_t)v);
                    u->nonzero++;
                    k++;
                }
                sink.end(coef + ((size_t)g.block0[c] + (size_t)by * (uint32_t)g.bw[c] + bx) * 64);
            }
        }
        if (!code) u->mcus++;
    }
    if (code == -1) code = MAV_JPEG_E_CODE;
    if (code == -2) code = br.marker >= 0xD0 && br.marker <= 0xD7 ? MAV_JPEG_E_RESTART : MAV_JPEG_E_TRUNCATED;
    if (!code) {
        // the interval's end: the bits left of the last byte are padding; behind them stands RSTn with n = interval mod 8, or, behind the
        // last interval, anything but an RSTn
        const bool whole = br.cnt >= 8;
        const int b = whole ? 0 : br.next();
        const bool rst = br.marker >= 0xD0 && br.marker <= 0xD7;
        if (!last) {
            if (whole || b >= 0 || !rst || (uint32_t)(br.marker & 7) != (interval & 7u)) code = MAV_JPEG_E_RESTART;
        } else if (!whole && b < 0 && rst) {
            code = MAV_JPEG_E_RESTART;
        }
    }
    u->code = (uint32_t)code;
    u->stuffed = br.stuffed;
    u->end = br.pos;
}
// an interval whose start no marker gave
JC_HD void jc_missing_interval(uint32_t size, JcUnit* u)
{
    u->mcus = u->nonzero = u->zrl = u->stuffed = u->max_len = 0;
    u->code = MAV_JPEG_E_RESTART;
    u->end = size;
}
// a unit's result into the image's status, its error word and its row of the table
JC_HD void jc_merge(mav_jpeg_status* st, uint32_t* err, uint32_t* row, uint32_t interval, const JcUnit& u)
{
    JC_ADD(&st->mcus, u.mcus);
    JC_ADD(&st->nonzero, u.nonzero);
    JC_ADD(&st->zrl, u.zrl);
    JC_ADD(&st->stuffed, u.stuffed);
    JC_MAX(&st->max_code_len, u.max_len);
    if (u.code) JC_MIN(err, (interval << 4) | u.code);
    row[2] = u.end;
}
JC_HD int jc_verdict_code(uint32_t err) { return err == JC_NO_ERR ? 0 : (int)(err & 15u); }
// code and consumed of an image whose units have all merged
JC_HD void jc_verdict(mav_jpeg_status* st, uint32_t err, const uint32_t* table, uint32_t intervals)
{
    st->code = jc_verdict_code(err);
    st->consumed = st->code == MAV_JPEG_E_UNSUPPORTED ? 0 : table[4 * (err == JC_NO_ERR ? intervals - 1 : err >> 4) + 2];
}

// ---- the IDCT -------------------------------------------------------------------------------------------------------------------------------
JC_HD int32_t jc_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
// jidctint.c's 8-point pass on v[0 .. 7], in place, descaled by n.  Two's complement arithmetic that wraps (uint32_t), so that a corrupt
// stream's coefficients overflow into defined values.
JC_HD void jc_idct_pass(int32_t* v, int n)
{
    const uint32_t i0 = (uint32_t)v[0], i1 = (uint32_t)v[1], i2 = (uint32_t)v[2], i3 = (uint32_t)v[3], i4 = (uint32_t)v[4], i5 = (uint32_t)v[5],
                   i6 = (uint32_t)v[6], i7 = (uint32_t)v[7];
    uint32_t z1 = (i2 + i6) * 4433u;
    const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5;
    z4 = z4 * (uint32_t)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    v[0] = jc_descale(t10 + a3, n); v[7] = jc_descale(t10 - a3, n);
    v[1] = jc_descale(t11 + a2, n); v[6] = jc_descale(t11 - a2, n);
    v[2] = jc_descale(t12 + a1, n); v[5] = jc_descale(t12 - a1, n);
    v[3] = jc_descale(t13 + a0, n); v[4] = jc_descale(t13 - a0, n);
}
JC_HD uint8_t jc_clamp8(int32_t x) { return (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x); }
// one block, serially: coefficients in natural order, the table in natural order -> 8 rows of 8 samples at `out`, `pitch` apart
JC_HD void jc_idct_block(const int16_t* coef, const uint8_t* q, uint8_t* out, size_t pitch)
{
    int32_t ws[64], v[8];
    for (int c = 0; c < 8; c++) {
        for (int r = 0; r < 8; r++) v[r] = (int32_t)coef[r * 8 + c] * (int32_t)q[r * 8 + c];
        jc_idct_pass(v, 11);
        for (int r = 0; r < 8; r++) ws[r * 8 + c] = v[r];
    }
    for (int r = 0; r < 8; r++) {
        for (int c = 0; c < 8; c++) v[c] = ws[r * 8 + c];
        jc_idct_pass(v, 18);
        for (int c = 0; c < 8; c++) out[(size_t)r * pitch + c] = jc_clamp8(v[c] + 128);
    }
}

// ---- upsampling, colour, output -----------------------------------------------------------------------------------------------------------------
// component c of pixel (x, y): jdsample.c's h2v1 / h2v2 fancy upsampling, or replication where libjpeg replicates (downsampled width <= 2)
JC_HD uint32_t jc_upsample(const uint8_t* plane, const JcGeom& g, int c, int x, int y)
{
    const int pitch = g.bw[c] * 8, hs = g.hmax / g.h[c], vs = g.vmax / g.v[c], dw = g.dw[c], dh = g.dh[c];
    if (hs == 1) return plane[(size_t)y * pitch + x];
    const int cx = x >> 1;
    if (dw <= 2) return plane[(size_t)(vs == 2 ? y >> 1 : y) * pitch + cx];
    if (vs == 1) {
        const uint8_t* p = plane + (size_t)y * pitch;
        if (x & 1) return cx == dw - 1 ? p[cx] : (3u * p[cx] + p[cx + 1] + 2u) >> 2;
        return cx == 0 ? p[0] : (3u * p[cx] + p[cx - 1] + 1u) >> 2;
    }
    const int cy = y >> 1, ny = (y & 1) ? (cy + 1 < dh ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t *p0 = plane + (size_t)cy * pitch, *p1 = plane + (size_t)ny * pitch;
    const uint32_t cur = 3u * p0[cx] + p1[cx];
    if (x & 1) return cx == dw - 1 ? (cur * 4u + 7u) >> 4 : (cur * 3u + (3u * p0[cx + 1] + p1[cx + 1]) + 7u) >> 4;
    return cx == 0 ? (cur * 4u + 8u) >> 4 : (cur * 3u + (3u * p0[cx - 1] + p1[cx - 1]) + 8u) >> 4;
}
// jdcolor.c's tables as arithmetic: FIX(1.402), FIX(1.772), FIX(0.71414), FIX(0.34414) at 16 bits, `>>` arithmetic
JC_HD void jc_ycc_to_rgb(int y, int cb, int cr, uint32_t* r, uint32_t* g, uint32_t* b)
{
    cb -= 128;
    cr -= 128;
    *r = jc_clamp8(y + ((91881 * cr + 32768) >> 16));
    *g = jc_clamp8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    *b = jc_clamp8(y + ((116130 * cb + 32768) >> 16));
}
JC_HD int jc_out_channels(int comps, int format) { return format == MAV_JPEG_OUT_SAMPLES ? comps : format == MAV_JPEG_OUT_BGR ? 3 : 1; }
// pixel (x, y) in the output format: px[0 .. jc_out_channels - 1]
JC_HD void jc_pixel(const uint8_t* planes, const JcGeom& g, int format, int x, int y, uint8_t* px)
{
    const uint32_t Y = jc_upsample(planes + (size_t)g.block0[0] * 64, g, 0, x, y);
    if (g.comps == 1) {
        px[0] = (uint8_t)Y;
        if (format == MAV_JPEG_OUT_BGR) px[1] = px[2] = (uint8_t)Y;
        return;
    }
    const uint32_t Cb = jc_upsample(planes + (size_t)g.block0[1] * 64, g, 1, x, y), Cr = jc_upsample(planes + (size_t)g.block0[2] * 64, g, 2, x, y);
    if (format == MAV_JPEG_OUT_SAMPLES) {
        px[0] = (uint8_t)Y; px[1] = (uint8_t)Cb; px[2] = (uint8_t)Cr;
        return;
    }
    uint32_t r, gg, b;
    jc_ycc_to_rgb((int)Y, (int)Cb, (int)Cr, &r, &gg, &b);
    if (format == MAV_JPEG_OUT_BGR) { px[0] = (uint8_t)b; px[1] = (uint8_t)gg; px[2] = (uint8_t)r; }
    else px[0] = JC_GRAY_PX(b, gg, r);
}

// ---- the host decoder: the same functions, called serially ------------------------------------------------------------------------------------
struct JcHostSrc { const uint8_t* z; uint32_t byte(uint32_t pos) const { return z[pos]; } };
struct JcHostPar { int lane() const { return 0; } int lanes() const { return 1; } void sync() const {} };
struct JcHostSink {
    int16_t blk[64];
    void begin() { memset(blk, 0, sizeof blk); }
    void coef(uint32_t i, int16_t v) { blk[i] = v; }
    void end(int16_t* dst) { memcpy(dst, blk, sizeof blk); }
};
// the interval table of a segment: rows (offset, first MCU, end, spare) for the markers found, at most `intervals` rows; returns the markers found
static inline uint32_t jc_scan_intervals_host(const uint8_t* z, uint32_t size, const JcGeom& g, uint32_t* table)
{
    uint32_t found = 0;
    table[0] = 0; table[1] = 0; table[2] = 0; table[3] = 0;
    if (g.ri)
        for (uint32_t i = 0; i + 1 < size; i++)
            if (jc_is_rst(z[i], z[i + 1])) {
                found++;
                if (found < (uint32_t)g.intervals) {
                    uint32_t* row = table + 4 * found;
                    row[0] = i + 2; row[1] = found * (uint32_t)g.ri; row[2] = 0; row[3] = 0;
                }
            }
    return found;
}
// MAV_OK, or MAV_ERR_OOM when the host has no memory for the coefficients; the verdict is status->code
static inline int jc_decode_host(const uint8_t* file, size_t n, const mav_jpeg_info* I, int format, uint8_t* out, mav_jpeg_status* st)
{
    memset(st, 0, sizeof *st);
    const bool sized = jc_shape_ok(I->W, I->H, I->components, 1);
    const size_t out_bytes = sized ? (size_t)I->W * I->H * jc_out_channels(I->components, format) : 0;
    memset(out, 0, out_bytes);
    if (!sized || !jc_info_ok(I, I->W, I->H, I->components, n)) {
        st->code = MAV_JPEG_E_UNSUPPORTED;
        return 0;
    }
    JcGeom g;
    jc_geometry(I, &g);
    const uint32_t blocks = jc_total_blocks(g), size = (uint32_t)I->entropy_bytes;
    int16_t* coef = (int16_t*)malloc((size_t)blocks * 128);
    uint8_t* planes = (uint8_t*)malloc((size_t)blocks * 64);
    uint32_t* table = (uint32_t*)malloc((size_t)g.intervals * 16);
    JcTables* T = (JcTables*)malloc(sizeof(JcTables));
    if (!coef || !planes || !table || !T) {
        free(coef); free(planes); free(table); free(T);
        return -3;
    }
    const uint8_t* z = file + I->entropy_offset;
    JcHostSrc src{z};
    JcHostPar par;
    JcHostSink sink;
    const uint32_t found = jc_scan_intervals_host(z, size, g, table);
    uint32_t err = JC_NO_ERR;
    st->intervals = (uint32_t)g.intervals;
    jc_build_tables(par, I, T);
    for (uint32_t k = 0; k < (uint32_t)g.intervals; k++) {
        JcUnit u;
        uint32_t* row = table + 4 * k;
        if (k > found) {
            row[0] = size; row[1] = k * (uint32_t)g.ri; row[3] = 0;
            jc_missing_interval(size, &u);
        } else {
            const uint32_t first = row[1], left = (uint32_t)g.mcus - first;
            jc_decode_interval(src, size, row[0], I, g, T, sink, coef, k, first, g.ri && (uint32_t)g.ri < left ? (uint32_t)g.ri : left,
                               k + 1 == (uint32_t)g.intervals, &u);
        }
        jc_merge(st, &err, row, k, u);
    }
    jc_verdict(st, err, table, (uint32_t)g.intervals);
    if (st->code == 0) {
        for (int c = 0; c < g.comps; c++)
            for (int by = 0; by < g.bh[c]; by++)
                for (int bx = 0; bx < g.bw[c]; bx++)
                    jc_idct_block(coef + ((size_t)g.block0[c] + (size_t)by * g.bw[c] + bx) * 64, I->quant[I->comp[c].tq],
                                  planes + (size_t)g.block0[c] * 64 + (size_t)by * 8 * (g.bw[c] * 8) + (size_t)bx * 8, (size_t)g.bw[c] * 8);
        const int oc = jc_out_channels(g.comps, format);
        for (int y = 0; y < I->H; y++)
            for (int x = 0; x < I->W; x++) jc_pixel(planes, g, format, x, y, out + ((size_t)y * I->W + x) * oc);
    }
    free(coef); free(planes); free(table); free(T);
    return 0;
}
#endif

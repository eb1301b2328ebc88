// PNG encoder kernels (include/mavflow.h: mav_png_encode*): device-resident 8-bit images -> one RFC 1950 zlib stream per image whose
// inflated bytes are the PNG scanline stream (per row the filter-type byte 1 = Sub, then W * C filtered bytes in file order: gray, RGB
// or RGBA -- the B <-> R swap of a BGR(A) image happens on load).
//
// The scanline stream of an image is cut into SEGMENTS of PNG_SEG bytes (the last one shorter), one workgroup each, joined the way
// pigz / Z_FULL_FLUSH joins independent deflate streams:
//   78 01 | segment 0 | segment 1 | ... | last segment | Adler-32 (big-endian)
// A segment is ONE deflate block and ends on a byte boundary; no match reaches back across a segment start:
//   coded   BTYPE=10: Sub-filtered bytes as literals and byte-run tokens (distance 1, length 3 .. 258), a dynamic Huffman code of its
//           own (lengths <= 15), the code-length alphabet sent with a FIXED complete code (lengths 0 .. 12 in 4 bits, 13 .. 15 and
//           the unused repeat symbols in 5), ONE distance code of 1 bit; a non-final segment is closed by an empty stored block
//           (000, pad to the byte, 00 00 FF FF), the final one has BFINAL = 1 and is padded to the byte;
//   stored  BTYPE=00 (5 bytes + the segment's bytes) whenever the coded form would not be shorter -- so a segment never costs more
//           than its length + 5 bytes.
// Sub needs no other row, so segment boundaries are free to fall anywhere in the stream.  Everything is integer arithmetic and the
// bit packing ORs disjoint bit ranges into LDS words: the same image gives the same bytes on every call.
//
// Launch chain of one chunk of images: k_png_segment (grid: segments x images; bytes into the segment's worst-case slot, byte count
// and Adler partial beside it) -> k_png_image_scan (per image: offsets of its segments, stream size, Adler-32 combined from the
// partials) -> k_png_index (offsets of the images in the output buffer) -> k_png_compact (every segment to its final place, zlib
// header and Adler-32 around each image).
#include "mavflow_internal.h"

#define PNG_THREADS 256
#define PNG_WAVES (PNG_THREADS / 64)
#define PNG_WORDS (MAV_PNG_SEG / 64)          // run-start bitmask words of a full segment
#define PNG_ADLER 65521u
#define PNG_NSYM 286                          // literal / length symbols sent (HLIT = 29)
#define PNG_HDR_FIXED 74                      // BFINAL, BTYPE, HLIT, HDIST, HCLEN (17 bits) + 19 x 3 bits of code-length code lengths

size_t png_segments(size_t raw) { return (raw + MAV_PNG_SEG - 1) / MAV_PNG_SEG; }
size_t png_workspace_per_image(size_t raw)
{
    // slots + per-segment record (uint4) + per-segment offset (u64), + the image's (size, adler) pair
    return png_segments(raw) * ((size_t)MAV_PNG_SLOT + sizeof(uint4) + sizeof(unsigned long long)) + 2 * sizeof(unsigned long long);
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// OR `nb` (<= 24) bits of v into the LDS bit stream at bit offset o (LSB first).  Disjoint ranges: the result does not depend on order.
__device__ __forceinline__ void put_bits(uint32_t* out, uint32_t o, uint32_t v, uint32_t nb)
{
    const uint32_t w = o >> 5, sh = o & 31;
    atomicOr(&out[w], v << sh);
    if (sh + nb > 32) atomicOr(&out[w + 1], v >> (32 - sh));
}
// extra bits of length symbol s (257 .. 285)
__device__ __forceinline__ uint32_t len_extra_bits(uint32_t s) { return (s < 265 || s == 285) ? 0u : (s - 261) >> 2; }

// What position i of the segment emits: nothing (sym < 0: inside a run token), a literal (sym < 256) or a run token (sym >= 257, with
// `ev` in `eb` extra bits).  A maximal run of equal bytes [s, e) is: literal at s, then the r = e - s - 1 bytes after it in tokens of
// 258 starting at s + 1 -- a last piece of 1 or 2 bytes is literals, as is all of r < 3.
struct PngTok { int sym; uint32_t eb, ev; };
__device__ __forceinline__ PngTok png_token(uint32_t i, const uint8_t* f, const unsigned long long* mask, const uint32_t* prev, const uint32_t* nxt)
{
    PngTok t{(int)f[i], 0u, 0u};
    const uint32_t w = i >> 6, l = i & 63;
    const unsigned long long m = mask[w];
    const unsigned long long lower = m & (~0ull >> (63 - l));
    const uint32_t s = lower ? (w << 6) + 63 - (uint32_t)__clzll((long long)lower) : prev[w];
    if (i == s) return t;
    const unsigned long long upper = l < 63 ? (m & (~0ull << (l + 1))) : 0ull;
    const uint32_t e = upper ? (w << 6) + (uint32_t)__ffsll((unsigned long long)upper) - 1 : nxt[w];
    const uint32_t r = e - s - 1, k = i - s - 1;
    if (r < 3) return t;
    const uint32_t q = k % 258, rem = r - (k - q);          // rem: what the piece that holds i still has to cover
    if (rem < 3) return t;
    if (q) { t.sym = -1; return t; }
    const uint32_t len = rem < 258 ? rem : 258;
    if (len == 258) { t.sym = 285; return t; }
    const uint32_t v = len - 3;
    if (v < 8) { t.sym = 257 + (int)v; return t; }
    t.eb = (31 - __clz((int)v)) - 2;
    t.sym = 261 + 4 * (int)t.eb + (int)((v >> t.eb) & 3);
    t.ev = v & ((1u << t.eb) - 1);
    return t;
}

// One segment.  grid = (segments of one image, images of the chunk).
template <int C>
__global__ __launch_bounds__(PNG_THREADS) void k_png_segment(const uint8_t* __restrict__ imgs, uint32_t rowbytes, unsigned long long img_bytes,
                                                             unsigned long long raw, uint32_t nseg, uint8_t* __restrict__ slots,
                                                             uint4* __restrict__ meta)
{
    __shared__ uint32_t s_f[MAV_PNG_SEG / 4];               // the segment's filtered bytes
    __shared__ uint32_t s_out[MAV_PNG_SEG / 4 + 8];         // its coded form (only ever filled when shorter than the stored form)
    __shared__ unsigned long long s_mask[PNG_WORDS];        // bit i: a run of equal bytes starts at i
    __shared__ uint32_t s_prev[PNG_WORDS], s_nxt[PNG_WORDS];// last run start before / first run start after each mask word
    __shared__ uint32_t s_whist[PNG_WAVES][288];            // symbol counts of each wave's part of the segment
    __shared__ uint32_t s_hist[288], s_ctab[288], s_key[288];
    __shared__ uint16_t s_sym[288];
    __shared__ uint8_t s_len[288];
    __shared__ uint32_t s_nc[34], s_nextcode[16], s_red[16], s_n;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t seg = blockIdx.x;
    const unsigned long long seg0 = (unsigned long long)seg * MAV_PNG_SEG;
    const uint32_t N = (uint32_t)(raw - seg0 < MAV_PNG_SEG ? raw - seg0 : MAV_PNG_SEG);
    const bool final_seg = seg + 1 == nseg;
    const uint32_t stride = rowbytes + 1;
    const unsigned long long row0 = seg0 / stride;
    const uint32_t col0 = (uint32_t)(seg0 - row0 * stride);
    const uint8_t* img = imgs + (size_t)blockIdx.y * img_bytes;
    uint8_t* fb = (uint8_t*)s_f;

    // ---- 1. Sub filter into LDS, Adler partial sums --------------------------------------------------------------------------------
    for (int i = tid; i < MAV_PNG_SEG / 4 + 8; i += PNG_THREADS) s_out[i] = 0;
    for (int i = tid; i < PNG_WAVES * 288; i += PNG_THREADS) (&s_whist[0][0])[i] = 0;
    uint32_t s1 = 0, s2 = 0;                                 // sum of bytes, sum of byte * (N - i): below 2^32 for <= 96 bytes per thread
    for (uint32_t i = tid; i < N; i += PNG_THREADS) {
        uint32_t col = col0 + i;
        unsigned long long row = row0;
        if (col >= stride) { const uint32_t q = col / stride; row += q; col -= q * stride; }
        uint32_t v = 1;                                      // the row's filter-type byte: Sub
        if (col) {
            const uint32_t x = col - 1, px = x / C, ch = x - px * C;
            const uint32_t mc = (C >= 3 && ch < 3) ? 2 - ch : ch;
            const uint8_t* p = img + row * rowbytes + (size_t)px * C + mc;
            v = (uint32_t)(uint8_t)(p[0] - (px ? p[-C] : 0));
        }
        fb[i] = (uint8_t)v;
        s1 += v;
        s2 += v * (N - i);
    }
    s1 = wave_sum(s1 % PNG_ADLER);
    s2 = wave_sum(s2 % PNG_ADLER);
    if (lane == 0) { s_red[wave] = s1; s_red[4 + wave] = s2; }
    __syncthreads();
    const uint32_t adler_a = (1 + s_red[0] + s_red[1] + s_red[2] + s_red[3]) % PNG_ADLER;
    const uint32_t adler_b = (N + s_red[4] + s_red[5] + s_red[6] + s_red[7]) % PNG_ADLER;

    // ---- 2. run starts as a bit mask, and per mask word the nearest run start outside it ---------------------------------------------
    const uint32_t nwords = (N + 63) >> 6;
    for (uint32_t w = wave; w < nwords; w += PNG_WAVES) {
        const uint32_t i = (w << 6) + lane;
        const bool start = i < N && (i == 0 || fb[i] != fb[i - 1]);
        const unsigned long long m = __ballot(start);
        if (lane == 0) s_mask[w] = m;
    }
    __syncthreads();
    for (uint32_t w = tid; w < nwords; w += PNG_THREADS) {
        uint32_t p = 0, q = N;
        for (int j = (int)w - 1; j >= 0; j--) {
            const unsigned long long m = s_mask[j];
            if (m) { p = ((uint32_t)j << 6) + 63 - (uint32_t)__clzll((long long)m); break; }
        }
        for (uint32_t j = w + 1; j < nwords; j++) {
            const unsigned long long m = s_mask[j];
            if (m) { q = (j << 6) + (uint32_t)__ffsll(m) - 1; break; }
        }
        s_prev[w] = p; s_nxt[w] = q;
    }
    __syncthreads();

    // ---- 3. symbol counts: every wave takes a contiguous part of the segment (the same parts as in step 6) ---------------------------
    const uint32_t part = (((N + PNG_WAVES - 1) / PNG_WAVES) + 63) & ~63u;
    const uint32_t p_begin = wave * part < N ? wave * part : N, p_end = p_begin + part < N ? p_begin + part : N;
    for (uint32_t i = p_begin + lane; i < p_end; i += 64) {
        const PngTok t = png_token(i, fb, s_mask, s_prev, s_nxt);
        if (t.sym >= 0) atomicAdd(&s_whist[wave][t.sym], 1u);
    }
    __syncthreads();
    for (int s = tid; s < 288; s += PNG_THREADS) {
        s_hist[s] = s < PNG_NSYM ? s_whist[0][s] + s_whist[1][s] + s_whist[2][s] + s_whist[3][s] + (s == 256 ? 1u : 0u) : 0u;
        s_len[s] = 0;
    }
    __syncthreads();

    // ---- 4. code lengths: used symbols sorted by count (rank sort), then one thread builds the Huffman lengths in place (Moffat &
    //         Katajainen's minimum-redundancy algorithm) and limits them to 15 bits by moving codes between lengths until the Kraft sum
    //         is exactly one (a complete code, as inflate demands of the literal / length code)
    for (int s = tid; s < 288; s += PNG_THREADS) {
        const uint32_t fs = s_hist[s];
        uint32_t rank = 0, n = 0;
        for (int j = 0; j < PNG_NSYM; j++) {
            const uint32_t fj = s_hist[j];
            n += fj != 0;
            rank += fj != 0 && (fj < fs || (fj == fs && j < s));
        }
        if (fs) { s_key[rank] = fs; s_sym[rank] = (uint16_t)s; }
        if (s == 0) s_n = n;
    }
    __syncthreads();
    if (tid == 0) {
        const int n = (int)s_n;                              // >= 2: end-of-block and at least one literal
        uint32_t* A = s_key;
        int root = 0, leaf = 2, next;
        A[0] += A[1];
        for (next = 1; next < n - 1; next++) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2; next = n - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
            while (avbl > used) { A[next--] = dpth; avbl--; }
            avbl = 2 * used; dpth++; used = 0;
        }
        for (int l = 0; l < 34; l++) s_nc[l] = 0;
        for (int i = 0; i < n; i++) s_nc[A[i] > 32 ? 32 : A[i]]++;
        for (int l = 16; l <= 32; l++) s_nc[15] += s_nc[l];
        uint32_t total = 0;
        for (int l = 15; l > 0; l--) total += s_nc[l] << (15 - l);
        while (total > (1u << 15)) {                         // only ever too large: longer codes were cut to 15 bits
            s_nc[15]--;
            for (int l = 14; l > 0; l--)
                if (s_nc[l]) { s_nc[l]--; s_nc[l + 1] += 2; break; }
            total--;
        }
        int j = n;
        for (int l = 1; l <= 15; l++)
            for (uint32_t k = s_nc[l]; k > 0; k--) s_len[s_sym[--j]] = (uint8_t)l;
        uint32_t code = 0;
        s_nextcode[0] = 0;
        for (int l = 1; l <= 15; l++) { code = (code + s_nc[l - 1]) << 1; s_nextcode[l] = code; }
    }
    __syncthreads();

    // ---- 5. canonical codes (bit-reversed: Huffman codes go into the stream most significant bit first), the block header, and the
    //         bits each wave's part will take
    for (int s = tid; s < 288; s += PNG_THREADS) {
        const uint32_t len = s_len[s];
        uint32_t c = 0;
        if (len) {
            uint32_t r = 0;
            for (int j = 0; j < s; j++) r += s_len[j] == len;
            c = (__brev(s_nextcode[len] + r) >> (32 - len)) | (len << 16);
        }
        s_ctab[s] = c;
    }
    // header: the 286 literal / length code lengths and the one distance code's length (1), each as its fixed code-length code
    uint32_t hl[2], hb[2];
    for (int k = 0; k < 2; k++) {
        const int s = 2 * tid + k;
        hl[k] = s < PNG_NSYM ? s_len[s] : 1u;
        hb[k] = s <= PNG_NSYM ? (hl[k] <= 12 ? 4u : 5u) : 0u;
    }
    const uint32_t hincl = wave_incl_scan(hb[0] + hb[1], lane);
    if (lane == 63) s_red[wave] = hincl;
    {
        uint32_t bits = 0;                                   // this wave's part: sum of count x (code length + extra bits + distance bit)
        for (int s = lane; s < PNG_NSYM; s += 64)
            bits += s_whist[wave][s] * ((uint32_t)s_len[s] + (s > 256 ? len_extra_bits(s) + 1 : 0));
        bits = wave_sum(bits);
        if (lane == 0) s_red[4 + wave] = bits;
    }
    __syncthreads();
    uint32_t hdr_bits = PNG_HDR_FIXED, tok_base = 0;
    {
        uint32_t hoff = PNG_HDR_FIXED + hincl - hb[0] - hb[1];
        for (int w = 0; w < PNG_WAVES; w++) {
            if (w < wave) { hoff += s_red[w]; tok_base += s_red[4 + w]; }
            hdr_bits += s_red[w];
        }
        const uint32_t tok_bits = s_red[4] + s_red[5] + s_red[6] + s_red[7];
        const uint32_t eob = s_ctab[256];
        const uint32_t T = hdr_bits + tok_bits + (eob >> 16);
        const uint32_t coded = final_seg ? (T + 7) >> 3 : ((T + 3 + 7) >> 3) + 4;
        uint8_t* slot = slots + ((size_t)blockIdx.y * nseg + seg) * MAV_PNG_SLOT;
        if (coded >= N + 5) {
            // ---- stored block: 5 bytes + the segment as it is ------------------------------------------------------------------------
            if (tid == 0) {
                slot[0] = final_seg ? 1 : 0;
                slot[1] = (uint8_t)(N & 255); slot[2] = (uint8_t)(N >> 8);
                slot[3] = (uint8_t)(~N & 255); slot[4] = (uint8_t)((~N >> 8) & 255);
                meta[(size_t)blockIdx.y * nseg + seg] = make_uint4(N + 5, adler_a, adler_b, N);
            }
            for (uint32_t i = tid; i < N; i += PNG_THREADS) slot[5 + i] = fb[i];
            return;
        }
        // ---- 6. coded block ----------------------------------------------------------------------------------------------------------
        if (tid == 0) {
            put_bits(s_out, 0, (final_seg ? 1u : 0u) | (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13), 17);
            // code-length code lengths in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: symbols 0 .. 12 take 4 bits, the rest 5
            const uint32_t cl[19] = {5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 5, 4, 5};
            for (int k = 0; k < 19; k++) put_bits(s_out, 17 + 3 * k, cl[k], 3);
            put_bits(s_out, hdr_bits + tok_bits, eob & 0xffff, eob >> 16);
            if (!final_seg) put_bits(s_out, (coded - 4) * 8 + 16, 0xffffu, 16);      // 000, pad, then LEN = 0, NLEN = 0xffff
        }
        for (int k = 0; k < 2; k++)
            if (hb[k]) {
                // canonical code of length value v: v (4 bits) for v <= 12, 26 + (v - 13) (5 bits) above
                const uint32_t code = hl[k] <= 12 ? hl[k] : 13 + hl[k];
                put_bits(s_out, hoff, __brev(code) >> (32 - hb[k]), hb[k]);
                hoff += hb[k];
            }
        uint32_t carry = hdr_bits + tok_base;
        for (uint32_t base = p_begin; base < p_end; base += 64) {
            const uint32_t i = base + lane;
            uint32_t v = 0, nb = 0;
            if (i < p_end) {
                const PngTok t = png_token(i, fb, s_mask, s_prev, s_nxt);
                if (t.sym >= 0) {
                    const uint32_t c = s_ctab[t.sym], len = c >> 16;
                    v = (c & 0xffff) | (t.ev << len);
                    nb = len + (t.sym > 256 ? t.eb + 1 : 0);  // extra bits, then the distance code: one 0 bit
                }
            }
            const uint32_t incl = wave_incl_scan(nb, lane);
            if (nb) put_bits(s_out, carry + incl - nb, v, nb);
            carry += __shfl(incl, 63);
        }
        __syncthreads();
        uint4* dst = (uint4*)slot;
        const uint4* src = (const uint4*)s_out;
        for (uint32_t i = tid; i < (coded + 15) / 16; i += PNG_THREADS) dst[i] = src[i];
        if (tid == 0) meta[(size_t)blockIdx.y * nseg + seg] = make_uint4(coded, adler_a, adler_b, N);
    }
}

// Per image: where each of its segments starts inside the image's zlib stream (after the 2 header bytes), the stream's size and its
// Adler-32.  With segment partials a_j = 1 + sum of bytes, b_j = len_j + sum of byte * (len_j - i), joining them front to back
// (a = a1 + a2 - 1, b = b1 + b2 + len2 * (a1 - 1), mod 65521) unrolls to  A = 1 + sum (a_j - 1),  B = sum [b_j + (a_j - 1) * (bytes behind
// segment j)], which needs no order.  grid = images of the chunk.
__global__ __launch_bounds__(PNG_THREADS) void k_png_image_scan(const uint4* __restrict__ meta, uint32_t nseg, unsigned long long raw,
                                                                unsigned long long* __restrict__ segoff, unsigned long long* __restrict__ imgrec)
{
    __shared__ uint32_t s_w[PNG_WAVES];
    __shared__ unsigned long long s_a[PNG_WAVES], s_b[PNG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint4* m = meta + (size_t)blockIdx.x * nseg;
    unsigned long long* so = segoff + (size_t)blockIdx.x * nseg;
    unsigned long long carry = 2, sa = 0, sb = 0;
    for (uint32_t base = 0; base < nseg; base += PNG_THREADS) {
        const uint32_t j = base + tid;
        uint4 r = make_uint4(0, 1, 0, 0);
        if (j < nseg) r = m[j];
        const uint32_t incl = wave_incl_scan(r.x, lane);
        __syncthreads();                                     // s_w of the previous round has been read
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        unsigned long long off = carry + incl - r.x;
        uint32_t tot = 0;
        for (int w = 0; w < PNG_WAVES; w++) { if (w < wave) off += s_w[w]; tot += s_w[w]; }
        if (j < nseg) {
            so[j] = off;
            const unsigned long long end = (unsigned long long)(j + 1) * MAV_PNG_SEG < raw ? (unsigned long long)(j + 1) * MAV_PNG_SEG : raw;
            const unsigned long long a1 = (r.y + PNG_ADLER - 1) % PNG_ADLER;
            sa += a1;
            sb += (r.z + a1 * ((raw - end) % PNG_ADLER)) % PNG_ADLER;
        }
        carry += tot;
    }
    sa = wave_sum64(sa); sb = wave_sum64(sb);
    if (lane == 0) { s_a[wave] = sa; s_b[wave] = sb; }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long A = (1 + s_a[0] + s_a[1] + s_a[2] + s_a[3]) % PNG_ADLER, B = (s_b[0] + s_b[1] + s_b[2] + s_b[3]) % PNG_ADLER;
        imgrec[2 * blockIdx.x] = carry + 4;
        imgrec[2 * blockIdx.x + 1] = (B << 16) | A;
    }
}

// index[img0 + i] = (offset, size) of the chunk's images, packed behind the images before them.  One thread: a chunk holds few images.
__global__ void k_png_index(const unsigned long long* __restrict__ imgrec, int img0, int nimg, unsigned long long* __restrict__ index)
{
    if (threadIdx.x || blockIdx.x) return;
    unsigned long long off = img0 ? index[2 * (img0 - 1)] + index[2 * (img0 - 1) + 1] : 0;
    for (int i = 0; i < nimg; i++) {
        index[2 * (img0 + i)] = off;
        index[2 * (img0 + i) + 1] = imgrec[2 * i];
        off += imgrec[2 * i];
    }
}

// Every segment from its slot to its final place (any byte alignment: whole destination words are assembled from two slot words), the
// zlib header in front of an image's first segment and the Adler-32 behind its last.  grid = (segments, images of the chunk).
__global__ __launch_bounds__(PNG_THREADS) void k_png_compact(const uint8_t* __restrict__ slots, const uint4* __restrict__ meta,
                                                             const unsigned long long* __restrict__ segoff,
                                                             const unsigned long long* __restrict__ imgrec, uint32_t nseg, int img0,
                                                             const unsigned long long* __restrict__ index, uint8_t* __restrict__ out)
{
    const int tid = threadIdx.x;
    const size_t s = (size_t)blockIdx.y * nseg + blockIdx.x;
    const uint32_t n = meta[s].x;
    uint8_t* img_out = out + index[2 * (img0 + blockIdx.y)];
    uint8_t* dst = img_out + segoff[s];
    const uint8_t* src = slots + s * MAV_PNG_SLOT;
    const uint32_t* src32 = (const uint32_t*)src;
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > n) head = n;
    const uint32_t nw = (n - head) >> 2, tail = head + 4 * nw;
    if ((uint32_t)tid < head) dst[tid] = src[tid];
    if ((uint32_t)tid < n - tail) dst[tail + tid] = src[tail + tid];
    uint32_t* dst32 = (uint32_t*)(dst + head);
    const uint32_t sh = head * 8;                            // source byte of destination word w: head + 4 w
    for (uint32_t w = tid; w < nw; w += PNG_THREADS) {
        const uint32_t lo = src32[w];
        dst32[w] = sh ? (lo >> sh) | (src32[w + 1] << (32 - sh)) : lo;      // the slot has 16 spare bytes behind the longest segment
    }
    if (tid == 0) {
        if (blockIdx.x == 0) { img_out[0] = 0x78; img_out[1] = 0x01; }
        if (blockIdx.x + 1 == nseg) {
            const uint32_t ad = (uint32_t)imgrec[2 * blockIdx.y + 1];
            dst[n] = (uint8_t)(ad >> 24); dst[n + 1] = (uint8_t)(ad >> 16); dst[n + 2] = (uint8_t)(ad >> 8); dst[n + 3] = (uint8_t)ad;
        }
    }
}

// `nimg` images (img0 .. of the call) of H rows of rowbytes = W * C bytes; ws: png_workspace_per_image(raw) * nimg bytes, 16-byte aligned.
void launch_png_encode(hipStream_t st, const uint8_t* imgs, int img0, int nimg, int W, int H, int C, uint8_t* ws, uint8_t* out,
                       unsigned long long* index)
{
    const uint32_t rowbytes = (uint32_t)W * C;
    const unsigned long long raw = (unsigned long long)H * (rowbytes + 1), img_bytes = (unsigned long long)H * rowbytes;
    const uint32_t nseg = (uint32_t)png_segments(raw);
    const size_t segs = (size_t)nseg * nimg;
    uint8_t* slots = ws;
    uint4* meta = (uint4*)(slots + segs * MAV_PNG_SLOT);
    unsigned long long* segoff = (unsigned long long*)(meta + segs);
    unsigned long long* imgrec = segoff + segs;
    const uint8_t* src = imgs + (size_t)img0 * img_bytes;
    const dim3 grid(nseg, nimg);
    if (C == 1) hipLaunchKernelGGL(k_png_segment<1>, grid, dim3(PNG_THREADS), 0, st, src, rowbytes, img_bytes, raw, nseg, slots, meta);
    else if (C == 3) hipLaunchKernelGGL(k_png_segment<3>, grid, dim3(PNG_THREADS), 0, st, src, rowbytes, img_bytes, raw, nseg, slots, meta);
    else hipLaunchKernelGGL(k_png_segment<4>, grid, dim3(PNG_THREADS), 0, st, src, rowbytes, img_bytes, raw, nseg, slots, meta);
    hipLaunchKernelGGL(k_png_image_scan, dim3(nimg), dim3(PNG_THREADS), 0, st, meta, nseg, raw, segoff, imgrec);
    hipLaunchKernelGGL(k_png_index, dim3(1), dim3(64), 0, st, imgrec, img0, nimg, index);
    hipLaunchKernelGGL(k_png_compact, grid, dim3(PNG_THREADS), 0, st, slots, meta, segoff, imgrec, nseg, img0, index, out);
}

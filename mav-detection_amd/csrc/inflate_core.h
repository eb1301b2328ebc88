// zlib-wrapped DEFLATE (RFC 1950, RFC 1951), one source for host and device: integer arithmetic only, no inline assembly.
//
// inf_run() parses the zlib header, decodes the blocks into TOKENS -- a literal, a (length, distance) match, a run of stored bytes --
// and parses the trailer.  It proves every token in bounds before it hands it to the sink (pos + length <= raw size, 1 <= distance
// <= pos, stored bytes inside the stream), so the copy stage needs no checks of its own.  The policies:
//     Src   uint32_t word(size_t pos): the four stream bytes at pos .. pos + 3, little endian, ZERO where pos + i >= size.  Nothing
//           else reads the stream, so nothing reads past stream + size.
//     Par   lane() / lanes() / sync(): the strides of the table-filling loops (host: 0, 1, nothing; device: the lane, 64, a barrier).
//           Everything else runs on values that are the same in every lane.
//     Sink  literal(pos, byte), match(pos, length, distance), stored(pos, stream offset, length), finish().
//
// TERMINATION.  The block loop runs once per block, and a block header consumes three bits.  The symbol loop's every iteration consumes
// at least one bit (a code has at least one bit; a code not found ends the run).  The code-length loops consume at least one bit per
// iteration and are bounded by 19 and 320 entries.  A field whose last bit lies past the stream's end ends the run with TRUNCATED, so
// the bits consumed are bounded by 8 * size, and the refill advances by four bytes only when the field in hand needs it: the read
// position never passes size + 8.  Output is bounded by the raw size: a token that would pass it ends the run with OVERFLOW.
#ifndef MAV_INFLATE_CORE_H
#define MAV_INFLATE_CORE_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/mavflow_png_decode.h"

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ inline
#else
#define INF_HD inline
#endif
// a value every lane holds alike, kept on the scalar side of the device
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_U32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define INF_U32(x) ((uint32_t)(x))
#endif

#define INF_FAST_LL 10               // first-level bits of the literal/length table
#define INF_FAST_D 8                 // and of the distance table
#define INF_MAX_LL 288
#define INF_MAX_D 32

// One stream's code tables: 3656 bytes (LDS on the device).  A first-level entry is (symbol << 4) | length, 0 where the code is longer
// than the first level (or absent); count[] / sym[] are the canonical form (symbols in code order, codes of each length counted).
struct InfTables {
    uint16_t ll_lut[1 << INF_FAST_LL];
    uint16_t d_lut[1 << INF_FAST_D];
    uint16_t ll_count[16], d_count[16], c_count[16];
    uint16_t ll_sym[INF_MAX_LL], d_sym[INF_MAX_D], c_sym[20];
    uint8_t lens[INF_MAX_LL + INF_MAX_D];
};

INF_HD uint64_t inf_u64(uint64_t v) { return (uint64_t)INF_U32((uint32_t)v) | ((uint64_t)INF_U32((uint32_t)(v >> 32)) << 32); }

template <class Src> struct InfBits {
    Src& src;
    uint64_t n, pos = 0, buf = 0;    // the stream's size; the next byte to fetch; the bits in hand, the next one lowest
    uint32_t cnt = 0;
    INF_HD InfBits(Src& s, uint64_t size) : src(s), n(size) {}
    // at least 32 bits in hand (zeros past the end)
    INF_HD void refill()
    {
        if (cnt <= 32) {
            buf = inf_u64(buf | ((uint64_t)src.word((size_t)pos) << cnt));
            cnt += 32;
            pos += 4;
        }
    }
    INF_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }
    INF_HD void drop(uint32_t k) { buf >>= k; cnt -= k; }
    INF_HD uint64_t used_bits() const { return pos * 8 - cnt; }
    // stream bits not yet consumed (0 when the reader is past the end)
    INF_HD uint64_t avail() const { const uint64_t u = used_bits(); return u < n * 8 ? n * 8 - u : 0; }
    INF_HD void align() { drop(cnt & 7); }
    INF_HD uint64_t byte_pos() const { return (used_bits() + 7) / 8; }
};

// Canonical tables of `n` code lengths.  zlib's verdicts (inftrees.c): over-subscribed: refused; incomplete: refused unless `allow_one`
// (the literal/length and distance sets, never the code-length code) and no code is longer than one bit; no code at all: accepted for
// those two sets (every code is then unused).  Returns 0 or MAV_PNG_E_CODE_LENGTHS.  lut == NULL: no first level (the code-length code).
template <class Par>
INF_HD int inf_build(Par& par, const uint8_t* lens, int n, bool allow_one, uint16_t* count, uint16_t* sym, uint16_t* lut, int fast)
{
    uint32_t offs[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    par.sync();
    if (par.lane() == 0)
        for (int s = 0; s < n; s++) count[lens[s]]++;
    par.sync();
    int left = 1, max = 0;
    for (int l = 1; l < 16; l++) {
        const int c = (int)INF_U32(count[l]);
        left = (left << 1) - c;
        if (left < 0) return MAV_PNG_E_CODE_LENGTHS;
        if (c) max = l;
    }
    if (left > 0 && max != 0 && !(allow_one && max == 1)) return MAV_PNG_E_CODE_LENGTHS;
    if (max == 0 && !allow_one) return MAV_PNG_E_CODE_LENGTHS;
    offs[1] = 0;
    next[1] = 0;
    for (int l = 1; l < 15; l++) {
        offs[l + 1] = offs[l] + INF_U32(count[l]);
        next[l + 1] = (next[l] + INF_U32(count[l])) << 1;
    }
    if (lut)
        for (int i = par.lane(); i < (1 << fast); i += par.lanes()) lut[i] = 0;
    par.sync();
    for (int s = 0; s < n; s++) {
        const uint32_t l = INF_U32(lens[s]);
        if (!l) continue;
        if (par.lane() == 0) sym[offs[l]] = (uint16_t)s;
        offs[l]++;
        const uint32_t code = next[l]++;
        if (lut && l <= (uint32_t)fast) {
            uint32_t r = 0;
            for (uint32_t b = 0; b < l; b++) r |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t k = r + ((uint32_t)par.lane() << l); k < (1u << fast); k += (uint32_t)par.lanes() << l) lut[k] = (uint16_t)((s << 4) | l);
        }
    }
    par.sync();
    return 0;
}

// One code of a canonical table: the symbol, or -1 where the bits in hand are no code (an incomplete set's unused code), or -2 where
// the stream ends inside the code.  A code not found is judged over its 15 bits.
template <class Src>
INF_HD int inf_decode(InfBits<Src>& b, const uint16_t* count, const uint16_t* sym, const uint16_t* lut, int fast)
{
    b.refill();
    const uint64_t avail = b.avail();
    if (lut) {
        const uint32_t e = INF_U32(lut[b.peek(fast)]);
        if (e) {
            if ((e & 15u) > avail) return -2;
            b.drop(e & 15u);
            return (int)(e >> 4);
        }
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code |= (uint32_t)(b.buf >> (l - 1)) & 1u;
        const uint32_t c = INF_U32(count[l]);
        if (code - first < c) {
            if (l > avail) return -2;
            b.drop(l);
            return (int)INF_U32(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return avail < 15 ? -2 : -1;
}

// the order in which a dynamic block sends the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
INF_HD uint32_t inf_cl_order(uint32_t i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// a field of k <= 16 bits into `var`, or out with TRUNCATED
#define INF_TAKE(var, k)                                          \
    do {                                                          \
        b.refill();                                               \
        if ((uint64_t)(k) > b.avail()) return MAV_PNG_E_TRUNCATED; \
        var = b.peek(k);                                          \
        b.drop(k);                                                \
    } while (0)

// The run.  st: zeroed here, then filled; adler_computed is the caller's (the copy stage's bytes are its to read).  Returns st->code.
template <class Src, class Par, class Sink>
INF_HD int inf_blocks(Src& src, uint64_t n, uint64_t raw_bytes, InfTables* T, Par& par, Sink& sink, mav_png_status* st)
{
    InfBits<Src> b(src, n);
    uint32_t v;
    // -- RFC 1950 header
    uint32_t cmf, flg;
    INF_TAKE(cmf, 8);
    INF_TAKE(flg, 8);
    st->consumed = b.byte_pos();
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 32u) || ((cmf << 8) | flg) % 31u) return MAV_PNG_E_HEADER;
    uint64_t pos = 0;
    bool fixed_built = false;
    for (uint32_t last = 0; !last;) {
        uint32_t type;
        INF_TAKE(last, 1);
        INF_TAKE(type, 2);
        if (type == 3) return MAV_PNG_E_BLOCK_TYPE;
        if (type == 0) {
            uint32_t len, nlen;
            b.align();
            INF_TAKE(len, 16);
            INF_TAKE(nlen, 16);
            st->blocks[0]++;
            if ((len ^ 0xFFFFu) != nlen) return MAV_PNG_E_STORED_LEN;
            // the bits in hand are whole bytes here: the stored bytes start at the reader's byte position
            const uint64_t at = b.byte_pos();
            if (pos + len > raw_bytes) return MAV_PNG_E_OVERFLOW;
            if (at + len > n) return MAV_PNG_E_TRUNCATED;
            if (len) sink.stored(pos, at, len);
            pos += len;
            st->produced = pos;
            b.pos = at + len;
            b.buf = 0;
            b.cnt = 0;
            st->consumed = b.byte_pos();
            continue;
        }
        int nll, nd;
        if (type == 1) {
            st->blocks[1]++;
            nll = INF_MAX_LL;
            nd = INF_MAX_D;
            if (!fixed_built) {
                par.sync();
                for (int i = par.lane(); i < INF_MAX_LL + INF_MAX_D; i += par.lanes())
                    T->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                par.sync();
            }
        } else {
            st->blocks[2]++;
            fixed_built = false;
            uint32_t hlit, hdist, hclen;
            INF_TAKE(hlit, 5);
            INF_TAKE(hdist, 5);
            INF_TAKE(hclen, 4);
            nll = (int)hlit + 257;
            nd = (int)hdist + 1;
            const int ncl = (int)hclen + 4;
            if (nll > 286 || nd > 30) return MAV_PNG_E_CODE_LENGTHS;
            par.sync();
            for (int i = par.lane(); i < 19; i += par.lanes()) T->lens[i] = 0;
            par.sync();
            for (int i = 0; i < ncl; i++) {
                INF_TAKE(v, 3);
                if (par.lane() == 0) T->lens[inf_cl_order((uint32_t)i)] = (uint8_t)v;
            }
            par.sync();
            if (inf_build(par, T->lens, 19, false, T->c_count, T->c_sym, (uint16_t*)nullptr, 0)) return MAV_PNG_E_CODE_LENGTHS;
            // the lengths of both sets as ONE run: a repeat may cross from the literal/length set into the distance set
            int have = 0;
            uint32_t prev = 0;
            while (have < nll + nd) {
                const int s = inf_decode(b, T->c_count, T->c_sym, (const uint16_t*)nullptr, 0);
                if (s == -2) return MAV_PNG_E_TRUNCATED;
                if (s < 0) return MAV_PNG_E_CODE_LENGTHS;
                uint32_t rep = 1, val = (uint32_t)s;
                if (s == 16) {
                    if (have == 0) return MAV_PNG_E_CODE_LENGTHS;
                    INF_TAKE(v, 2);
                    rep = 3 + v;
                    val = prev;
                } else if (s == 17) {
                    INF_TAKE(v, 3);
                    rep = 3 + v;
                    val = 0;
                } else if (s == 18) {
                    INF_TAKE(v, 7);
                    rep = 11 + v;
                    val = 0;
                }
                if (have + (int)rep > nll + nd) return MAV_PNG_E_CODE_LENGTHS;
                if (par.lane() == 0)
                    for (uint32_t k = 0; k < rep; k++) T->lens[have + k] = (uint8_t)val;
                have += (int)rep;
                prev = val;
            }
            par.sync();
            if (INF_U32(T->lens[256]) == 0) return MAV_PNG_E_CODE_LENGTHS;
        }
        if (!(type == 1 && fixed_built)) {
            if (inf_build(par, T->lens, nll, true, T->ll_count, T->ll_sym, T->ll_lut, INF_FAST_LL)) return MAV_PNG_E_CODE_LENGTHS;
            if (inf_build(par, T->lens + nll, nd, true, T->d_count, T->d_sym, T->d_lut, INF_FAST_D)) return MAV_PNG_E_CODE_LENGTHS;
            fixed_built = type == 1;
        }
        st->consumed = b.byte_pos();
        // -- the symbols of the block
        for (;;) {
            const int s = inf_decode(b, T->ll_count, T->ll_sym, T->ll_lut, INF_FAST_LL);
            if (s == -2) return MAV_PNG_E_TRUNCATED;
            if (s < 0 || s >= 286) return MAV_PNG_E_SYMBOL;
            if (s < 256) {
                if (pos + 1 > raw_bytes) return MAV_PNG_E_OVERFLOW;
                sink.literal(pos, (uint32_t)s);
                pos += 1;
                st->produced = pos;
                continue;
            }
            if (s == 256) break;
            uint32_t len, dist;
            if (s < 265) len = (uint32_t)s - 254;
            else if (s == 285) len = 258;
            else {
                const uint32_t e = ((uint32_t)s - 261) >> 2;
                INF_TAKE(v, e);
                len = ((4 + (((uint32_t)s - 265) & 3u)) << e) + 3 + v;
            }
            const int d = inf_decode(b, T->d_count, T->d_sym, T->d_lut, INF_FAST_D);
            if (d == -2) return MAV_PNG_E_TRUNCATED;
            if (d < 0 || d >= 30) return MAV_PNG_E_SYMBOL;
            if (d < 4) dist = (uint32_t)d + 1;
            else {
                const uint32_t e = ((uint32_t)d >> 1) - 1;
                INF_TAKE(v, e);
                dist = ((2 + ((uint32_t)d & 1u)) << e) + 1 + v;
            }
            if (dist > pos) return MAV_PNG_E_DISTANCE;
            if (pos + len > raw_bytes) return MAV_PNG_E_OVERFLOW;
            sink.match(pos, len, dist);
            pos += len;
            st->produced = pos;
            if (len > st->max_length) st->max_length = len;
            if (dist > st->max_distance) st->max_distance = dist;
        }
        st->consumed = b.byte_pos();
    }
    if (pos != raw_bytes) return MAV_PNG_E_SHORT;
    // -- RFC 1950 trailer: the Adler-32, most significant byte first
    b.align();
    uint32_t a = 0;
    for (int i = 0; i < 4; i++) {
        INF_TAKE(v, 8);
        a = (a << 8) | v;
    }
    st->adler_stream = a;
    st->consumed = b.byte_pos();
    return 0;
}

template <class Src, class Par, class Sink>
INF_HD int inf_run(Src& src, uint64_t n, uint64_t raw_bytes, InfTables* T, Par& par, Sink& sink, mav_png_status* st)
{
    *st = mav_png_status{};
    st->code = inf_blocks(src, n, raw_bytes, T, par, sink, st);
    sink.finish();
    return st->code;
}

// ---- the host policies: the stream in memory, one lane, a serial copy -----------------------------------------------------------------
struct InfHostSrc {
    const uint8_t* z;
    size_t n;
    uint32_t word(size_t pos) const
    {
        uint32_t w = 0;
        for (size_t i = 0; i < 4; i++)
            if (pos + i < n) w |= (uint32_t)z[pos + i] << (8 * i);
        return w;
    }
};
struct InfHostPar {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
};
struct InfHostSink {
    const uint8_t* z;
    uint8_t* raw;
    void literal(uint64_t pos, uint32_t byte) { raw[pos] = (uint8_t)byte; }
    void match(uint64_t pos, uint32_t len, uint32_t dist)
    {
        for (uint32_t i = 0; i < len; i++) raw[pos + i] = raw[pos - dist + i];
    }
    void stored(uint64_t pos, uint64_t at, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++) raw[pos + i] = z[at + i];
    }
    void finish() {}
};
// Adler-32 of n bytes, continued from (s1, s2): exact integer arithmetic, chunks short enough that nothing wraps
inline uint32_t inf_adler32_host(const uint8_t* p, size_t n)
{
    uint32_t s1 = 1, s2 = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;
        for (size_t i = 0; i < k; i++) { s1 += p[i]; s2 += s1; }
        s1 %= 65521u;
        s2 %= 65521u;
        p += k;
        n -= k;
    }
    return (s2 << 16) | s1;
}
// The whole host decode: raw must hold raw_bytes.  Returns st->code.
inline int inf_inflate_host(const uint8_t* z, size_t n, uint8_t* raw, size_t raw_bytes, mav_png_status* st)
{
    InfTables T;
    InfHostSrc src{z, n};
    InfHostPar par;
    InfHostSink sink{z, raw};
    if (inf_run(src, n, raw_bytes, &T, par, sink, st) == 0) {
        st->adler_computed = inf_adler32_host(raw, raw_bytes);
        if (st->adler_computed != st->adler_stream) st->code = MAV_PNG_E_ADLER;
    }
    return st->code;
}
#endif

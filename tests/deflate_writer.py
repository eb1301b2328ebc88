"""A bit-level DEFLATE writer (RFC 1950 / 1951) for the decoder's case table: stored, fixed and dynamic blocks from chosen code lengths
and raw token lists, with every field open to being written wrong on purpose.  Nothing here looks at the decoder; zlib is the judge of
what these streams mean (tests/png_decode_cases.py).

Tokens: an int 0 .. 255 is a literal; (length, distance) is a match; ("ll", symbol) writes a bare literal/length symbol and
("ll", symbol, extra, nbits) one with its extra bits; ("d", code, extra, nbits) a bare distance code -- the last three for symbols no
encoder would write."""
import struct
import zlib

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length):
    """(symbol, extra value, extra bits) of a match length 3 .. 258"""
    assert 3 <= length <= 258
    k = 28 if length == 258 else max(j for j in range(28) if LBASE[j] <= length)
    return 257 + k, length - LBASE[k], LEXT[k]


def distance_code(dist):
    assert 1 <= dist <= 32768
    k = max(j for j in range(30) if DBASE[j] <= dist)
    return k, dist - DBASE[k], DEXT[k]


def canonical(lengths):
    """{symbol: (code, length)} of a list of code lengths, RFC 1951 3.2.2 (no check of the set: broken sets are wanted too)"""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def complete_lengths(symbols, size):
    """`size` code lengths, a COMPLETE code over the given symbols (at least two): the first 2^L - n of them one bit shorter"""
    symbols = list(symbols)
    n = len(symbols)
    assert n >= 2
    L = (n - 1).bit_length()
    out = [0] * size
    for i, s in enumerate(symbols):
        out[s] = L - 1 if i < (1 << L) - n else L
    return out


def rle_lengths(lens):
    """the code-length symbols of a run of lengths, greedy with 16 / 17 / 18: [(symbol, extra value, extra bits)]"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11, 7))
                run -= k
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3, 2))
                run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


class Writer:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        """nbits of value, least significant first"""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, nbits):
        """a Huffman code: most significant bit first"""
        for k in range(nbits - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += bytes(data)

    @property
    def bit_length(self):
        return 8 * len(self.out) + self.n

    # ---- the zlib wrapper
    def header(self, cmf=0x78, fdict=False, fcheck=True):
        flg = 0x20 if fdict else 0
        flg += (31 - ((cmf << 8) + flg) % 31) % 31
        if not fcheck:
            flg ^= 1                                   # one off a multiple of 31
        self.raw(bytes([cmf, flg]))
        return self

    def trailer(self, data, wrong=False):
        self.align()
        self.raw(struct.pack(">I", (zlib.adler32(bytes(data)) ^ (1 if wrong else 0)) & 0xFFFFFFFF))
        return self

    # ---- blocks
    def block_header(self, final, btype):
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)

    def stored(self, data, final=False, nlen=None):
        data = bytes(data)
        assert len(data) <= 65535
        self.block_header(final, 0)
        self.align()
        self.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
        self.raw(data)
        return self

    def tokens(self, toks, ll, dd):
        """the tokens with the codes ll / dd ({symbol: (code, length)}); the end-of-block symbol is the caller's token ("ll", 256)"""
        for t in toks:
            if isinstance(t, int):
                self.code(*ll[t])
            elif t[0] == "ll":
                self.code(*ll[t[1]])
                if len(t) == 4:
                    self.bits(t[2], t[3])
            elif t[0] == "d":
                self.code(*dd[t[1]])
                self.bits(t[2], t[3])
            else:
                length, dist = t
                s, ev, eb = length_symbol(length)
                self.code(*ll[s])
                self.bits(ev, eb)
                c, ev, eb = distance_code(dist)
                self.code(*dd[c])
                self.bits(ev, eb)

    def fixed(self, toks, final=False, eob=True):
        self.block_header(final, 1)
        self.tokens(list(toks) + ([("ll", 256)] if eob else []), canonical(FIXED_LL), canonical(FIXED_D))
        return self

    def dynamic(self, toks, ll_lens, d_lens, final=False, eob=True, cl_lens=None, cl_syms=None, hclen=None):
        """a dynamic block.  ll_lens (257 .. 288 entries) and d_lens (1 .. 32) are sent as ONE run of code-length symbols (cl_syms
        replaces rle_lengths' greedy choice); cl_lens: the 19 lengths of the code-length code (default: a complete code over the
        symbols used); hclen: how many of them are sent."""
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        syms = rle_lengths(ll_lens + d_lens) if cl_syms is None else list(cl_syms)
        if cl_lens is None:
            used = sorted({s for s, _, _ in syms})
            if len(used) == 1:
                used = sorted(set(used) | {0 if used[0] != 0 else 1})
            cl_lens = complete_lengths(used, 19)
        cl = canonical(cl_lens)
        if hclen is None:
            hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
        self.block_header(final, 2)
        self.bits(len(ll_lens) - 257, 5)
        self.bits(len(d_lens) - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lens[s], 3)
        for s, ev, eb in syms:
            self.code(*cl[s])
            self.bits(ev, eb)
        self.tokens(list(toks) + ([("ll", 256)] if eob else []), canonical(ll_lens), canonical(d_lens))
        return self

    def done(self):
        self.align()
        return bytes(self.out)


def expand(toks, out=b""):
    """the bytes a token list stands for, appended to `out`"""
    out = bytearray(out)
    for t in toks:
        if isinstance(t, int):
            out.append(t)
        elif not isinstance(t[0], str):
            length, dist = t
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)

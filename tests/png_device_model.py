"""The device PNG encoder's zlib stream, byte for byte, on the CPU.

Written from the format's description (DESIGN.md 4b and the header comment of csrc/kernels_png.hip), not from the kernel's data layout:
no bit masks, no waves, no LDS words.  The encoder is all integers and every tie is decided by a stated rule, so its output is a function
of the scanline stream alone; this file is that function.  tests/png_stream_ref.py is a second PRODUCER of the block layout (other tail
rule, other way to stay within 15 bits); this one is the MODEL the device's bytes are compared with.

Per segment of SEG bytes of the scanline stream (the last one shorter), each on its own:
  tokens     a maximal run of equal bytes [s, e) is a literal at s; the e - s - 1 bytes behind it go in pieces of 258 counted from s + 1;
             a piece -- or the whole remainder -- of fewer than 3 bytes is literals; a piece of 3 .. 258 is one length symbol with its extra
             bits (RFC 1951; 258 is symbol 285) and the single distance code (distance 1);
  histogram  over the 286 literal / length symbols, end-of-block counted once;
  lengths    the used symbols in ascending (count, symbol) order; a Huffman tree by the two-queue merge, a leaf taken before an internal
             node of the same weight (what Moffat & Katajainen's in-place algorithm does); only the NUMBER of leaves per depth is kept;
             depths above 15 count as 15; while the Kraft sum, in units of 2^-15, is above 2^15: one code leaves length 15, one code of
             the longest non-empty length l < 15 moves to l + 1, and one more code is added at l + 1; the lengths are then handed out
             shortest first to the most frequent symbols (of equal counts: the higher symbol first); canonical codes in symbol order;
  header     BFINAL, BTYPE = 10, HLIT = 29, HDIST = 0, HCLEN = 15; the code-length code is fixed (lengths 0 .. 12 in 4 bits, 13 .. 18 in
             5); 286 lengths and the one distance code's length 1, no repeat symbols;
  closing    the last segment is padded to the byte; any other is followed by an empty stored block (000, pad, 00 00 FF FF);
  stored     BTYPE = 00 (5 bytes + the segment) iff the coded form's bytes, closing included, are >= N + 5.
Stream: 78 01, the segments, Adler-32 big-endian."""
import struct

import numpy as np

SEG = 24576
NSYM = 286
EOB = 256
MAXLEN = 15
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _length_tables():
    sym, eb, ev = np.zeros(259, np.int64), np.zeros(259, np.int64), np.zeros(259, np.int64)
    for length in range(3, 259):
        k = max(j for j in range(29) if LBASE[j] <= length)
        sym[length], eb[length], ev[length] = 257 + k, LEXT[k], length - LBASE[k]
    return sym, eb, ev


LEN_SYM, LEN_EB, LEN_EV = _length_tables()


# ---- images <-> scanline streams ---------------------------------------------------------------------------------------------------
def scanlines(img) -> bytes:
    """The Sub-filtered scanline stream of an (H, W) / (H, W, C) u8 image, C = 1 gray, 3 BGR, 4 BGRA (the file holds gray / RGB / RGBA)."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    H, W, C = a.shape
    assert a.dtype == np.uint8 and C in (1, 3, 4)
    if C >= 3:
        a = a[:, :, [2, 1, 0] + ([3] if C == 4 else [])]
    rows = a.reshape(H, W * C).astype(np.int16)
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = 1
    out[:, 1:C + 1] = rows[:, :C]
    out[:, C + 1:] = (rows[:, C:] - rows[:, :-C]) & 255
    return out.tobytes()


def image_of_stream(stream: bytes, W: int) -> np.ndarray:
    """The (H, W) gray image whose Sub-filtered rows are `stream`: H rows of the filter byte 01 and W bytes; a pixel is the running sum
    modulo 256 along its row."""
    b = np.frombuffer(bytes(stream), np.uint8)
    assert W >= 1 and b.size and b.size % (W + 1) == 0, (b.size, W)
    rows = b.reshape(-1, W + 1)
    assert (rows[:, 0] == 1).all(), "every row starts with the filter byte 01"
    return np.ascontiguousarray((np.cumsum(rows[:, 1:].astype(np.uint32), axis=1) & 255).astype(np.uint8))


# ---- one segment ---------------------------------------------------------------------------------------------------------------------
def tokens(seg):
    """(symbol, number of extra bits, extra value) of every token of the segment, in order (no end-of-block)."""
    d = np.frombuffer(bytes(seg), np.uint8).astype(np.int64)
    n = d.size
    assert 1 <= n <= SEG
    s = np.concatenate(([0], np.flatnonzero(d[1:] != d[:-1]) + 1))               # run starts
    e = np.concatenate((s[1:], [n]))
    r = e - s - 1                                                               # bytes behind the run's first literal
    full, rem = r // 258, r % 258
    tail = np.where(rem >= 3, 1, rem)                                           # one length symbol, or 0 .. 2 literals
    count = 1 + full + tail
    run = np.repeat(np.arange(s.size), count)
    j = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)     # the token's place within its run
    byte, full_t, rem_t = d[s][run], full[run], rem[run]
    is_tail_len = (j > full_t) & (rem_t >= 3)
    sym = np.where(j == 0, byte, np.where(j <= full_t, 285, np.where(is_tail_len, LEN_SYM[rem_t], byte)))
    eb = np.where(is_tail_len, LEN_EB[rem_t], 0)
    ev = np.where(is_tail_len, LEN_EV[rem_t], 0)
    return sym, eb, ev


def histogram(sym):
    h = np.bincount(sym, minlength=NSYM).astype(np.int64)
    h[EOB] += 1
    return h


def leaf_depths(weights):
    """The depth of every leaf of the Huffman tree of `weights` (ascending, at least two): two queues, ties take the leaf."""
    n = len(weights)
    assert n >= 2 and all(weights[i] <= weights[i + 1] for i in range(n - 1))
    w = list(weights)                                                          # nodes 0 .. n - 1 leaves, then internal ones as made
    parent = [-1] * (2 * n - 1)
    leaf, node = 0, n                                                          # next unused leaf, next unused internal node
    for new in range(n, 2 * n - 1):
        pair = []
        for _ in range(2):
            if leaf < n and (node >= new or w[leaf] <= w[node]):
                pair.append(leaf)
                leaf += 1
            else:
                pair.append(node)
                node += 1
        w.append(w[pair[0]] + w[pair[1]])
        parent[pair[0]] = parent[pair[1]] = new
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    return depth[:n]


def code_lengths(hist):
    """(lengths[286], info) of a histogram with at least two used symbols.  info: 'depth' the deepest leaf before the limit, 'trips' the
    limiter's steps, 'moved' the length l each step took a code from, 'clipped' the symbols deeper than 15."""
    hist = [int(v) for v in hist]
    assert len(hist) == NSYM
    used = sorted((c, s) for s, c in enumerate(hist) if c)                      # ascending (count, symbol)
    depths = leaf_depths([c for c, _ in used])
    nc = [0] * (MAXLEN + 1)
    for dpt in depths:
        nc[min(dpt, MAXLEN)] += 1
    total = sum(nc[l] << (MAXLEN - l) for l in range(1, MAXLEN + 1))
    moved = []
    while total > 1 << MAXLEN:
        nc[MAXLEN] -= 1
        l = max(k for k in range(1, MAXLEN) if nc[k])
        nc[l] -= 1
        nc[l + 1] += 2
        total -= 1
        moved.append(l)
    lengths = [0] * NSYM
    j = len(used)
    for l in range(1, MAXLEN + 1):                                              # shortest first, to the most frequent
        for _ in range(nc[l]):
            j -= 1
            lengths[used[j][1]] = l
    assert j == 0
    return lengths, dict(depth=max(depths), trips=len(moved), moved=moved, clipped=sum(dpt > MAXLEN for dpt in depths), used=len(used))


def canonical_codes(lengths):
    """code of every symbol with a length: counted up within a length in symbol order, shorter lengths first (RFC 1951 3.2.2)"""
    codes, code = [0] * len(lengths), 0
    for l in range(1, MAXLEN + 1):
        for s, ls in enumerate(lengths):
            if ls == l:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def _rev(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


def _pack(val, nb):
    """the fields (val[i] in nb[i] bits, least significant bit first) back to back -> bytes, the last one padded with zero bits"""
    val, nb = np.asarray(val, np.int64), np.asarray(nb, np.int64)
    idx = np.arange(nb.sum()) - np.repeat(np.cumsum(nb) - nb, nb)
    return np.packbits(((np.repeat(val, nb) >> idx) & 1).astype(np.uint8), bitorder="little").tobytes()


def coded_bits(hist, lengths):
    """T: the bits of the coded block up to and including end-of-block"""
    t = 17 + 19 * 3 + sum(4 if l <= 12 else 5 for l in lengths) + 4            # + the distance code's length 1
    for s, c in enumerate(hist):
        t += int(c) * (lengths[s] + (LEXT[s - 257] + 1 if s > 256 else 0))
    return t


def coded_size(T, final):
    return (T + 7) // 8 if final else (T + 3 + 7) // 8 + 4


def segment(seg, final):
    """(bytes, info) of one segment"""
    seg = bytes(seg)
    N = len(seg)
    sym, eb, ev = tokens(seg)
    hist = histogram(sym)
    lengths, info = code_lengths(hist)
    T = coded_bits(hist, lengths)
    coded = coded_size(T, final)
    info.update(N=N, T=T, coded=coded, stored=coded >= N + 5, final=final, hist=hist, lengths=lengths, tokens=(sym, eb, ev))
    if info["stored"]:
        return bytes([1 if final else 0]) + struct.pack("<HH", N, N ^ 0xFFFF) + seg, info
    codes = canonical_codes(lengths)
    L = np.array(lengths, np.int64)
    R = np.array([_rev(c, l) for c, l in zip(codes, lengths)], np.int64)         # Huffman codes enter the stream first bit first
    cl_len = [4] * 13 + [5] * 6
    cl_code = canonical_codes(cl_len)
    val = [(1 if final else 0) | (2 << 1) | (29 << 3) | (0 << 8) | (15 << 13)] + [cl_len[s] for s in CL_ORDER]
    nb = [17] + [3] * 19
    for l in lengths + [1]:
        val.append(_rev(cl_code[l], cl_len[l]))
        nb.append(cl_len[l])
    is_len = sym > 256
    val = np.concatenate((val, R[sym] | (ev << L[sym]), [R[EOB]]))              # code, extra bits, then the distance code: one 0 bit
    nb = np.concatenate((nb, L[sym] + eb + is_len, [L[EOB]]))
    assert int(nb.sum()) == T
    if not final:
        val, nb = np.concatenate((val, [0])), np.concatenate((nb, [3]))
    out = _pack(val, nb) + (b"" if final else b"\x00\x00\xff\xff")
    assert len(out) == coded
    return out, info


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def adler32(raw):
    d = np.frombuffer(bytes(raw), np.uint8).astype(np.uint64)
    n = d.size
    a = (1 + int(d.sum())) % 65521
    b = (n + int((d * np.arange(n, 0, -1, dtype=np.uint64)).sum())) % 65521      # below 2^64 for streams of tens of megabytes
    return (b << 16) | a


def stream_info(raw):
    """(the zlib stream, the info of every segment)"""
    raw = bytes(raw)
    assert raw
    parts, infos = [b"\x78\x01"], []
    for o in range(0, len(raw), SEG):
        z, info = segment(raw[o:o + SEG], o + SEG >= len(raw))
        parts.append(z)
        infos.append(info)
    parts.append(struct.pack(">I", adler32(raw)))
    return b"".join(parts), infos


def stream(raw) -> bytes:
    return stream_info(raw)[0]


def stream_of_image(img) -> bytes:
    return stream(scanlines(img))

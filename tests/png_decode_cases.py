"""The decoder's case table: zlib streams written bit by bit (tests/deflate_writer.py), by zlib itself and by the device encoder's CPU
model, each with the bytes it must inflate to -- or None -- and with what its NAME claims, as a predicate over the decoder's counters
(mav_png_status as a dict), so that a case which no longer reaches its corner fails instead of passing for another reason.

zlib is the judge: tests/test_png_decode_cases_cpu.py holds every case to zlib.decompress.  The raw bytes of a valid case start with a
byte 0 .. 4, so the device tests can send them as ONE image row (H = 1, W = raw size - 1, one channel) whose filter byte that is.

    python tests/png_decode_cases.py --dump FILE      the table as one binary file, for tools/inflate_check (format: dump())
"""
import os
import struct
import sys
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_writer as dw      # noqa: E402
import png_device_model as model  # noqa: E402

E = dict(HEADER=1, TRUNCATED=2, BLOCK_TYPE=3, STORED_LEN=4, CODE_LENGTHS=5, SYMBOL=6, DISTANCE=7, OVERFLOW=8, SHORT=9, ADLER=10, FILTER=11)
STATUS_DTYPE = np.dtype([("code", "<i4"), ("adler_stream", "<u4"), ("adler_computed", "<u4"), ("blocks", "<u4", (3,)), ("consumed", "<u8"),
                         ("produced", "<u8"), ("max_length", "<u4"), ("max_distance", "<u4")])
assert STATUS_DTYPE.itemsize == 48


@dataclass(frozen=True)
class Case:
    name: str
    stream: bytes
    raw: Optional[bytes]                  # what it inflates to; None: it must be refused
    raw_size: int                         # the size the decoder is told to produce
    claim: Callable[[dict], bool]         # what the name says, read off the counters
    code: int = 0                         # the MAV_PNG_E_* a refused case must carry (0: valid)


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _scanlines(W, H, ch, seed, smooth=True):
    """an image's filtered scanline stream with all five filter types in turn (the bytes are arbitrary; only inflate reads them here)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W * ch]
    body = ((x * 3 + y * 5) // 7 + (rng.integers(0, 3, (H, W * ch)) if smooth else rng.integers(0, 256, (H, W * ch)))) & 255
    rows = np.empty((H, 1 + W * ch), np.uint8)
    rows[:, 0] = np.arange(H) % 5
    rows[:, 1:] = body
    return rows.tobytes()


def _z(build, data, **kw):
    """header, the blocks `build` writes, trailer"""
    w = dw.Writer().header(**{k: v for k, v in kw.items() if k in ("cmf", "fdict", "fcheck")})
    build(w)
    return w.trailer(data, wrong=kw.get("wrong_adler", False)).done()


def _valid_cases():
    C = []

    def add(name, stream, raw, claim):
        assert raw and raw[0] <= 4, name
        C.append(Case(name, bytes(stream), bytes(raw), len(raw), claim))

    # -- stored blocks
    big = b"\x00" + _noise(65534, 1)
    raw = b"\x00" + big
    add("stored_len_0_1_65535", _z(lambda w: w.stored(b"").stored(b"\x00").stored(big).stored(b"", final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (4, 0, 0) and s["produced"] == 65536 and s["max_length"] == 0)
    lits = [0] + list(range(1, 63))
    tail = [9, 8, 7, 6, 5]
    raw = bytes(lits) + b"stored-ten" + bytes(tail)
    add("stored_straddles_token_batch", _z(lambda w: w.fixed(lits).stored(b"stored-ten").fixed(tail, final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (1, 2, 0) and s["produced"] == 63 + 10 + 5)
    # -- fixed only
    toks = [0, 1, 2, 3, (4, 2), 200, 255, (10, 6)]
    raw = dw.expand(toks)
    add("fixed_block_only", _z(lambda w: w.fixed(toks, final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (0, 1, 0) and s["max_length"] == 10 and s["max_distance"] == 6)
    # -- dynamic: a code of length 15 (the chain 1, 2, ..., 14, 15, 15 over the literals 0 .. 14 and end-of-block)
    ll = [0] * 257
    for i in range(15):
        ll[i] = i + 1
    ll[256] = 15
    toks = list(range(15)) + [14, 14, 0]
    raw = dw.expand(toks)
    add("dynamic_code_of_length_15", _z(lambda w: w.dynamic(toks, ll, [1], final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (0, 0, 1) and s["produced"] == 18 and s["max_length"] == 0)
    # -- one distance code (length 1: an incomplete set zlib accepts)
    ll = dw.complete_lengths([0, 5, 6, 256, 257, 258], 259)
    toks = [0, 5, 6, (3, 1), (4, 1), 5]
    raw = dw.expand(toks)
    add("one_distance_code", _z(lambda w: w.dynamic(toks, ll, [1], final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (0, 0, 1) and s["max_distance"] == 1 and s["max_length"] == 4)
    # -- no distance code at all, literals only
    ll = dw.complete_lengths([0, 1, 2, 256], 257)
    toks = [0, 1, 2, 2, 1, 0]
    raw = dw.expand(toks)
    add("no_distance_code_literals_only", _z(lambda w: w.dynamic(toks, ll, [0], final=True), raw), raw,
        lambda s: tuple(s["blocks"]) == (0, 0, 1) and s["max_length"] == 0 and s["produced"] == 6)
    # -- a repeat code running from the literal/length lengths into the distance lengths: ... 3 (symbol 256) | 3 3 3 3 3 3 3 3
    ll = [0] * 258
    ll[0] = ll[1] = 4                        # 2 / 16 + 7 / 8 = 1: complete
    for sym in (2, 3, 4, 5, 6, 256, 257):
        ll[sym] = 3
    dl = [3] * 8
    syms = dw.rle_lengths(ll + dl)
    assert any(s == 16 for s, _, _ in syms)
    # the run 3 3 | 3 3 3 3 3 3 3 3 (256, 257, then the distance set) is one length 3 and repeats: a 16 that starts in the first set
    toks = [0, 1, 2, 3, (3, 4), (3, 7), 6]
    raw = dw.expand(toks)
    z = _z(lambda w: w.dynamic(toks, ll, dl, final=True), raw)
    add("repeat_code_crosses_into_distance_lengths", z, raw,
        lambda s: tuple(s["blocks"]) == (0, 0, 1) and s["max_distance"] == 7 and s["produced"] == 11)
    # -- the extremes of a match
    toks = [0, (258, 1)]
    raw = dw.expand(toks)
    add("match_258_at_distance_1", _z(lambda w: w.fixed(toks, final=True), raw), raw,
        lambda s: s["max_length"] == 258 and s["max_distance"] == 1 and s["produced"] == 259)
    head = b"\x00" + _noise(32767, 2)
    raw = dw.expand([(3, 32768)], head)
    add("distance_32768_at_position_32768", _z(lambda w: w.stored(head).fixed([(3, 32768)], final=True), raw), raw,
        lambda s: s["max_distance"] == 32768 and s["produced"] == 32768 + 3 and tuple(s["blocks"]) == (1, 1, 0))
    toks = [0, 7, 9, (3, 3)]
    raw = dw.expand(toks)
    add("distance_equal_to_position", _z(lambda w: w.fixed(toks, final=True), raw), raw,
        lambda s: s["max_distance"] == 3 and s["produced"] == 6 and s["max_length"] == 3)
    toks = [0, 1, 2, 3, 4, (13, 5)]
    raw = dw.expand(toks)
    add("overlapping_match_distance_not_dividing_length", _z(lambda w: w.fixed(toks, final=True), raw), raw,
        lambda s: s["max_distance"] == 5 and s["max_length"] == 13 and 13 % 5 != 0)
    toks = [0] + [(i * 7) & 255 for i in range(1, 63)] + [(100, 7), (150, 33), 1, 2, (70, 64), 3]
    raw = dw.expand(toks)
    add("match_split_across_token_batch", _z(lambda w: w.fixed(toks, final=True), raw), raw,
        lambda s: s["max_length"] == 150 and s["produced"] == 63 + 100 + 150 + 2 + 70 + 1)
    # -- a sync-flush marker (an empty stored block) followed by an empty final block
    raw = _scanlines(40, 9, 3, 3)
    co = zlib.compressobj(6)
    z = co.compress(raw) + co.flush(zlib.Z_SYNC_FLUSH) + co.flush(zlib.Z_FINISH)
    add("sync_flush_then_empty_final_block", z, raw, lambda s: s["blocks"][0] == 1 and sum(s["blocks"]) == 3)
    # -- where the last block ends: a fixed block is 3 + 8 a + 9 b + 7 bits for a literals below 144 and b above
    for name, toks in (("ends_on_byte_boundary", [0, 1, 2] + [200] * 6), ("ends_mid_byte", [0, 1, 2] + [200] * 3)):
        w = dw.Writer().header()
        w.fixed(toks, final=True)
        assert (w.bit_length % 8 == 0) == (name == "ends_on_byte_boundary")
        raw = dw.expand(toks)
        z = w.trailer(raw).done()
        add(name, z, raw, lambda s, n=len(z): s["consumed"] == n and tuple(s["blocks"]) == (0, 1, 0))
    toks = [0, 4, 4, (5, 1)]
    raw = dw.expand(toks)
    z = _z(lambda w: w.fixed(toks, final=True), raw)
    add("trailing_bytes_after_adler", z + b"trailing junk", raw, lambda s, n=len(z): s["consumed"] == n)
    # -- zlib's own streams
    img = _scanlines(61, 37, 3, 4)
    for level in (0, 1, 6, 9):
        add(f"zlib_level_{level}", zlib.compress(img, level), img,
            (lambda s: s["blocks"][0] >= 1 and s["max_length"] == 0) if level == 0 else (lambda s: s["blocks"][1] + s["blocks"][2] >= 1 and s["max_length"] >= 3))
    for name, strategy in (("Z_RLE", zlib.Z_RLE), ("Z_FIXED", zlib.Z_FIXED)):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
        flat = _scanlines(64, 16, 1, 5)[:300] + bytes(700) + _scanlines(64, 16, 1, 5)[300:]
        add(f"zlib_strategy_{name}", co.compress(flat) + co.flush(), flat,
            (lambda s: s["max_distance"] == 1 and s["max_length"] == 258) if name == "Z_RLE" else (lambda s: s["blocks"][1] >= 1 and s["blocks"][2] == 0))
    noise = b"\x02" + _noise(70000, 6)
    add("zlib_noise_two_stored_blocks", zlib.compress(noise, 6), noise, lambda s: s["blocks"][0] >= 2)
    # -- the device encoder's streams (its CPU model): Sub-filtered rows, segments of 24576 bytes, byte-run matches
    rng = np.random.default_rng(7)
    flat_img = np.repeat(rng.integers(0, 256, (40, 30, 1), dtype=np.uint8), 3, axis=2)
    flat_img[:, 10:] = flat_img[:, 10:11]
    raw = model.scanlines(flat_img)
    add("device_model_coded_segment", model.stream(raw), raw, lambda s: s["blocks"][2] >= 1 and s["max_distance"] == 1)
    big_img = rng.integers(0, 256, (70, 131, 3), dtype=np.uint8)
    big_img[20:50] = 17
    raw = model.scanlines(big_img)
    add("device_model_two_segments", model.stream(raw), raw, lambda s: sum(s["blocks"]) >= 3 and s["produced"] == 70 * (1 + 131 * 3))
    return C


def _malformed_cases():
    # every refused case is asked for the SAME raw size N, so that the whole family fits one device call
    C = []
    toks = [0, 1, 2, 3, (4, 2), 200, 7, 8, (3, 1)]
    good = dw.expand(toks)
    N = len(good)
    assert N == 14

    def add(name, stream, code, claim=lambda s: True):
        C.append(Case(name, bytes(stream), None, N, claim, E[code]))

    body = lambda w: w.fixed(toks, final=True)                                      # noqa: E731
    add("header_fdict_set", _z(body, good, fdict=True), "HEADER", lambda s: s["produced"] == 0)
    add("header_cinfo_8", _z(body, good, cmf=0x88), "HEADER", lambda s: s["produced"] == 0)
    add("header_fcheck", _z(body, good, fcheck=False), "HEADER", lambda s: s["produced"] == 0)
    add("header_cm_7", _z(body, good, cmf=0x77), "HEADER", lambda s: s["produced"] == 0)

    def type3(w):
        w.fixed([0, 1]).block_header(True, 3)
    add("block_type_3", _z(type3, good), "BLOCK_TYPE", lambda s: s["produced"] == 2 and tuple(s["blocks"]) == (0, 1, 0))
    add("stored_length_complement_wrong", _z(lambda w: w.stored(good, final=True, nlen=0x1234), good), "STORED_LEN", lambda s: s["blocks"][0] == 1)
    ll = dw.complete_lengths([0, 1, 2, 256], 257)
    add("code_16_with_nothing_before_it", _z(lambda w: w.dynamic([0], ll, [0], final=True, cl_syms=[(16, 0, 2), (2, 0, 0), (0, 0, 0)],
                                                                   cl_lens=dw.complete_lengths([0, 2, 16], 19)), good), "CODE_LENGTHS",
        lambda s: s["blocks"][2] == 1 and s["produced"] == 0)
    over = [0] * 257
    over[0] = over[1] = over[256] = 1
    add("oversubscribed_set", _z(lambda w: w.dynamic([], over, [0], final=True, eob=False), good), "CODE_LENGTHS", lambda s: s["blocks"][2] == 1)
    inc = [0] * 257
    inc[0] = inc[256] = 2
    add("incomplete_literal_set", _z(lambda w: w.dynamic([0], inc, [0], final=True), good), "CODE_LENGTHS", lambda s: s["blocks"][2] == 1)
    inc_d = dw.complete_lengths([0, 1, 256, 257], 258)
    add("incomplete_distance_set_two_codes", _z(lambda w: w.dynamic([0], inc_d, [2, 2], final=True), good), "CODE_LENGTHS", lambda s: s["blocks"][2] == 1)
    noeob = dw.complete_lengths([0, 1, 2, 3], 257)
    add("missing_end_of_block_code", _z(lambda w: w.dynamic([0], noeob, [0], final=True, eob=False), good), "CODE_LENGTHS", lambda s: s["blocks"][2] == 1)
    add("too_many_length_codes", _z(lambda w: w.dynamic([0], dw.complete_lengths([0, 256], 288), [0], final=True), good), "CODE_LENGTHS",
        lambda s: s["blocks"][2] == 1)
    add("repeat_past_the_end", _z(lambda w: w.dynamic([0], ll, [0], final=True, cl_syms=dw.rle_lengths(ll) + [(18, 127, 7)],
                                                       cl_lens=dw.complete_lengths([0, 2, 17, 18], 19)), good), "CODE_LENGTHS", lambda s: s["blocks"][2] == 1)
    add("symbol_286", _z(lambda w: w.fixed([0, 1, ("ll", 286)], final=True), good), "SYMBOL", lambda s: s["produced"] == 2)
    add("distance_code_30", _z(lambda w: w.fixed([0, 1, 2, ("ll", 257), ("d", 30, 0, 0)], final=True), good), "SYMBOL", lambda s: s["produced"] == 3)
    one = dw.complete_lengths([0, 256, 257], 258)
    add("unused_code_of_a_one_code_distance_set", _z(lambda w: w.dynamic([0, ("ll", 257)] , one, [1], final=True, eob=False)
                                                      .bits(1, 1).bits(0, 15), good), "SYMBOL", lambda s: s["produced"] == 1)
    add("distance_of_position_plus_1", _z(lambda w: w.fixed([0, 1, 2, (3, 4)], final=True), good), "DISTANCE", lambda s: s["produced"] == 3)
    long_toks = toks + [9]
    add("output_one_byte_long", _z(lambda w: w.fixed(long_toks, final=True), dw.expand(long_toks)), "OVERFLOW", lambda s: s["produced"] == N)
    m_toks = [0, 1, (N - 1, 2)]
    add("output_one_byte_long_in_a_match", _z(lambda w: w.fixed(m_toks, final=True), dw.expand(m_toks)), "OVERFLOW", lambda s: s["produced"] == 2)
    add("output_one_byte_long_stored", _z(lambda w: w.stored(good + b"x", final=True), good + b"x"), "OVERFLOW",
        lambda s: s["produced"] == 0 and s["blocks"][0] == 1)
    short_toks = toks[:-1] + [8, 8]
    assert len(dw.expand(short_toks)) == N - 1
    add("output_one_byte_short", _z(lambda w: w.fixed(short_toks, final=True), dw.expand(short_toks)), "SHORT", lambda s: s["produced"] == N - 1)
    add("wrong_adler", _z(body, good, wrong_adler=True), "ADLER", lambda s: s["produced"] == len(good) and s["adler_computed"] == zlib.adler32(good)
        and s["adler_stream"] == zlib.adler32(good) ^ 1)
    # truncation at every byte of one short stream: a dynamic block, a stored block and a fixed block
    ll3 = dw.complete_lengths([0, 5, 6, 256, 257, 258], 259)
    t1, t3 = [0, 5, 6, (3, 1)], [6, (4, 2)]
    whole = dw.expand(t3, dw.expand(t1) + b"abc")
    zt = _z(lambda w: w.dynamic(t1, ll3, [1]).stored(b"abc").fixed(t3, final=True), whole)
    assert zlib.decompress(zt) == whole and len(whole) == N
    for k in range(len(zt)):
        add(f"truncated_at_{k:02d}_of_{len(zt)}", zt[:k], "TRUNCATED", lambda s, k=k: s["consumed"] <= k)
    return C


@lru_cache(maxsize=None)
def cases():
    return tuple(_valid_cases()) + tuple(_malformed_cases())


def valid_cases():
    return tuple(c for c in cases() if c.raw is not None)


def malformed_cases():
    return tuple(c for c in cases() if c.raw is None)


def filter_case():
    """FILTER is the un-filter pass's: a stream that inflates well to an image row whose filter byte is 5"""
    raw = b"\x05" + bytes(range(20))
    return Case("filter_byte_5", zlib.compress(raw, 6), raw, len(raw), lambda s: s["produced"] == 21, E["FILTER"])


def zlib_verdict(stream):
    """zlib.decompress's bytes, or None where it refuses the stream"""
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


def mutations(n, seed):
    """n seeded mutations of the valid streams: bit flips, truncations, spliced blocks (a stretch of one stream written over another)"""
    rng = np.random.default_rng(seed)
    src = [c for c in valid_cases() if len(c.stream) < 4000]
    out = []
    for _ in range(n):
        c = src[int(rng.integers(len(src)))]
        z = bytearray(c.stream)
        kind = int(rng.integers(4))
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                z[int(rng.integers(len(z)))] ^= 1 << int(rng.integers(8))
        elif kind == 1:
            z = z[:int(rng.integers(len(z)))]
        elif kind == 2:
            o = src[int(rng.integers(len(src)))].stream
            a, b = sorted(int(v) for v in rng.integers(0, len(o), 2))
            at = int(rng.integers(2, len(z)))
            z[at:at + (b - a)] = o[a:b]
        else:
            at = int(rng.integers(2, len(z)))
            z[at:at] = _noise(int(rng.integers(1, 9)), int(rng.integers(1 << 30)))
        out.append((bytes(z), c.raw_size))
    return out


# ---- the un-filter pass ------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 2), (63, 65), (64, 64), (65, 63), (300, 129))       # W x H: one pixel, one column, one row, the 64-row band and its edges
RAW_SHAPES = SHAPES[:7]                                                                   # where the per-byte numpy reference is affordable


def filter_types(k, H):
    """the filter type of every row of image k of 25: rows 0, 1 carry the ordered pair (k // 5, k % 5), rows 1, 2 the pair (k % 5, k // 5)
    -- over the 25 images both run through all 25 ordered pairs --, the rows below cycle"""
    f0, f1 = divmod(k, 5)
    return ([f0, f1, f0] + [(r + f0) % 5 for r in range(3, H)])[:H]


@lru_cache(maxsize=None)
def unfilter_images(W, H, bpp):
    """((25, H, W, bpp) u8 images, their raw scanline streams): even images are random bytes; odd ones are built for Paeth ties -- few
    distinct values at both ends of the byte range, in runs, so that |p - a| = |p - b| and |p - b| = |p - c| are common"""
    import unfilter_ref as ur
    rng = np.random.default_rng([W, H, bpp])
    imgs = rng.integers(0, 256, (25, H, W, bpp), dtype=np.uint8)
    ties = np.array([0, 1, 2, 128, 254, 255], np.uint8)[rng.integers(0, 6, (25, (H + 1) // 2, (W + 2) // 3, bpp))]
    ties = np.repeat(np.repeat(ties, 2, axis=1), 3, axis=2)[:, :H, :W]
    imgs[1::2] = ties[1::2]
    raws = tuple(ur.filter_rows(imgs[k].reshape(H, W * bpp), bpp, filter_types(k, H)) for k in range(25))
    imgs.setflags(write=False)
    return imgs, raws


@lru_cache(maxsize=None)
def unfilter_raw(W, H, bpp):
    """25 raw scanline streams of random bytes (odd ones from the tie set) under the same filter types, and what they un-filter to by
    tests/unfilter_ref.py: ((25, H, W, bpp) u8, raws)"""
    import unfilter_ref as ur
    rng = np.random.default_rng([W, H, bpp, 1])
    raws, outs = [], []
    for k in range(25):
        body = rng.integers(0, 256, (H, W * bpp), dtype=np.uint8)
        if k & 1:
            body = np.array([0, 1, 2, 128, 254, 255], np.uint8)[body % 6]
        rows = np.empty((H, 1 + W * bpp), np.uint8)
        rows[:, 0] = filter_types(k, H)
        rows[:, 1:] = body
        raws.append(rows.tobytes())
        outs.append(ur.unfilter(raws[-1], H, W * bpp, bpp).reshape(H, W, bpp))
    out = np.stack(outs)
    out.setflags(write=False)
    return out, tuple(raws)


def pack(streams):
    """(streams u8, index (n, 2) u64) of a list of zlib streams, back to back"""
    index, at = [], 0
    for z in streams:
        index.append((at, len(z)))
        at += len(z)
    return np.frombuffer(b"".join(streams) + b"\0", np.uint8), np.array(index, np.uint64).reshape(-1, 2)


def status_dict(rec):
    return {k: rec[k].tolist() for k in STATUS_DTYPE.names}


def inflate_host(lib, stream, raw_size):
    """mav_png_inflate_host: (the raw bytes written, the status as a dict)"""
    raw = np.zeros(max(1, raw_size), np.uint8)
    st = np.zeros(1, STATUS_DTYPE)
    z = np.frombuffer(bytes(stream) + b"\0", np.uint8)
    assert lib.mav_png_inflate_host(z.ctypes.data, len(stream), raw.ctypes.data, raw_size, st.ctypes.data) == 0
    return raw[:raw_size].tobytes(), status_dict(st[0])


def dump(path):
    """u32 count; per case: u32 name length, name, u64 raw size, i32 code, u64 stream length, stream, u64 raw length (0 for a refused
    case), raw -- little endian"""
    with open(path, "wb") as f:
        cs = cases() + (filter_case(),)
        f.write(struct.pack("<I", len(cs)))
        for c in cs:
            name = c.name.encode()
            code = 0 if c.name == "filter_byte_5" else c.code
            raw = c.raw or b""
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<QiQ", c.raw_size, code, len(c.stream)) + c.stream
                    + struct.pack("<Q", len(raw)) + raw)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
        print(f"{len(cases()) + 1} cases -> {sys.argv[2]}")
    else:
        sys.exit(__doc__)

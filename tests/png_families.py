"""The hostile inputs of the PNG encoder's model tests, written in the STREAM domain (the Sub-filtered scanline bytes the encoder sees) and
turned into gray images with png_device_model.image_of_stream.  tests/test_png_device_model_cpu.py proves on the CPU that every family
reaches what its name says; tests/test_gpu_png_model.py sends the same images through the device.  Everything is generated from seeds.

A family is a list of (name, image) with images of (H, W) gray or (H, W, C) u8.  Families whose images share a size are stacked into one
device call by the GPU test."""
import functools

import numpy as np

import png_device_model as model

SEG = model.SEG


def _head_rows(stream, W):
    """force the filter byte 01 at the head of every row of W + 1 bytes"""
    a = np.array(np.frombuffer(bytes(stream), np.uint8))
    a[::W + 1] = 1
    return a.tobytes()


def no_run_arrangement(counts, rng):
    """bytes with the given {value: count} and no two neighbours equal: most frequent first into the even places, then the odd ones"""
    order = sorted(counts, key=lambda v: (-counts[v], v))
    seq = np.repeat(np.array(order, np.uint8), [counts[v] for v in order])
    n = seq.size
    out = np.empty(n, np.uint8)
    half = (n + 1) // 2
    out[0::2], out[1::2] = seq[:half], seq[half:]
    assert n < 2 or (out[1:] != out[:-1]).all(), "a count above half of the bytes: runs cannot be avoided"
    return out


# ---- deep: histograms whose unrestricted Huffman tree is deeper than 15 ---------------------------------------------------------------
# A segment holds at most 24 576 bytes + end-of-block.  A Huffman tree of depth d needs a total count of at least Fibonacci(d + 2)
# (Fibonacci(22) = 17 711, Fibonacci(23) = 28 657), so 20 is the deepest tree ANY segment of this encoder can have: the depths here are 16,
# 17, 19 and that maximum.  Deeper trees exist only as bare histograms (test_png_device_model_cpu.py feeds them to the model's limiter).
DEEP_W = SEG - 2                                            # one row of 24 575 bytes: one segment, the filter byte and 24 574 literals


def strict_chain(k, bottom=2):
    """the smallest counts (ascending, `bottom` ones first) whose two-queue Huffman tree with ties to the leaf is one chain: every next
    leaf is heavier than the internal node made two steps before it"""
    w = [1] * (bottom + 1)
    while len(w) < k:
        w.append(sum(w[:-1]) + 1)
    return w


def _deep_hist(chain, fillers, total):
    """counts: the chain (its first two are end-of-block and the filter byte 01), then `fillers` equal symbols sharing what is left"""
    rest = total - sum(chain)
    if rest < 0 or (fillers == 0 and rest) or (fillers and rest < fillers * (chain[-1] + 1)):
        return None
    w = list(chain)
    if fillers:
        w += [rest // fillers + (1 if i < rest % fillers else 0) for i in range(fillers)]
    return w


def _hist_of_weights(w, rng):
    """weights w[0] = end-of-block, w[1] = the byte 01, the rest on seeded literal values other than 1"""
    vals = [int(v) for v in rng.permutation(np.r_[0, 2:256])[:len(w) - 2]]
    h = [0] * model.NSYM
    h[model.EOB], h[1] = w[0], w[1]
    for v, c in zip(vals, w[2:]):
        h[v] = c
    return h


def _deep_stream(want, seed, bottom=2):
    """a one-segment stream of DEEP_W + 1 bytes without runs whose histogram satisfies want(info); searched over chain length / fillers"""
    rng = np.random.default_rng(seed)
    total = DEEP_W + 2                                      # all literals + end-of-block
    for k in range(bottom + 2, bottom + 40):
        chain = strict_chain(k, bottom)
        for fillers in range(0, 60):
            w = _deep_hist(chain, fillers, total)
            if w is None or w[0] != 1 or w[1] != 1 or max(w) > (DEEP_W + 1) // 2 or len(w) > 256:
                continue
            h = _hist_of_weights(w, rng)
            if want(model.code_lengths(h)[1]):
                counts = {v: c for v, c in enumerate(h[:256]) if c and v != 1}
                return b"\x01" + no_run_arrangement(counts, rng).tobytes()
    raise AssertionError("no histogram found")


@functools.lru_cache(maxsize=None)
def deep():
    out = []
    for d in (16, 17, 19, 20):
        out.append((f"deep{d}", model.image_of_stream(_deep_stream(lambda i: i["depth"] == d, d), DEEP_W)))
    # many symbols at the bottom: more than 100 codes longer than 15 bits, so length 14 runs empty and the limiter moves codes from l < 14
    wide = _deep_stream(lambda i: i["clipped"] > 100 and i["moved"] and min(i["moved"]) < 14, 99, bottom=120)
    out.append(("deep-wide", model.image_of_stream(wide, DEEP_W)))
    return out


# ---- tiny -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny():
    out = [(f"1x1 value {v}", np.full((1, 1), v, np.uint8)) for v in (1, 0, 2, 255)]        # value 1: the stream 01 01, two used symbols
    rng = np.random.default_rng(11)
    out += [("1x7 ones", np.full((7, 1), 1, np.uint8)), ("1x7 noise", rng.integers(0, 256, (7, 1), dtype=np.uint8)),
            ("1x7 two values", rng.integers(0, 2, (7, 1), dtype=np.uint8)),
            ("1x1 bgr", np.array([[[1, 1, 1]]], np.uint8)), ("1x1 bgra", np.array([[[3, 2, 1, 0]]], np.uint8))]
    return out


# ---- runs -----------------------------------------------------------------------------------------------------------------------------
def _runs_stream(lengths):
    parts = [b"\x01", b"\xfe"]
    for k, L in enumerate(lengths):
        parts.append(bytes([10 + (k * 7) % 200]) * L)       # neighbouring runs differ (7 k mod 200 never repeats at once)
        parts.append(bytes([220 + k % 30]))                 # a separator that differs from both neighbours
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def runs_stream():
    """run lengths 1 .. 1100, then 4 .. 262 once more so that a run cut by a segment edge has a whole twin"""
    return _runs_stream(list(range(1, 1101)) + list(range(262, 3, -1)))


PLANT_FULL_SEGMENTS = 12
PLANT_TAIL = 10001
PLANT_OFFSETS = (-2, -1, 0, 1)                              # bits 62, 63 of the mask word before an edge, bits 0, 1 of the one behind it
PLANT_EVENTS = ("start", "end", "piece")


def part_of(n):
    """the bytes each of the encoder's four waves takes of a segment of n bytes"""
    return (-(-n // 4) + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def planted_stream():
    """(stream, plants): a background without runs; per full segment one run at a plain mask-word edge, one at each of the three interior
    wave-part edges and one at the segment's end, planted so that the run's start / its end / the edge between its first and second
    258-piece falls 2 or 1 bytes before the edge, on it, or 1 behind.  plants: dicts(anchor, event, off, s, e, at) -- the run is [s, e)
    and `at` the stream position of the event."""
    n = PLANT_FULL_SEGMENTS * SEG + PLANT_TAIL
    a = (2 + (np.arange(n) * 5) % 97).astype(np.uint8)
    a[0] = 1
    plants = []

    def plant(anchor, event, off, at):
        if event == "start":
            s, e = at, at + 40
        elif event == "end":
            s, e = at - 40, at
        else:
            s, e = at - 259, at + 40                        # literal at s, a 258-piece from s + 1, the next piece starts at `at`
        assert 1 <= s and e < n
        a[s:e] = 200 + len(plants) % 50
        plants.append(dict(anchor=anchor, event=event, off=off, s=s, e=e, at=at))

    for g in range(PLANT_FULL_SEGMENTS):
        event, off = PLANT_EVENTS[g // 4], PLANT_OFFSETS[g % 4]
        for anchor, B in (("word", 448), ("part1", 6144), ("part2", 12288), ("part3", 18432), ("segment", SEG)):
            plant(anchor, event, off, g * SEG + B + off)
    base, part = PLANT_FULL_SEGMENTS * SEG, part_of(PLANT_TAIL)
    plant("tail-part1", "start", -1, base + part - 1)
    plant("tail-part2", "end", 1, base + 2 * part + 1)
    plant("tail-part3", "piece", 0, base + 3 * part)
    return a.tobytes(), plants


@functools.lru_cache(maxsize=None)
def runs():
    a, b = runs_stream(), planted_stream()[0]
    return [("runs 1..1100", model.image_of_stream(a, len(a) - 1)), ("runs planted", model.image_of_stream(b, len(b) - 1))]


# ---- long rows ------------------------------------------------------------------------------------------------------------------------
def random_run_stream(rng, n, alphabet=256, long_every=40):
    """n bytes: runs of random lengths (mostly 1 .. 8, now and then up to 1500) of random values, neighbours differing"""
    lens = rng.integers(1, 9, n)
    big = rng.random(n) < 1.0 / long_every
    lens[big] = rng.integers(3, 1500, int(big.sum()))
    k = int(np.searchsorted(np.cumsum(lens), n)) + 1
    lens = lens[:k]
    vals = np.cumsum(rng.integers(1, alphabet, k)) % alphabet                  # steps of 1 .. alphabet - 1: never the same value twice
    return np.repeat(vals.astype(np.uint8), lens)[:n].tobytes()


@functools.lru_cache(maxsize=None)
def long_rows():
    out = []
    for W in (SEG - 2, SEG - 1, SEG, SEG + 1):              # a row of W + 1 bytes: the filter byte lands last, first and mid-segment
        rng = np.random.default_rng(W)
        out.append((f"{W}x3 gray", model.image_of_stream(_head_rows(random_run_stream(rng, 3 * (W + 1)), W), W)))
    out += [(f"60000x2 constant {v}", np.full((2, 60000), v, np.uint8)) for v in (200, 1, 0)]
    rng = np.random.default_rng(9000)
    g = model.image_of_stream(_head_rows(random_run_stream(rng, 3 * 9001, long_every=15), 9000), 9000)
    out.append(("9000x3 bgr", np.ascontiguousarray(np.stack([g, np.roll(g, 7, axis=1), 255 - g], -1))))
    return out


# ---- edge: the stored / coded decision near equality -----------------------------------------------------------------------------------
EDGE_W, EDGE_H = 4095, 8                                    # rows of 4096 bytes: a full, non-last segment of 6 rows and a last one of 2


def margin(seg, final):
    """coded bytes - (N + 5) of a segment: >= 0 means stored"""
    h = model.histogram(model.tokens(seg)[0])
    return model.coded_size(model.coded_bits(h, model.code_lengths(h)[0]), final) - (len(seg) + 5)


def _edge_pair(n, final, seed):
    """(stored, coded): noise of n bytes (row heads 01) with just as many bytes overwritten by one value that the margin changes sign"""
    rng = np.random.default_rng(seed)
    base = np.array(np.frombuffer(_head_rows(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), EDGE_W), np.uint8))
    order = rng.permutation(np.flatnonzero(np.arange(n) % (EDGE_W + 1) != 0))

    def build(m):
        a = base.copy()
        a[order[:m]] = 77
        return a.tobytes()

    lo, hi = 0, order.size                                  # margin(lo) >= 0 > margin(hi)
    assert margin(build(lo), final) >= 0 > margin(build(hi), final)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if margin(build(mid), final) >= 0:
            lo = mid
        else:
            hi = mid
    return build(lo), build(hi)


@functools.lru_cache(maxsize=None)
def edge():
    first = _edge_pair(SEG, False, 501)
    last = _edge_pair(EDGE_H * (EDGE_W + 1) - SEG, True, 502)
    out = []
    for i, a in enumerate(("stored", "coded")):
        for j, b in enumerate(("stored", "coded")):
            out.append((f"edge {a}+{b}", model.image_of_stream(first[i] + last[j], EDGE_W)))
    return out


FAMILIES = dict(deep=deep, tiny=tiny, runs=runs, long_rows=long_rows, edge=edge)


def all_cases():
    """[(family, name, image)]"""
    return [(f, n, img) for f, fn in FAMILIES.items() for n, img in fn()]

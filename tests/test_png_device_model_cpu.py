"""tests/png_device_model.py -- the CPU statement of the device PNG encoder's stream that tests/test_gpu_png_model.py compares the
device's bytes with -- is held here to references that are not the encoder (zlib's inflate and Adler-32, a heapq Huffman, Kraft's sum),
and every input family of tests/png_families.py proves that it reaches the part of the kernel it is named after.  No GPU."""
import heapq
import zlib

import numpy as np
import pytest

import png_device_model as model
import png_families as fam
import png_stream_ref as ref
from mavflow.frame_source import decode_png, png_wrap

SEG = model.SEG


def _inflates_to(z, raw):
    d = zlib.decompressobj()
    got = d.decompress(z)
    return got == raw and d.eof and d.unused_data == b"" and d.unconsumed_tail == b""


def _heap_huffman(hist):
    """(cost, depth) of a plain heapq Huffman tree of the used symbols"""
    h = [(int(c), s, 0) for s, c in enumerate(hist) if c]          # (weight, tie-break, depth of the subtree)
    heapq.heapify(h)
    cost, k = 0, len(hist)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a[0] + b[0]
        heapq.heappush(h, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return cost, h[0][2]


def _check_stream(raw, tag):
    """the model's stream of `raw` against zlib, Kraft and heapq; returns (stream, infos)"""
    z, infos = model.stream_info(raw)
    assert _inflates_to(z, raw), f"{tag}: zlib does not inflate the model's stream to its input"
    assert z[:2] == b"\x78\x01" and int.from_bytes(z[-4:], "big") == zlib.adler32(raw) == model.adler32(raw), tag
    assert len(infos) == -(-len(raw) // SEG) and sum(i["N"] for i in infos) == len(raw)
    size = 6
    for k, i in enumerate(infos):
        L = i["lengths"]
        assert max(L) <= 15 and sum(1 << (15 - l) for l in L if l) == 1 << 15, f"{tag} segment {k}: not a complete code of <= 15 bits"
        assert all((l > 0) == (c > 0) for l, c in zip(L, i["hist"])), f"{tag} segment {k}: a used symbol without a code, or the reverse"
        cost, depth = _heap_huffman(i["hist"])
        if depth <= 15 or i["depth"] <= 15:
            assert sum(int(c) * l for c, l in zip(i["hist"], L)) == cost, f"{tag} segment {k}: not a minimum-redundancy code"
            assert i["trips"] == 0
        n = i["N"] + 5 if i["stored"] else i["coded"]
        assert n <= i["N"] + 5 and i["stored"] == (i["coded"] >= i["N"] + 5) and i["final"] == (k == len(infos) - 1), f"{tag} segment {k}"
        size += n
    assert size == len(z), tag
    return z, infos


def _infos(img):
    return _check_stream(model.scanlines(img), "")[1]


# ---- the model against references that are not the encoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(fam.FAMILIES))
def test_every_family_inflates_with_complete_optimal_codes(family):
    for name, img in fam.FAMILIES[family]():
        raw = model.scanlines(img)
        z, _ = _check_stream(raw, name)
        a = img if img.ndim == 3 else img[:, :, None]
        px, _ = decode_png(png_wrap(a.shape[1], a.shape[0], a.shape[2], z))       # the project's own decoder: same pixels, file order
        want = a[:, :, 0] if a.shape[2] == 1 else a[:, :, [2, 1, 0] + ([3] if a.shape[2] == 4 else [])]
        assert np.array_equal(px, want), name


def _fuzz_stream(rng, k):
    kind = ("skewed", "geometric", "fibonacci", "flat")[k % 4]
    nseg = 1 + (k // 4) % 4
    n = int(rng.integers(1, SEG + 1)) + (nseg - 1) * SEG
    A = int(rng.choice([1, 2, 3, 5, 17, 60, 200, 256]))
    vals = rng.permutation(256)[:A]
    if kind == "skewed":
        p = 1.0 / np.arange(1, A + 1) ** rng.uniform(1.0, 3.0)
    elif kind == "geometric":
        p = rng.uniform(0.4, 0.9) ** np.arange(A)
    elif kind == "fibonacci":
        f = [1.0, 2.0]
        while len(f) < A:
            f.append(f[-1] + f[-2])
        p = np.array(f[:A][::-1])
    else:
        p = np.ones(A)
    a = np.array(vals[rng.choice(A, n, p=p / p.sum())], np.uint8)
    if k % 3:                                                  # a random run layout over it, in blocks
        runs = np.frombuffer(fam.random_run_stream(rng, n, long_every=int(rng.integers(5, 200))), np.uint8)
        bs = int(rng.integers(1, 500))
        keep = np.repeat(rng.random(n // bs + 1) < rng.uniform(0.0, 1.0), bs)[:n]
        a = np.where(keep, a, runs)
    return a.tobytes()


def test_seeded_fuzz_inflates_with_complete_optimal_codes():
    rng = np.random.default_rng(2024)
    used, depth, segs = set(), 0, set()
    streams = [_fuzz_stream(rng, k) for k in range(96)]
    streams += [b"\x01\x01", b"\x00", b"\x07\x07\x07", bytes(range(256)) * 3]
    for k in (17, 19, 21):                                     # exact Fibonacci-like counts without runs: trees of depth 16, 18, 20
        streams.append(fam.no_run_arrangement(dict(zip(rng.permutation(256)[:k - 1].tolist(), fam.strict_chain(k)[1:])), rng).tobytes())
    # every symbol at once: all literals, and runs whose pieces need each of the 29 length symbols
    streams.append(bytes(range(256)) * 8 + b"".join(bytes([k]) * (model.LBASE[k] + 1) + b"\xff" for k in range(29)))
    for k, raw in enumerate(streams):
        _, infos = _check_stream(raw, f"fuzz {k}")
        used |= {i["used"] for i in infos}
        depth = max(depth, max(i["depth"] for i in infos))
        segs.add(len(infos))
    print(f"fuzz: used symbols {min(used)} .. {max(used)}, deepest unrestricted tree {depth}, segments {sorted(segs)}")
    assert min(used) == 2 and max(used) == 286 and segs == {1, 2, 3, 4}
    assert depth == 20, "no fuzz histogram reaches the deepest tree a segment can have"


def test_limiter_on_bare_histograms_deeper_than_any_segment():
    """A segment's counts sum to at most 24 577, and a Huffman tree of depth d needs Fibonacci(d + 2) of them: 20 is the deepest tree the
    device can meet (the deep family has it).  The model's limiter is the statement of the rule for ANY histogram, so it is also run
    here on what no segment can hold: chains of depth 22, 25 and 31, and 2 000 random skewed histograms."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    assert fib[21] == 17711 <= SEG + 1 < fib[22] == 28657          # fib[k] here is Fibonacci(k + 1): depth 20 fits, depth 21 does not
    deepest = 0
    for d in (16, 20, 22, 25, 31):
        h = [0] * model.NSYM
        for s, c in enumerate(fam.strict_chain(d + 1)):
            h[s] = c
        L, info = model.code_lengths(h)
        assert info["depth"] == d and max(L) == 15 and sum(1 << (15 - l) for l in L if l) == 1 << 15
        deepest = max(deepest, info["depth"])
    rng = np.random.default_rng(7)
    trips = 0
    for k in range(2000):
        n = int(rng.integers(2, model.NSYM + 1))
        h = np.zeros(model.NSYM, np.int64)
        base = rng.uniform(1.2, 2.2)
        h[rng.permutation(model.NSYM)[:n]] = 1 + (base ** rng.uniform(0, 30, n)).astype(np.int64)
        L, info = model.code_lengths(h)
        assert max(L) <= 15 and sum(1 << (15 - l) for l in L if l) == 1 << 15, k
        assert all((l > 0) == (c > 0) for l, c in zip(L, h))
        order = sorted(range(model.NSYM), key=lambda s: (h[s], s))
        assert all(L[a] >= L[b] for a, b in zip(order, order[1:]) if h[a]), "a rarer symbol with a shorter code"
        deepest, trips = max(deepest, info["depth"]), max(trips, info["trips"])
    print(f"bare histograms: deepest {deepest}, most limiter steps {trips}")
    assert deepest >= 31 and trips > 100


def test_scanlines_and_image_of_stream():
    rng = np.random.default_rng(3)
    for C in (1, 3, 4):
        img = rng.integers(0, 256, (5, 9, C), dtype=np.uint8)
        file_order = img if C == 1 else img[:, :, [2, 1, 0] + ([3] if C == 4 else [])]
        assert model.scanlines(img) == ref.sub_rows(np.ascontiguousarray(file_order))
    assert model.scanlines(np.full((2, 3), 7, np.uint8)) == bytes([1, 7, 0, 0]) * 2
    raw = fam._head_rows(rng.integers(0, 256, 6 * 11, dtype=np.uint8).tobytes(), 10)
    img = model.image_of_stream(raw, 10)
    assert img.shape == (6, 10) and img.dtype == np.uint8 and model.scanlines(img) == raw
    assert model.image_of_stream(b"\x01\x01", 1).tolist() == [[1]] and model.image_of_stream(b"\x01\xff\x02", 2).tolist() == [[255, 1]]
    with pytest.raises(AssertionError):
        model.image_of_stream(b"\x00\x05", 1)                     # a row must start with the filter byte 01


def test_token_rule_by_hand():
    def toks(b):
        s, eb, ev = model.tokens(b)
        return list(zip(s.tolist(), eb.tolist(), ev.tolist()))
    assert toks(b"\x05" * 3) == [(5, 0, 0)] * 3                               # r = 2: literals
    assert toks(b"\x05" * 4) == [(5, 0, 0), (257, 0, 0)]                      # r = 3
    assert toks(b"\x05" * 259) == [(5, 0, 0), (285, 0, 0)]                    # r = 258
    assert toks(b"\x05" * 258) == [(5, 0, 0), (284, 5, 30)]                   # r = 257 = 227 + 30
    assert toks(b"\x05" * 261 + b"\x06") == [(5, 0, 0), (285, 0, 0), (5, 0, 0), (5, 0, 0), (6, 0, 0)]      # a tail of 2 behind a 258-piece
    assert toks(b"\x05" * 262) == [(5, 0, 0), (285, 0, 0), (257, 0, 0)]
    assert toks(b"\x09" + b"\x05" * 14) == [(9, 0, 0), (5, 0, 0), (266, 1, 0)]  # r = 13 = 13 + 0, one extra bit
    assert model.stream(b"\x01\x01") == bytes.fromhex("7801" "010200fdff0101" "00050003")


# ---- every family reaches its target ------------------------------------------------------------------------------------------------
def test_family_deep_reaches_the_limiter_at_every_depth():
    cases = dict(fam.deep())
    depths = {}
    for name, img in cases.items():
        assert img.shape == (1, fam.DEEP_W)
        raw = model.scanlines(img)
        assert (np.frombuffer(raw, np.uint8)[1:] != np.frombuffer(raw, np.uint8)[:-1]).all(), f"{name}: the stream has a run"
        (i,) = _infos(img)
        assert not i["stored"] and i["trips"] >= 1 and max(i["lengths"]) == 15
        depths[name] = i
        print(f"{name}: depth {i['depth']}, {i['used']} symbols, {i['clipped']} deeper than 15, limiter steps {i['trips']} from lengths {sorted(set(i['moved']))}")
    assert [depths[f"deep{d}"]["depth"] for d in (16, 17, 19, 20)] == [16, 17, 19, 20]
    assert depths["deep16"]["moved"] == [14]                              # the one trip the old suite reached, kept
    wide = depths["deep-wide"]
    assert wide["clipped"] > 100 and wide["trips"] > 40 and min(wide["moved"]) < 13 and wide["depth"] >= 16
    assert any(min(i["moved"]) < 14 for i in depths.values())


def test_family_tiny_has_two_symbols():
    infos = {name: _infos(img) for name, img in fam.tiny()}
    assert model.scanlines(fam.tiny()[0][1]) == b"\x01\x01" and infos["1x1 value 1"][0]["used"] == 2
    assert all(len(i) == 1 for i in infos.values())
    assert {i[0]["used"] for i in infos.values()} >= {2, 3}


def test_family_runs_uses_every_length_symbol_with_every_extra_value():
    raw = fam.runs_stream()
    seen, tails = set(), set()
    for o in range(0, len(raw), SEG):
        seg = raw[o:o + SEG]
        sym, eb, ev = model.tokens(seg)
        seen |= set(zip(sym[sym > 256].tolist(), ev[sym > 256].tolist()))
        tails |= {(e - s - 1) % 258 for s, e in _maximal_runs(seg).items() if e - s - 1 >= 258}      # what is left behind the 258-pieces
    want = {(257 + k, v) for k in range(29) for v in range(1 << model.LEXT[k])} - {(284, 31)}      # 227 + 31 = 258 is symbol 285's length
    assert want == {(int(model.LEN_SYM[n]), int(model.LEN_EV[n])) for n in range(3, 259)}
    assert seen == want, sorted(want - seen)
    assert tails >= {0, 1, 2}
    lens = sorted(set(np.diff(np.flatnonzero(np.diff(np.frombuffer(raw, np.uint8).astype(int)) != 0)).tolist()))
    assert set(range(1, 1101)) <= set(lens)


def _maximal_runs(raw):
    d = np.frombuffer(raw, np.uint8)
    s = np.concatenate(([0], np.flatnonzero(d[1:] != d[:-1]) + 1))
    return dict(zip(s.tolist(), np.concatenate((s[1:], [d.size])).tolist()))


def test_family_runs_plants_events_on_every_edge():
    raw, plants = fam.planted_stream()
    runs = _maximal_runs(raw)
    long_runs = {s: e for s, e in runs.items() if e - s > 1}
    assert long_runs == {p["s"]: p["e"] for p in plants}, "the background has runs of its own, or a plant is not a maximal run"
    nfull = fam.PLANT_FULL_SEGMENTS
    assert len(raw) == nfull * SEG + fam.PLANT_TAIL and fam.part_of(SEG) == 6144 and fam.part_of(fam.PLANT_TAIL) == 2560
    seen = {}
    for p in plants:
        at = {"start": p["s"], "end": p["e"], "piece": p["s"] + 1 + 258}[p["event"]]
        assert at == p["at"] and (p["event"] != "piece" or p["e"] - at >= 3)
        seg, pos = divmod(at - p["off"], SEG)                  # the edge itself, within its segment
        n = SEG if seg < nfull else fam.PLANT_TAIL
        part = fam.part_of(n)
        edge = {"word": pos % 64 == 0 and pos % part != 0, "part1": pos == part, "part2": pos == 2 * part, "part3": pos == 3 * part,
                "segment": pos == 0 and seg >= 1}
        kind = p["anchor"].replace("tail-", "")
        assert edge[kind], p
        seen.setdefault((p["anchor"], p["event"]), set()).add(at % 64)
    for anchor in ("word", "part1", "part2", "part3", "segment"):
        for event in fam.PLANT_EVENTS:
            assert seen[(anchor, event)] == {62, 63, 0, 1}, (anchor, event)
    assert {k[0] for k in seen if k[0].startswith("tail")} == {"tail-part1", "tail-part2", "tail-part3"}
    # and runs that lie across a segment edge: cut there, the second half starts again with a literal
    crossing = [p for p in plants if p["s"] // SEG != (p["e"] - 1) // SEG]
    assert len(crossing) >= 6


def test_family_long_rows_put_the_filter_byte_everywhere_and_a_segment_inside_a_run():
    cases = dict(fam.long_rows())
    where = set()
    for W in (SEG - 2, SEG - 1, SEG, SEG + 1):
        img = cases[f"{W}x3 gray"]
        assert img.shape == (3, W)
        _infos(img)
        pos = (W + 1) % SEG                                     # where the second row's filter byte falls in its segment
        where.add("last" if pos == SEG - 1 else "first" if pos == 0 else "mid")
    assert where == {"last", "first", "mid"}
    for v in (200, 1, 0):
        img = cases[f"60000x2 constant {v}"]
        raw = model.scanlines(img)
        inside = none_start = 0
        for k, o in enumerate(range(0, len(raw), SEG)):
            seg = raw[o:o + SEG]
            one_value = len(set(seg)) == 1
            inside += one_value and o > 0 and raw[o - 1] == seg[0] and o + SEG < len(raw) and raw[o + SEG] == seg[0]
            none_start += one_value                               # no run start behind position 0: every mask word but the first is empty
        assert inside >= 1 and none_start >= 1, v
        assert len(_infos(img)) == 5
    assert cases["9000x3 bgr"].shape == (3, 9000, 3) and 9000 * 3 + 1 > SEG
    _infos(cases["9000x3 bgr"])
    b = cases["9000x3 bgr"]
    assert not np.array_equal(b[:, :, 0], b[:, :, 2])               # a B <-> R mix-up would show


def test_family_edge_sits_on_both_sides_of_both_formulae():
    seen = set()
    for name, img in fam.edge():
        assert img.shape == (fam.EDGE_H, fam.EDGE_W)
        first, last = _infos(img)
        for i in (first, last):
            m = i["coded"] - (i["N"] + 5)
            assert -16 <= m <= 16, (name, m)
            assert i["stored"] == (m >= 0)
            seen.add((i["final"], i["stored"]))
            print(f"{name}: {'last' if i['final'] else 'non-last'} segment of {i['N']}: coded {i['coded']} against {i['N'] + 5}")
        assert name == f"edge {'stored' if first['stored'] else 'coded'}+{'stored' if last['stored'] else 'coded'}"
        assert first["coded"] == (first["T"] + 3 + 7) // 8 + 4 and last["coded"] == (last["T"] + 7) // 8
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_header_uses_the_five_bit_code_length_codes():
    lens = set()
    for _, _, img in fam.all_cases():
        for i in model.stream_info(model.scanlines(img))[1]:
            if not i["stored"]:
                lens |= set(i["lengths"])
    print(f"code lengths in coded segments: {sorted(lens)}")
    assert {0, 13, 14, 15} <= lens and lens & set(range(1, 13))


def test_families_share_sizes_for_the_batched_calls():
    shapes = {}
    for f, name, img in fam.all_cases():
        shapes.setdefault((f, img.shape), []).append(name)
    groups = {k: v for k, v in shapes.items() if len(v) > 1}
    assert {k[0] for k in groups} == {"deep", "tiny", "long_rows", "edge"}
    assert len(groups[("deep", (1, fam.DEEP_W))]) == 5 and len(groups[("edge", (fam.EDGE_H, fam.EDGE_W))]) == 4

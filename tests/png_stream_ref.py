"""CPU statement of the device PNG encoder's segment format (not a performance model): Sub-filtered bytes -> literals + distance-1 run tokens -> one dynamic
Huffman block with a FIXED code-length code (13 symbols of 4 bits + 6 of 5), a single 1-bit distance code; segments joined by empty
stored blocks.  Checks that zlib inflates it."""
import heapq, struct, zlib
import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LEN = [4] * 13 + [5] * 6          # symbol s of the code-length alphabet has length CL_LEN[s]


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):               # LSB first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):              # Huffman code: MSB first
        self.put(int(format(c, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def canonical(lengths):
    codes, code = {}, 0
    for L in range(1, 16):
        for s, l in enumerate(lengths):
            if l == L:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def huff_lengths(freq):
    h = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    if len(h) == 1:
        h.append((1, 999, ((h[0][1] + 1) % len(freq),)))
    heapq.heapify(h)
    L = [0] * len(freq)
    k = 1000
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for s in a[2] + b[2]:
            L[s] += 1
        heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2]))
        k += 1
    assert max(L) <= 15
    return L


def tokens(data):
    i, n, out = 0, len(data), []
    while i < n:
        j = i + 1
        while j < n and data[j] == data[i]:
            j += 1
        run = j - i
        out.append(("lit", data[i]))
        run -= 1
        while run >= 3:
            l = min(run, 258)
            if run - l in (1, 2) and l > 5:
                l -= 3 - (run - l)        # leave a tail of 3 so it is a token too
            out.append(("run", l))
            run -= l
        out += [("lit", data[i])] * run
        i = j
    return out


def len_sym(l):
    for k in range(28, -1, -1):
        if l >= LBASE[k]:
            return 257 + k, l - LBASE[k], LEXT[k]


def segment(data, bits, final):
    toks = tokens(data)
    freq = [0] * 286
    freq[256] = 1
    for t, v in toks:
        freq[v if t == "lit" else len_sym(v)[0]] += 1
    f2 = list(freq)
    while True:
        try:
            L = huff_lengths(f2)
            break
        except AssertionError:
            f2 = [(v + 1) // 2 if v else 0 for v in f2]      # flatten the histogram until no code is longer than 15 bits
    codes = canonical(L)
    cl_codes = canonical(CL_LEN)
    start = len(bits.out)
    bits.put(1 if final else 0, 1)
    bits.put(2, 2)
    bits.put(286 - 257, 5)
    bits.put(0, 5)                     # HDIST = 0: one distance code
    bits.put(19 - 4, 4)
    for s in CL_ORDER:
        bits.put(CL_LEN[s], 3)
    for l in L + [1]:                  # 286 literal/length lengths, then the single distance code's length 1
        bits.code(cl_codes[l], CL_LEN[l])
    for t, v in toks:
        if t == "lit":
            bits.code(codes[v], L[v])
        else:
            s, e, eb = len_sym(v)
            bits.code(codes[s], L[s])
            bits.put(e, eb)
            bits.code(0, 1)            # distance symbol 0 (distance 1), no extra bits
    bits.code(codes[256], L[256])
    if not final:
        bits.put(0, 3)                 # empty stored block: BFINAL 0, BTYPE 00
        bits.align()
        bits.out += b"\x00\x00\xff\xff"
    else:
        bits.align()
    return len(bits.out) - start


def adler_part(b):
    a = np.frombuffer(b, np.uint8).astype(np.uint64)
    n = len(b)
    return int((1 + a.sum()) % 65521), int((n + (a * np.arange(n, 0, -1, dtype=np.uint64)).sum()) % 65521), n


def stream(raw, seg):
    bits = Bits()
    bits.out += b"\x78\x01"
    A, B = 1, 0
    for o in range(0, len(raw), seg):
        d = raw[o:o + seg]
        segment(d, bits, o + seg >= len(raw))
        a2, b2, n2 = adler_part(d)
        B = (B + b2 + n2 * (A - 1)) % 65521
        A = (A + a2 - 1) % 65521
    assert ((B << 16) | A) == zlib.adler32(raw)
    return bytes(bits.out) + struct.pack(">I", (B << 16) | A)


def sub_rows(img):
    H = img.shape[0]
    rows = img.reshape(H, -1).astype(np.int16)
    bpp = img.shape[2]
    d = rows.copy()
    d[:, bpp:] -= rows[:, :-bpp]
    out = np.empty((H, 1 + rows.shape[1]), np.uint8)
    out[:, 0] = 1
    out[:, 1:] = d & 255
    return out.tobytes()


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    H, W = 48, 640
    y, x = np.mgrid[0:H, 0:W]
    cases = {
        "const": np.full((H, W, 3), 7, np.uint8),
        "ramp": np.stack([(x // 3) % 256, (y * 5) % 256, (x + y) % 256], -1).astype(np.uint8),
        "smooth+noise": np.clip(np.stack([x / 3, y * 4, (x + y) / 4], -1) + rng.normal(0, 1.0, (H, W, 3)), 0, 255).astype(np.uint8),
        "noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
        "tiny": np.full((1, 1, 3), 9, np.uint8),
    }
    for name, img in cases.items():
        raw = sub_rows(img)
        z = stream(raw, 8 * (1 + W * 3))
        d = zlib.decompressobj()
        got = d.decompress(z)
        assert got == raw and d.eof and d.unused_data == b"", name
        print(f"{name:13s} raw {len(raw):7d}  proto {len(z):7d}  zlib1(no filter) {len(zlib.compress(img[:, :, ::-1].tobytes(), 1)):7d}  raw/proto {len(raw) / len(z):.1f}")

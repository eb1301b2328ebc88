"""Baseline JPEG decoding restated in numpy from the arithmetic libjpeg-turbo uses (jdhuff.c, jidctint.c, jdsample.c, jdcolor.c): the
judge of the decoder's SAMPLES and GRAY outputs, and itself held to Pillow's pixels by tests/test_jpeg_cases_cpu.py.  It shares no
code with the library: its own segment walk (walk()), its own bit reader, and whole-array IDCT, upsampling and colour conversion.

    walk(data)    -> dict of the segments up to SOS (what mav_jpeg_parse reports), ValueError for a file it cannot walk
    decode(data)  -> {"samples": (H, W, c), "bgr": (H, W, 3), "gray": (H, W)} uint8
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def walk(data: bytes) -> dict:
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    out = {"quant": {}, "dc": {}, "ac": {}, "restart_interval": 0, "components": None}
    pos = 2
    while True:
        if data[pos] != 0xFF:
            raise ValueError(f"no marker at {pos}")
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        L = (data[pos] << 8) | data[pos + 1]
        body = data[pos + 2:pos + L]
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                q = np.zeros(64, np.uint8)
                q[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                out["quant"][body[0] & 15] = q
                body = body[65:]
        elif m == 0xC4:
            while body:
                counts = np.frombuffer(body[1:17], np.uint8).copy()
                n = int(counts.sum())
                out["ac" if body[0] >> 4 else "dc"][body[0] & 15] = (counts, np.frombuffer(body[17:17 + n], np.uint8).copy())
                body = body[17 + n:]
        elif m == 0xC0:
            out["H"], out["W"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            out["components"] = [[body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c], 0, 0] for c in range(body[5])]
        elif m == 0xDD:
            out["restart_interval"] = (body[0] << 8) | body[1]
        elif m == 0xDA:
            for c in range(body[0]):
                out["components"][c][4], out["components"][c][5] = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
            out["components"] = [tuple(c) for c in out["components"]]
            out["entropy_offset"], out["entropy_bytes"] = pos + L, len(data) - pos - L
            return out
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise ValueError(f"marker {m:02X}")
        pos += L


class _Bits:
    def __init__(self, z: bytes):
        self.z, self.pos, self.acc, self.n = z, 0, 0, 0

    def bit(self) -> int:
        if self.n == 0:
            b = self.z[self.pos]
            self.pos += 1
            if b == 0xFF:
                while self.z[self.pos] == 0xFF:
                    self.pos += 1
                assert self.z[self.pos] == 0, "marker inside an MCU"
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def restart(self) -> None:
        self.n = 0
        while self.z[self.pos] == 0xFF and self.z[self.pos + 1] == 0xFF:
            self.pos += 1
        assert self.z[self.pos] == 0xFF and 0xD0 <= self.z[self.pos + 1] <= 0xD7
        self.pos += 2


def _table(counts, values):
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(counts[length - 1])):
            out[(length, code)] = int(values[p])
            code += 1
            p += 1
        code <<= 1
    return out


def _symbol(br, table) -> int:
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("no code")


def _extend(v: int, t: int) -> int:
    return v if t == 0 or v >= 1 << (t - 1) else v - (1 << t) + 1


def _pass(i, n):
    """the 8-point pass on the leading axis of an int64 array (8, ...)"""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3])
    return (out + (1 << (n - 1))) >> n


def _idct(blocks):
    """(n, 8, 8) dequantised int64 -> (n, 8, 8) uint8"""
    cols = _pass(np.moveaxis(blocks, 1, 0), 11)              # (row, n, col): the pass runs down the columns
    rows = _pass(np.moveaxis(cols, 2, 0), 18)                # (col, row, n)
    return np.clip(np.moveaxis(rows, (0, 1, 2), (2, 1, 0)) + 128, 0, 255).astype(np.uint8)


def _h2v1(p):
    """(h, w) int64 -> (h, 2 w): triangle filter along the row, the ends replicated"""
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for k, other in ((0, up), (1, down)):
        s = 3 * p + other
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[k::2, 0::2] = (3 * s + left + 8) >> 4
        out[k::2, 1::2] = (3 * s + right + 7) >> 4
        out[k::2, 0] = (4 * s[:, 0] + 8) >> 4
        out[k::2, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def decode(data: bytes) -> dict:
    f = walk(data)
    W, H, comps, ri = f["W"], f["H"], f["components"], f["restart_interval"]
    n = len(comps)
    hmax, vmax = (comps[0][1], comps[0][2]) if n == 3 else (1, 1)
    hv = [(c[1], c[2]) if n == 3 else (1, 1) for c in comps]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coef = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in hv]
    br = _Bits(data[f["entropy_offset"]:] + b"\xff\xd9")
    dc = [_table(*f["dc"][c[4]]) for c in comps]
    ac = [_table(*f["ac"][c[5]]) for c in comps]
    pred = [0] * n
    for m in range(mcux * mcuy):
        if ri and m and m % ri == 0:
            br.restart()
            pred = [0] * n
        my, mx = divmod(m, mcux)
        for c, (h, v) in enumerate(hv):
            for b in range(h * v):
                blk = coef[c][my * v + b // h, mx * h + b % h]
                t = _symbol(br, dc[c])
                pred[c] += _extend(br.bits(t), t)
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = _symbol(br, ac[c])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                    k += 1
    planes = []
    for c, (h, v) in enumerate(hv):
        bh, bw = coef[c].shape[:2]
        px = _idct((coef[c] * f["quant"][comps[c][3]].astype(np.int64)).reshape(-1, 8, 8)).reshape(bh, bw, 8, 8)
        plane = px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8).astype(np.int64)
        dw, dh = -(-W * h // hmax), -(-H * v // vmax)
        plane = plane[:dh, :dw]                              # the edge rules see the real downsampled size
        if hmax // h == 2:
            if dw <= 2:                                      # libjpeg replicates a component this narrow
                plane = np.repeat(np.repeat(plane, 2, 1), vmax // v, 0)
            else:
                plane = _h2v2(plane) if vmax // v == 2 else _h2v1(plane)
        planes.append(plane[:H, :W])
    samples = np.stack(planes, -1).astype(np.uint8)
    if n == 1:
        g = samples[..., 0]
        return {"samples": samples, "bgr": np.repeat(g[..., None], 3, 2), "gray": g}
    y, cb, cr = (planes[k] for k in range(3))
    cb, cr = cb - 128, cr - 128
    r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0, 255)
    b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    gray = (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14
    return {"samples": samples, "bgr": np.stack([b, g, r], -1).astype(np.uint8), "gray": gray.astype(np.uint8)}

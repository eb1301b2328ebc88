"""A small JPEG bit writer for the scans no encoder emits (tests/jpeg_cases.py): segments written by hand, Huffman symbols written one
by one.  The tables are the writer's own, not Annex K's: every DC category 0 .. 11 has a 4-bit code, and every AC symbol a baseline
encoder can emit (EOB, ZRL, run 0 .. 15 x size 1 .. 10) has an 8-bit code, so a symbol's bits are known without a table lookup in
the reader's head.  The all-ones codes stay unused, as T.81 asks."""
import struct

DC_COUNTS = [0, 0, 0, 12] + [0] * 12
DC_VALUES = list(range(12))
AC_VALUES = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
AC_COUNTS = [0] * 7 + [len(AC_VALUES)] + [0] * 8
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

SOI, EOI = b"\xff\xd8", b"\xff\xd9"


def codes(counts, values):
    """{symbol: (code, length)} of a canonical table"""
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[p]] = (code, length)
            code += 1
            p += 1
        code <<= 1
    return out


DC = codes(DC_COUNTS, DC_VALUES)
AC = codes(AC_COUNTS, AC_VALUES)


def seg(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def dqt(tq: int, table=None, pq: int = 0) -> bytes:
    """one table in zigzag order (all ones by default); pq = 1 writes 16-bit entries"""
    table = [1] * 64 if table is None else list(table)
    body = bytes([(pq << 4) | tq]) + (b"".join(struct.pack(">H", v) for v in table) if pq else bytes(table))
    return seg(0xDB, body)


def dht_table(tc: int, th: int, counts, values) -> bytes:
    return bytes([(tc << 4) | th]) + bytes(counts) + bytes(values)


def dht(*tables) -> bytes:
    """DHT with one or more (class, id, counts, values) tables in ONE segment"""
    return seg(0xC4, b"".join(dht_table(*t) for t in tables))


def sof(W: int, H: int, comps, marker: int = 0xC0, precision: int = 8) -> bytes:
    """comps: [(id, h, v, tq)]"""
    return seg(marker, struct.pack(">BHHB", precision, H, W, len(comps)) + b"".join(bytes([i, (h << 4) | v, q]) for i, h, v, q in comps))


def sos(comps, ss: int = 0, se: int = 63, ahal: int = 0) -> bytes:
    """comps: [(id, td, ta)]"""
    return seg(0xDA, bytes([len(comps)]) + b"".join(bytes([i, (d << 4) | a]) for i, d, a in comps) + bytes([ss, se, ahal]))


def dri(n: int) -> bytes:
    return seg(0xDD, struct.pack(">H", n))


class Scan:
    """entropy-coded bytes, most significant bit first; FF is stuffed as it leaves"""

    def __init__(self, dc=DC, ac=AC):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.dc_codes, self.ac_codes = dc, ac

    def bits(self, value: int, n: int) -> "Scan":
        for k in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((value >> k) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0
        return self

    @staticmethod
    def _size(v: int) -> int:
        return abs(v).bit_length()

    def _value(self, v: int) -> "Scan":
        s = self._size(v)
        return self.bits(v if v >= 0 else v + (1 << s) - 1, s)

    def dc(self, diff: int) -> "Scan":
        self.bits(*self.dc_codes[self._size(diff)])
        return self._value(diff)

    def ac(self, run: int, v: int) -> "Scan":
        self.bits(*self.ac_codes[(run << 4) | self._size(v)])
        return self._value(v)

    def zrl(self) -> "Scan":
        return self.bits(*self.ac_codes[0xF0])

    def eob(self) -> "Scan":
        return self.bits(*self.ac_codes[0x00])

    def pad(self) -> "Scan":
        """one bits up to the byte boundary"""
        if self.n:
            self.bits((1 << (8 - self.n)) - 1, 8 - self.n)
        return self

    def marker(self, m: int, fill: int = 0) -> "Scan":
        self.pad()
        self.out += b"\xff" * fill + bytes([0xFF, m])
        return self

    def done(self) -> bytes:
        self.pad()
        return bytes(self.out)


def gray_file(W: int, H: int, entropy: bytes, before_sof: bytes = b"", restart: int = 0, tables: bytes = None, tail: bytes = EOI) -> bytes:
    """a one-component file with the writer's tables and an all-ones quantisation table around `entropy`"""
    tables = dht((0, 0, DC_COUNTS, DC_VALUES), (1, 0, AC_COUNTS, AC_VALUES)) if tables is None else tables
    return (SOI + before_sof + dqt(0) + sof(W, H, [(1, 1, 1, 0)]) + tables + (dri(restart) if restart else b"") + sos([(1, 0, 0)])
            + entropy + tail)

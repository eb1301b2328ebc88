"""The JPEG decoder's case table: files from Pillow's encoder (libjpeg-turbo), scans written bit by bit (tests/jpeg_writer.py) and files
that must be refused, each with the pixels Pillow decodes it to -- or the MAV_JPEG_E_* it must carry -- and with what its NAME claims,
as a predicate over the decoder's counters (mav_jpeg_status as a dict), so that a case which no longer reaches its corner fails
instead of passing for another reason.

Pillow is the judge: tests/golden/jpeg_frames.npz (tests/make_jpeg_fixtures.py) holds every encoder-made file and, for every valid
case, np.asarray(Image.open(file)); tests/test_jpeg_cases_cpu.py compares live whenever Pillow imports.

HAND-WRITTEN MAGNITUDES stay where IDCT output + 128 lies within [-256, 639]: outside that range libjpeg's range table wraps, while
this decoder clamps (include/mavflow_jpeg.h), and the two would part ways for a reason no test here is about.

    python tests/jpeg_cases.py --dump FILE      the table as one binary file, for tools/jpeg_check.c (format: dump())
"""
import os
import struct
import sys
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_writer as jw      # noqa: E402

E = dict(TRUNCATED=1, CODE=2, COEF_INDEX=3, RESTART=4, UNSUPPORTED=5)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_frames.npz")

SIZES = [(1, 1), (9, 17), (16, 16), (33, 31), (8, 130), (37, 53), (70, 130)]
SAMPLINGS = ["444", "422", "420", "gray"]
OPTIONS = ["plain", "optimize", "rmb2", "rmr1"]


def pil_specs():
    """(name, W, H, sampling, quality, option) of every file Pillow's encoder writes for the table: each size in each sampling, the
    qualities and options taken in turn; the largest size stays off quality 100 (noise does not compress) to keep the fixture small"""
    specs = []
    for si, (W, H) in enumerate(SIZES):
        for sj, samp in enumerate(SAMPLINGS):
            k = si * 4 + sj
            q = [35, 90, 100][k % 3] if (W, H) != (70, 130) else [35, 90][sj % 2]
            opt = OPTIONS[(si + sj) % 4]
            specs.append((f"pil_{W}x{H}_{samp}_q{q}_{opt}", W, H, samp, q, opt))
    specs.append(("pil_37x53_444_q90_rmb2_wraps_rst7", 37, 53, "444", 90, "rmb2"))
    specs.append(("pil_33x31_420_q100_plain_long_codes", 33, 31, "420", 100, "plain"))
    specs.append(("pil_33x31_422_q100_rmr1", 33, 31, "422", 100, "rmr1"))
    specs.append(("pil_64x48_420_q90_rmr1", 64, 48, "420", 90, "rmr1"))
    specs.append(("pil_33x31_420_q90_rmb2", 33, 31, "420", 90, "rmb2"))
    specs.append(("pil_64x48_444_q90_plain", 64, 48, "444", 90, "plain"))
    specs.append(("pil_64x48_422_q35_rmb2", 64, 48, "422", 35, "rmb2"))
    return specs


@dataclass(frozen=True)
class Case:
    name: str
    file: bytes
    pixels: Optional[np.ndarray]          # np.asarray(Image.open(file)): (H, W, 3) RGB or (H, W) gray; None: it must be refused
    claim: Callable[[dict], bool]         # what the name says, read off the counters
    code: int = 0                         # the MAV_JPEG_E_* a refused case must carry (0: valid)
    parser: Optional[str] = None          # refused by mav_jpeg_parse: a word its reason must hold

    @property
    def bgr(self):
        return None if self.pixels is None else (np.repeat(self.pixels[..., None], 3, 2) if self.pixels.ndim == 2
                                                 else np.ascontiguousarray(self.pixels[..., ::-1]))


def _geometry(W, H, samp):
    hmax, vmax = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[samp]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    blocks = mcux * mcuy * (1 if samp == "gray" else hmax * vmax + 2)
    return mcux, mcuy, blocks


def _pil_claim(W, H, samp, q, opt):
    mcux, mcuy, blocks = _geometry(W, H, samp)
    mcus = mcux * mcuy
    intervals = {"plain": 1, "optimize": 1, "rmb2": -(-mcus // 2), "rmr1": mcuy}[opt]

    def claim(s):
        ok = s["mcus"] == mcus and s["intervals"] == intervals and s["consumed"] > 0
        if q == 100 and W >= 16 and H >= 16:                 # (a frame smaller than a block is padded with copies of its edge)
            ok = ok and s["nonzero"] >= 32 * blocks          # dense blocks
        if q == 35:
            ok = ok and s["nonzero"] <= 24 * blocks          # sparse blocks
        return ok
    return claim


# ---- scans written by hand: one component, all-ones quantisation, the writer's tables ---------------------------------------------------------
def _zrl_chain():
    return jw.Scan().dc(40).zrl().zrl().zrl().ac(14, -9).done()          # k: 1 -> 17 -> 33 -> 49 -> coefficient 63; no EOB behind it


def _full_block():
    s = jw.Scan().dc(-25)
    for k in range(1, 64):
        s.ac(0, 1 if k % 3 else -2)
    return s.done()


def _big_categories():
    """two blocks: DC difference 2047 (category 11) with AC 1023 (size 10), then DC difference -2047 with AC -1023"""
    return jw.Scan().dc(2047).ac(0, 1023).eob().dc(-2047).ac(0, -1023).eob().done()


def _stuffed_end():
    """two intervals of one MCU; the first interval's last byte is FF (stuffed), straight in front of RST0"""
    for diff in range(1, 300):
        s = jw.Scan().dc(diff).zrl().zrl().zrl().ac(14, 127)
        if s.n == 7:                                                     # seven value bits 1111111 + one padding bit
            first = bytes(s.pad().out)
            assert first.endswith(b"\xff\x00")
            s.marker(0xD0).dc(-3).eob()
            return s.done()
    raise AssertionError("no alignment found")


def _fill_bytes():
    return jw.Scan().dc(17).ac(2, 5).eob().marker(0xD0, fill=3).dc(-30).ac(0, -7).eob().done()


def hand_valid():
    """(name, file, claim)"""
    two = jw.Scan().dc(9).ac(1, -4).eob().dc(12).eob().done()
    bogus = jw.dht((1, 0, [0, 1] + [0] * 14, [0x00]))                   # an AC table 0 that a later DHT replaces
    both = jw.dht((0, 0, jw.DC_COUNTS, jw.DC_VALUES), (1, 0, jw.AC_COUNTS, jw.AC_VALUES))
    odd = jw.seg(0xFE, b"abc") + jw.seg(0xE5, b"1234567") + jw.seg(0xE0, b"x") + jw.seg(0xFE, b"")
    return [
        ("hand_zrl_chain_then_coefficient_63", jw.gray_file(8, 8, _zrl_chain()), lambda s: s["zrl"] >= 3 and s["nonzero"] == 2 and s["mcus"] == 1),
        ("hand_full_block_without_eob", jw.gray_file(8, 8, _full_block()), lambda s: s["nonzero"] == 64 and s["zrl"] == 0),
        ("hand_dc_category_11_ac_size_10", jw.gray_file(16, 8, _big_categories()), lambda s: s["nonzero"] == 4 and s["mcus"] == 2),
        ("hand_interval_ends_in_stuffed_ff", jw.gray_file(16, 8, _stuffed_end(), restart=1),
         lambda s: s["stuffed"] >= 1 and s["intervals"] == 2 and s["mcus"] == 2),
        ("hand_fill_bytes_before_markers", jw.gray_file(16, 8, _fill_bytes(), restart=1, tail=b"\xff\xff" + jw.EOI),
         lambda s: s["intervals"] == 2 and s["mcus"] == 2),
        ("hand_dri_larger_than_mcu_count", jw.gray_file(16, 8, two, restart=100), lambda s: s["intervals"] == 1 and s["mcus"] == 2),
        ("hand_two_tables_in_one_dht_and_a_redefinition", jw.gray_file(16, 8, two, tables=bogus + both),
         lambda s: s["mcus"] == 2 and s["max_code_len"] == 8),
        ("hand_com_and_appn_of_odd_lengths", jw.gray_file(16, 8, two, before_sof=odd), lambda s: s["mcus"] == 2),
    ]


def _entropy_offset(data: bytes) -> int:
    import jpeg_ref
    return jpeg_ref.walk(data)["entropy_offset"]


def _rst_positions(data: bytes):
    off = _entropy_offset(data)
    return [i for i in range(off, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def _patched(data: bytes, at: int, old: bytes, new: bytes) -> bytes:
    assert data[at:at + len(old)] == old
    return data[:at] + new + data[at + len(old):]


def refused(files):
    """(name, file, code, parser word or None, claim); files: the encoder-made files by name"""
    rst = files["pil_33x31_420_q90_rmb2"]
    plain_name = next(n for n in sorted(files) if n.startswith("pil_37x53_") and n.split("_")[-1] in ("plain", "optimize") and "gray" not in n)
    plain = files[plain_name]
    mcux, mcuy, _ = _geometry(37, 53, plain_name.split("_")[2])
    c444 = next(files[n] for n in sorted(files) if "_444_" in n and n.startswith("pil_33x31_"))
    off = _entropy_offset(plain)
    marks = _rst_positions(rst)
    assert len(marks) >= 2 and rst[marks[1] + 1] == 0xD1
    any_ = lambda s: True
    out = [
        ("cut_in_first_mcu", plain[:off + 3], E["TRUNCATED"], None, lambda s: s["mcus"] == 0),
        ("cut_in_last_mcu", plain[:-5], E["TRUNCATED"], None, lambda s: s["mcus"] == mcux * mcuy - 1),
        ("cut_inside_a_code", jw.gray_file(8, 8, jw.Scan().dc(3).bits(0b0000, 4).done()[:1], tail=b""), E["TRUNCATED"], None, lambda s: s["mcus"] == 0),
        ("sixteen_bits_that_are_no_code", jw.gray_file(8, 8, jw.Scan().dc(3).bits(0xFFFF, 16).bits(0, 32).done()), E["CODE"], None,
         lambda s: s["mcus"] == 0 and s["stuffed"] >= 1),
        ("run_past_coefficient_63", jw.gray_file(8, 8, jw.Scan().dc(3).zrl().zrl().zrl().ac(15, 1).eob().bits(0, 32).done()), E["COEF_INDEX"], None,
         lambda s: s["zrl"] == 3),
        ("restart_marker_missing", rst[:marks[1]] + rst[marks[1] + 2:], E["RESTART"], None, any_),
        ("restart_marker_wrong_number", _patched(rst, marks[1], b"\xff\xd1", b"\xff\xd5"), E["RESTART"], None, any_),
        ("restart_marker_surplus", rst[:-2] + bytes([0xFF, 0xD0 + len(marks) % 8]) + rst[-2:], E["RESTART"], None, any_),
        ("pil_progressive", files["pil_progressive"], E["UNSUPPORTED"], "SOF2", any_),
        ("pil_cmyk_four_components", files["pil_cmyk"], E["UNSUPPORTED"], "4 components", any_),
        ("luma_sampling_1x2", _luma_sampling(c444, 1, 2), E["UNSUPPORTED"], "sampling", any_),
        ("luma_sampling_4x1", _luma_sampling(c444, 4, 1), E["UNSUPPORTED"], "sampling", any_),
        ("dqt_16_bit", jw.SOI + jw.dqt(0, [1] * 64, pq=1) + jw.sof(8, 8, [(1, 1, 1, 0)]) + jw.sos([(1, 0, 0)]) + jw.EOI, E["UNSUPPORTED"], "16-bit", any_),
        ("sof1_extended", jw.SOI + jw.dqt(0) + jw.sof(8, 8, [(1, 1, 1, 0)], marker=0xC1) + jw.EOI, E["UNSUPPORTED"], "SOF1", any_),
        ("sof9_arithmetic", jw.SOI + jw.dqt(0) + jw.sof(8, 8, [(1, 1, 1, 0)], marker=0xC9) + jw.EOI, E["UNSUPPORTED"], "arithmetic", any_),
        ("dac_arithmetic_conditioning", jw.SOI + jw.seg(0xCC, b"\x00\x10") + jw.EOI, E["UNSUPPORTED"], "DAC", any_),
        ("twelve_bit_samples", jw.SOI + jw.dqt(0) + jw.sof(8, 8, [(1, 1, 1, 0)], precision=12) + jw.EOI, E["UNSUPPORTED"], "12-bit", any_),
        ("more_than_one_scan", _one_of_three(c444), E["UNSUPPORTED"], "more than one scan", any_),
        ("adobe_transform_0", c444[:2] + jw.seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00") + c444[2:], E["UNSUPPORTED"], "Adobe", any_),
        ("component_ids_rgb", _rgb_ids(c444), E["UNSUPPORTED"], "R, G, B", any_),
        ("scan_names_an_undefined_table", jw.SOI + jw.dqt(0) + jw.sof(8, 8, [(1, 1, 1, 0)]) + jw.dht((0, 0, jw.DC_COUNTS, jw.DC_VALUES))
         + jw.sos([(1, 0, 0)]) + jw.EOI, E["UNSUPPORTED"], "AC table 0", any_),
        ("spectral_selection_not_0_63", jw.gray_file(8, 8, b"\x00").replace(jw.sos([(1, 0, 0)]), jw.sos([(1, 0, 0)], se=5)), E["UNSUPPORTED"], "Ss, Se", any_),
        ("oversubscribed_code_set", jw.gray_file(8, 8, b"\x00", tables=jw.dht((0, 0, [3] + [0] * 15, [0, 1, 2]), (1, 0, jw.AC_COUNTS, jw.AC_VALUES))),
         E["UNSUPPORTED"], "over-subscribed", any_),
        ("segment_past_the_file", (jw.SOI + jw.dqt(0))[:-10], E["TRUNCATED"], "passes the file's end", any_),
    ]
    return out


def _segments(data: bytes):
    """[(marker, offset of the FF, length with the marker)] up to SOS"""
    pos, out = 2, []
    while True:
        m, L = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.append((m, pos, L + 2))
        if m == 0xDA:
            return out
        pos += L + 2


def _one_of_three(data: bytes) -> bytes:
    m, at, n = next(s for s in _segments(data) if s[0] == 0xDA)
    body = data[at + 4:at + n]
    return data[:at] + jw.seg(0xDA, bytes([1]) + body[1:3] + body[-3:]) + data[at + n:]


def _luma_sampling(data: bytes, h: int, v: int) -> bytes:
    out = bytearray(data)
    at = next(s for s in _segments(data) if s[0] == 0xC0)[1]
    out[at + 4 + 7] = (h << 4) | v
    return bytes(out)


def _rgb_ids(data: bytes) -> bytes:
    out = bytearray(data)
    for m, at, n in _segments(data):
        if m == 0xC0:
            for c, ch in enumerate(b"RGB"):
                out[at + 4 + 6 + 3 * c] = ch
        if m == 0xDA:
            for c, ch in enumerate(b"RGB"):
                out[at + 4 + 1 + 2 * c] = ch
    return bytes(out)


@lru_cache(maxsize=1)
def cases():
    z = np.load(GOLDEN, allow_pickle=False)
    files = {k[5:]: z[k].tobytes() for k in z.files if k.startswith("file_")}
    out = []
    for name, W, H, samp, q, opt in pil_specs():
        out.append(Case(name, files[name], z["px_" + name], _pil_claim(W, H, samp, q, opt)))
    for name, data, claim in hand_valid():
        out.append(Case(name, data, z["px_" + name], claim))
    for name, data, code, parser, claim in refused(files):
        out.append(Case(name, data, None, claim, code, parser))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def valid():
    return [c for c in cases() if c.code == 0]


def dump(path: str) -> None:
    """'JPGC', u32 count; per case: u32 name size, name, i32 code (0: valid), u8 refused-by-parser, u32 file size, file, u32 H, u32 W,
    u32 pixel bytes (0: none), the BGR pixels"""
    with open(path, "wb") as f:
        all_ = cases()
        f.write(b"JPGC" + struct.pack("<I", len(all_)))
        for c in all_:
            bgr = c.bgr
            px = b"" if bgr is None else bgr.tobytes()
            H, W = (0, 0) if bgr is None else bgr.shape[:2]
            f.write(struct.pack("<I", len(c.name)) + c.name.encode() + struct.pack("<iBI", c.code, c.parser is not None, len(c.file)) + c.file
                    + struct.pack("<III", H, W, len(px)) + px)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    else:
        for c in cases():
            print(f"{c.name:55s} {len(c.file):6d} bytes  code {c.code}  {'parser' if c.parser else ''}")

"""TEST INFRASTRUCTURE -- the frames, Farneback parameters and inputs at which every stage of the flow path is held to the oracle and
to the float64 restatement (tests/test_gpu_stages.py, tests/test_stage_ref64_cpu.py), and the kernel form each stage takes there.

The library dispatches a stage to one of several kernels on the layer's width, the parameters and the area ratio of the initial
flow.  Each case below names the forms it is there to reach; tests/test_gpu_stages.py::test_every_kernel_form_is_reached derives the
forms from the same predicates the dispatch uses (kernels_flow.hip launch_blur_iter / launch_polyexp / launch_blur_resize /
launch_initial_m, kernels_window.hip launch_area_resize_flow) and fails when a form of FORMS is no longer reached.

The sibling tables: tests/detect_cases.py (detection path, kernels_detect.hip), tests/sparse_cases.py (sparse path, kernels_lk.hip),
tests/window_cases.py (window search, kernels_window.hip) and tests/schedule_cases.py (the host scheduler's band, stream, strip and
M-slot forms, mavflow.cpp).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from initial_flow_ref import area_ratio

# every kernel form of the stages, as the dispatch names them
FORMS = {
    "sweep": {"fast<6>", "fast<6,false>", "generic<0>", "generic<0>+lds>64K"},
    "polyexp": {"polyexp<8>", "polyexp<7>", "polyexp<5>", "polyexp<0>"},
    "initial_m": {"mode0", "mode1", "mode2"},      # launch_initial_m: k_update_matrices<FlowSource::kind> -- ZERO, COARSER, FIELD
    "initial_flow": {"copy", "fast", "fast+remainder", "general"},
    "blur0": {"blur3_u8", "two-pass"},
    "blur": {"fused", "two-pass"},
}
# Not reached, on purpose:
#   k_blur_iter_generic<6> -- the winsize 12 / 13 sweep for a flow pointer that is 4-byte but not 8-byte aligned.  Every buffer the
#   library allocates, and every stage hook's, is aligned; only a caller's misaligned device pointer could select it, and tests do
#   not hand kernels misaligned device pointers.
UNTESTED = {"sweep": {"generic<6>"}}


def sweep_lds_bytes(winsize: int) -> int:
    """kernels_flow.hip blur_iter_lds_bytes: the generic sweep's 5 planes of (32 + 2m) x pitch floats, padded to a bank offset."""
    m = winsize // 2
    ext = 32 + 2 * m
    pitch = ext if ext & 1 else ext + 1
    p = ext * pitch
    while (p - ext) % 32:
        p += 1
    return 4 * 5 * p


def sweep_form(w: int, winsize: int) -> str:
    if winsize // 2 == 6:
        return "fast<6>" if w % 4 == 0 else "fast<6,false>"
    return "generic<0>+lds>64K" if sweep_lds_bytes(winsize) > 64 * 1024 else "generic<0>"


def polyexp_form(n: int) -> str:
    return f"polyexp<{n if n in (5, 7, 8) else 0}>"


def initial_flow_form(W: int, H: int, w: int, h: int) -> str:
    if (w, h) == (W, H):
        return "copy"
    _, ix, whole_x = area_ratio(W, w)
    _, iy, whole_y = area_ratio(H, h)
    if whole_x and whole_y:
        return "fast" if (ix * iy) % 4 == 0 else "fast+remainder"
    return "general"


def blur0_form(W: int, H: int) -> str:
    """launch_blur_resize at scale 1: the 3x3 u8 kernel (blur3_fast_ok) or the separable two-pass form."""
    return "blur3_u8" if W % 4 == 0 and W >= 8 and H >= 2 else "two-pass"


# ---- layer images: the dispatch of kernels_flow.hip launch_blur_resize / launch_blur_multi, restated -------------------------------
DEPTHS = {"u8": 1, "u16": 2, "f32": 4}           # bytes per pixel of a frame
DEPTH_DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
LDS_DEFAULT, LDS_TWO_PASS, LDS_HROWS = 64 * 1024, 48 * 1024, 48 * 1024
# bounds of a layer image (tests/test_gpu_stages.py, tests/test_gpu_depth.py, tests/test_gpu_blur_forms.py)
BLUR_ATOL = 1.6e-4          # u8 frames, layers k >= 1, |GPU - oracle|: measured 7.6e-5 (3840x2160); was 2e-4
# wide frames: max |GPU - checker| / max |checker|.  The GPU's Gaussian accumulates tap by tap with fused multiply-adds, the checker in
# OpenCV's symmetric form: a few float32 roundings apart.
F32_LAYER0_REL = 5e-7       # first MI355X measurement 1.34e-7 (float32, 333x227)
COARSE_REL = 2e-6           # first MI355X measurement 5.36e-7 (float32 layer 4, 3840x2160 / 5 levels)


def pyramid(W: int, H: int, pyr_scale: float, levels: int):
    """mavflow.cpp mav_create: (w, h, ksize) of every layer, layer 0 first.  A layer exists while both sides stay >= 32 px; sigma =
    (1 / scale - 1) / 2, ksize = cv_round(5 sigma) | 1, at least 3 (round() rounds half to even, as nearbyint does)."""
    n, scale = 0, 1.0
    for _ in range(levels):
        scale *= pyr_scale
        if W * scale < 32 or H * scale < 32:
            break
        n += 1
    out = []
    for k in range(n + 1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        out.append((round(W * scale), round(H * scale), max(round((1.0 / scale - 1) * 0.5 * 5) | 1, 3)))
    return out


def fused_blur_rows(H: int, h: int, ksize: int, th: int = 16) -> int:
    return int((th - 1) * (H / h)) + (ksize | 1) + 4


def fused_lds_bytes(rows: int, pitch_w: int, esize: int) -> int:
    return rows * 256 + (rows + 3) * 4 * pitch_w * esize


def staged_pitch_words(W: int, w: int, ksize: int) -> int:
    return (int(63 * (W / w)) + (ksize | 1) + 2 + 3) // 4 + 3


def blur_is_fused(W: int, H: int, w: int, h: int, ksize: int, esize: int) -> bool:
    """blur_resize_is_fused"""
    if (w, h) == (W, H) or ksize > 13 or H <= 2 * ksize or W <= 2 * ksize or fused_blur_rows(H, h, ksize) * 256 > LDS_HROWS:
        return False
    return esize == 1 or fused_lds_bytes(fused_blur_rows(H, h, ksize), staged_pitch_words(W, w, ksize), esize) <= LDS_DEFAULT


def fused_plan(W: int, H: int, w: int, h: int, ksize: int, quad: bool, esize: int):
    """fused_plan + fused_fast_ok: (tile height, staged rows, row pitch in quads -- 0: unstaged, dynamic LDS bytes, fast tile?).  Every
    layer past the first has its coordinate tables, so the fast tile asks for quad-addressable rows, a staged region and 5 or 13 taps."""
    pitch = staged_pitch_words(W, w, ksize)
    th, rows = 16, fused_blur_rows(H, h, ksize)
    may_be_fast = quad and ksize in (5, 13)
    if fused_lds_bytes(rows, pitch, esize) > LDS_DEFAULT:
        rows8 = fused_blur_rows(H, h, ksize, 8)
        if may_be_fast and fused_lds_bytes(rows8, pitch, esize) <= LDS_DEFAULT:
            th, rows = 8, rows8
        else:
            pitch = 0
    return th, rows, pitch, fused_lds_bytes(rows, pitch, esize), may_be_fast and pitch > 0


def two_pass_rows_blk(W: int, w: int, ksize: int, esize: int) -> int:
    """the rows_blk loop of launch_blur_resize: rows per staged block of k_blur_resize_h, 0 where even four rows exceed 48 KB"""
    row_bytes = staged_pitch_words(W, w, ksize) * 4 * esize
    rows_blk = 16
    while rows_blk > 4 and rows_blk * row_bytes > LDS_TWO_PASS:
        rows_blk >>= 1
    return rows_blk if rows_blk * row_bytes <= LDS_TWO_PASS else 0


def blur_form(W: int, H: int, layer, depth: str, two_pass: bool = False) -> str:
    """The code path launch_blur_resize takes for layer = (w, h, ksize) of W x H frames of `depth` whose rows are quad-addressable when
    W % 4 == 0 (frames the library stages itself; layer 0 is the layer of the frame's own size and carries sigma 0).  The names:
      3x3                               k_blur3
      fused/fast<KS>/th<TH>             k_blur_resize_fused<FP_FAST5 / FP_FAST13>: blur_fused_tile_fast<KS, TH>
      fused/generic/quad|px/ks<5|13|0>  <FP_GENERIC>, staged through stage_rows by quads or pixel by pixel; blur_h4_run<KS>, 0 = run-time
      fused/generic/unstaged/ks<5|n>    <FP_GENERIC> with pitch_w == 0: blur_h4 from global memory, its 5-tap branch or the general one
      two-pass/quad|px                  k_blur_resize_h (staged rows, tap pairs in LDS) + k_blur_resize_v
      two-pass/direct/ks<5|n>           k_blur_resize_h_direct (blur_h4 from global memory) + k_blur_resize_v"""
    w, h, ksize = layer
    esize, quad = DEPTHS[depth], W % 4 == 0
    if (w, h) == (W, H) and ksize == 3 and quad and W >= 8 and H >= 2:
        return "3x3"                             # (blur3_fast_ok.  Only layer 0 has the frame's size: pyramid() rounds a coarser one down)
    h4 = "ks5" if ksize == 5 else "ksn"
    if not two_pass and blur_is_fused(W, H, w, h, ksize, esize):
        th, _, pitch, _, fast = fused_plan(W, H, w, h, ksize, quad, esize)
        if fast:
            return f"fused/fast{ksize}/th{th}"
        if pitch == 0:
            return f"fused/generic/unstaged/{h4}"
        return f"fused/generic/{'quad' if quad else 'px'}/ks{ksize if ksize in (5, 13) else 0}"
    if two_pass_rows_blk(W, w, ksize, esize):
        return f"two-pass/{'quad' if quad else 'px'}"
    return f"two-pass/direct/{h4}"


def blur_coarse_name(form: str) -> str:
    """what mav_schedule_info calls the form a layer takes unforced"""
    return form.split("/")[0]


# every (depth, form) the dispatch can select; tests/test_stage_cases_cpu.py sweeps blur_form over frame sizes, pyramids and depths and
# finds no other.  Wide pixels take a fused tile only where the staged 64 x 16 region fits 64 KB, which no 13-tap layer does.
_BLUR_ALL_DEPTHS = {"3x3", "fused/fast5/th16", "fused/generic/quad/ks0", "fused/generic/px/ks5", "fused/generic/px/ks0",
                    "two-pass/quad", "two-pass/px"}
_BLUR_U8_ONLY = {"fused/fast13/th16", "fused/fast13/th8", "fused/generic/px/ks13", "fused/generic/unstaged/ksn"}
BLUR_FORMS = {f"{d}:{f}" for d in DEPTHS for f in _BLUR_ALL_DEPTHS} | {f"u8:{f}" for f in _BLUR_U8_ONLY} | {"f32:two-pass/direct/ksn"}
FORMS["blur_form"] = BLUR_FORMS
# Not reached, on purpose: k_blur_resize_h_direct for 1- and 2-byte pixels.  Four staged rows pass 48 KB only from 1 / scale > 187
# (u8) or > 93 (uint16), i.e. from frames of 6000 or 3000 pixels a side whose coarsest layer is 32 x 32 behind a Gaussian of several
# hundred taps; the float32 instantiation of the same template runs at 1600 x 1600.
UNTESTED["blur_form"] = {"u8:two-pass/direct/ksn", "u16:two-pass/direct/ksn"}

@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    pyr_scale: float = 0.4
    levels: int = 1
    winsize: int = 12
    poly_n: int = 8
    poly_sigma: float = 1.2
    expects: frozenset = field(default_factory=frozenset)     # forms this case is here to reach
    depths: tuple = tuple(DEPTHS)                             # BLUR_CASES: the frame depths the case runs at

    def fb(self):
        from mavflow import _lib
        p = _lib.fb_defaults(levels=self.levels)
        p.pyr_scale, p.winsize, p.poly_n, p.poly_sigma = self.pyr_scale, self.winsize, self.poly_n, self.poly_sigma
        return p

    def oracle_params(self):
        from oracle import fb_oracle
        return fb_oracle.Params(self.pyr_scale, self.levels, self.winsize, 10, self.poly_n, self.poly_sigma, 0)


def _f(*names):
    return frozenset(names)


CASES = [
    Case("640x480", 640, 480, expects=_f("fast<6>", "polyexp<8>", "blur3_u8", "general", "mode1", "fused")),
    Case("333x227_n7_w13", 333, 227, winsize=13, poly_n=7, poly_sigma=1.5, expects=_f("fast<6,false>", "polyexp<7>", "two-pass")),
    Case("1000x562_n5_w9", 1000, 562, winsize=9, poly_n=5, poly_sigma=1.1, expects=_f("generic<0>", "polyexp<5>")),
    Case("58x174_n6_w5", 58, 174, winsize=5, poly_n=6, poly_sigma=1.3, expects=_f("generic<0>", "polyexp<0>", "copy", "mode0")),
    Case("1920x1080_l3", 1920, 1080, levels=3, expects=_f("fast<6>", "fast<6,false>")),
    Case("3840x2160_l5", 3840, 2160, levels=5, expects=_f("fast<6>", "fast<6,false>", "two-pass")),
    Case("640x480_s05_l2_w31", 640, 480, pyr_scale=0.5, levels=2, winsize=31, expects=_f("generic<0>+lds>64K", "fast")),
    Case("300x240_s033", 300, 240, pyr_scale=1 / 3, levels=1, expects=_f("fast+remainder")),
    # frames smaller than the expansion halo (poly_n) and the sweep window, one layer
    Case("16x12_n3_w15", 16, 12, levels=0, winsize=15, poly_n=3, poly_sigma=0.9, expects=_f("generic<0>", "polyexp<0>", "blur3_u8")),
    Case("37x5_w31", 37, 5, levels=0, winsize=31, expects=_f("generic<0>+lds>64K", "two-pass")),
    Case("8x2", 8, 2, levels=0, expects=_f("fast<6>", "blur3_u8")),
    Case("3x7_w13", 3, 7, levels=0, winsize=13, poly_n=7, poly_sigma=1.5, expects=_f("fast<6,false>")),
    Case("1x1", 1, 1, levels=0, expects=_f("fast<6,false>", "two-pass", "copy")),
]
CASE_IDS = [c.name for c in CASES]

# Layer images alone (tests/test_gpu_blur_forms.py, tools/layer_bits.py): the smallest frames that reach each form of BLUR_FORMS.  A
# layer of 32 x 32 is one partial 64-wide tile and two (64 x 16) or four (64 x 8) tile rows.  Every fused layer also runs forced to
# the two-pass form (two-pass/quad, two-pass/px).
BLUR_CASES = [
    Case("80x80_l0", 80, 80, levels=0, expects=_f("u8:3x3", "u16:3x3", "f32:3x3")),
    Case("80x80_s04", 80, 80, expects=_f(*(f"{d}:{f}" for d in DEPTHS for f in ("fused/fast5/th16", "two-pass/quad")))),
    Case("81x80_s04", 81, 80, expects=_f(*(f"{d}:{f}" for d in DEPTHS for f in ("fused/generic/px/ks5", "two-pass/px")))),
    Case("80x80_s05", 80, 80, pyr_scale=0.5, expects=_f(*(f"{d}:fused/generic/quad/ks0" for d in DEPTHS))),
    Case("81x80_s05", 81, 80, pyr_scale=0.5, expects=_f(*(f"{d}:fused/generic/px/ks0" for d in DEPTHS))),
    # 13 taps at 1 / scale = 6.25 on layer 2: the 64 x 16 region is past 64 KB for u8, 64 x 8 fits; the wide depths go two-pass
    Case("200x200_s04_l2", 200, 200, levels=2, expects=_f("u8:fused/fast13/th8", "u16:two-pass/quad", "f32:two-pass/quad")),
    Case("202x200_s04_l2", 202, 200, levels=2, expects=_f("u8:fused/generic/unstaged/ksn", "u16:two-pass/px", "f32:two-pass/px")),
    # 13 taps at 1 / scale = 5.6: 64 740 of the 65 536 bytes
    Case("200x200_s0178", 200, 200, pyr_scale=0.178, expects=_f("u8:fused/fast13/th16")),
    Case("202x200_s0178", 202, 200, pyr_scale=0.178, expects=_f("u8:fused/generic/px/ks13")),
    # 123 taps at 1 / scale = 50: four staged rows of float pixels are past 48 KB (u8 and uint16 rows of this shape stay staged)
    Case("1600x1600_s002_f32", 1600, 1600, pyr_scale=0.02, expects=_f("f32:two-pass/direct/ksn"), depths=("f32",)),
    Case("333x227", 333, 227, expects=_f(*(f"{d}:{f}" for d in DEPTHS for f in ("fused/generic/px/ks5", "two-pass/px")))),
]
BLUR_CASE_IDS = [c.name for c in BLUR_CASES]


def blur_case_forms(c: Case):
    """{(depth:form, layer, forced two-pass)} of a case of BLUR_CASES: every layer as dispatched and, where that is a fused form, forced"""
    out = set()
    for d in c.depths:
        for k, layer in enumerate(pyramid(c.W, c.H, c.pyr_scale, c.levels)):
            form = blur_form(c.W, c.H, layer, d)
            out.add((f"{d}:{form}", k, False))
            if form.startswith("fused"):
                out.add((f"{d}:{blur_form(c.W, c.H, layer, d, True)}", k, True))
    return out


def blur_frames(c: Case, depth: str):
    """Two frames of a depth: texture and uniform noise.  u8: images(c); the wide depths carry values no u8 frame holds (16-bit texture,
    fractional floats on the 0 .. 255 scale), as tests/test_gpu_depth.py's stage frames do."""
    if depth == "u8":
        return images(c)
    import depth_ref
    rng = np.random.default_rng(11)
    img16 = depth_ref.pair16(c.W, c.H)[0]
    if depth == "u16":
        return [img16, rng.integers(0, 65536, (c.H, c.W)).astype(np.uint16)]
    return [(img16.astype(np.float64) / 257.0).astype(np.float32), rng.random((c.H, c.W), np.float32) * 255]
# the frames at which the float64 restatement is evaluated on every layer (numpy float64 at 4K is minutes of CPU): the 4K frame only
# on its coarser layers (1536 x 864 down)
REF64_MAX_PIXELS = 1920 * 1080


def images(c: Case):
    """Two frames: the textured synthetic pair's first frame and uniform noise (every gradient at once)."""
    from mavflow import synth
    rng = np.random.default_rng(11)
    return [synth.make_pair(c.W, c.H, 3)[0], rng.integers(0, 256, (c.H, c.W), dtype=np.uint8)]


def edge_targets(n: int):
    """Displaced coordinates at the edges of the inside test along an axis of n pixels: exactly 0, 0 reached through -0.0, the
    float just below 0 (-2^-20), exactly n - 1 (outside: the 2 x 2 neighbourhood leaves the image) and the largest float below
    n - 1 (inside, weight ~1 on the last column).  (n - 1 - 2^-20 itself is no float32 once n > 16: its float below n - 1 is.)"""
    below = float(np.nextafter(np.float32(n - 1), np.float32(-1)))
    return [0.0, -0.0, -2.0 ** -20, float(n - 1), below]


def smooth_flow(w: int, h: int, seed: int = 3) -> np.ndarray:
    """smooth plus noise, as tests/test_gpu_flow.py _stage_inputs builds it: a flow some way into an iteration"""
    from mavflow import synth
    rng = np.random.default_rng(seed)
    flow = (synth.true_flow(w, h, k=0.01) + rng.normal(0, 0.2, (h, w, 2))).astype(np.float32)
    flow[0, 0] = (-5.0, -7.0)
    flow[h - 1, w - 1] = (9.0, 3.0)
    return flow


def crafted_flow(w: int, h: int, seed: int = 3) -> np.ndarray:
    """smooth_flow with the pixels of every border (5 deep, the weighted frame) and a few inner rows / columns displaced so that
    x + dx (and y + dy) land exactly on edge_targets: the inside test and the border table at their edges, at once."""
    flow = smooth_flow(w, h, seed)
    xs = sorted(set(list(range(min(5, w))) + list(range(max(0, w - 5), w)) + [w // 2]))
    ys = sorted(set(list(range(min(5, h))) + list(range(max(0, h - 5), h)) + [h // 2]))
    for j, x in enumerate(xs):                                   # columns at the left / right border: dx aimed at a target
        flow[:, x, 0] = _aim(x, edge_targets(w), j)
    for i, y in enumerate(ys):                                   # rows at the top / bottom border: dy aimed at a target
        flow[y, :, 1] = _aim(y, edge_targets(h), i + 2)
    return flow


def _aim(p: int, targets, start: int) -> np.float32:
    """The float32 displacement d with float32(p) + d == target for the first target, from index `start` on (cyclically), that p
    can reach exactly (-2^-20 from p >= 16 cannot: the sum would need more than 24 bits); -0.0 is reached as p + (-p), or as
    0 + (-0.0) from p = 0."""
    for i in range(len(targets)):
        t = np.float32(targets[(start + i) % len(targets)])
        d = np.float32(t) - np.float32(p)
        if np.float32(p) + d == t and float(d) == float(t) - p:
            return d
    raise AssertionError((p, targets))

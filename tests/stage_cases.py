"""TEST INFRASTRUCTURE -- the frames, Farneback parameters and inputs at which every stage of the flow path is held to the oracle and
to the float64 restatement (tests/test_gpu_stages.py, tests/test_stage_ref64_cpu.py), and the kernel form each stage takes there.

The library dispatches a stage to one of several kernels on the layer's width, the parameters and the area ratio of the initial
flow.  Each case below names the forms it is there to reach; tests/test_gpu_stages.py::test_every_kernel_form_is_reached derives the
forms from the same predicates the dispatch uses (kernels_flow.hip launch_blur_iter / launch_polyexp / launch_blur_resize,
kernels_window.hip launch_area_resize_flow) and fails when a form of FORMS is no longer reached.

The sibling tables: tests/detect_cases.py (detection path, kernels_detect.hip), tests/sparse_cases.py (sparse path, kernels_lk.hip)
and tests/window_cases.py (window search, kernels_window.hip).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from initial_flow_ref import area_ratio

# every kernel form of the stages, as the dispatch names them
FORMS = {
    "sweep": {"fast<6>", "fast<6,false>", "generic<0>", "generic<0>+lds>64K"},
    "polyexp": {"polyexp<8>", "polyexp<7>", "polyexp<5>", "polyexp<0>"},
    "initial_m": {"mode0", "mode1", "mode2"},
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

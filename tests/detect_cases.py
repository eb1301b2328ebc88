"""TEST INFRASTRUCTURE -- the frames, batches and inputs at which every kernel instance of the detection path (csrc/kernels_detect.hip)
is held to the numpy oracle (oracle/foe_oracle.py, tests/render_ref.py) by tests/test_gpu_detect_forms.py, and the instance each case
takes there.  The counterpart of tests/stage_cases.py for the flow path.

The launchers dispatch on the frame's width, the batch, the presence of per-pair parameters, the outputs requested and two options.
Every predicate below restates one such decision and cites the line it mirrors; tests/test_detect_cases_cpu.py derives the forms each
case reaches from these predicates and fails when a form of FORMS is no longer reached, when a noise field stops separating the masks,
when a pixel sits inside the band in which device and oracle may differ (the GPU tests compare masks with array_equal: nothing is
excused), or when a planted rectangle is not the oracle's box.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import foe_oracle as fo
from test_frame0 import ARCCOS_ULPS, thresholds32, ulps32
from test_gpu_detect import PHI_ATOL

# every instance of the detection kernels, as the dispatch decides them
FORMS = {
    "phi.flow": {"f32", "f64"},                        # mav_stage_phi_mask / mav_detect / mav_phi_mask_f32 | mav_phi_mask
    "phi.vec": {"vec4", "vec1"},
    "phi.rot": {"rot", "norot"},                       # a DerotParams block is passed | none
    "phi.pair": {"plain", "derotate", "frame0"},
    "phi.path": {"screen", "exact"},
    "phi.tiles": {"gx1", "gx>1"},
    "phi.yloop": {"yloop1", "yloop>1:option", "yloop>1:auto"},
    "phi.sky": {"sky", "nosky"},
    "phi.masks": {"both", "fixed-only", "dyn-only"},   # a NULL mask output
    "foe.chunks": {"chunks1", "chunks>1"},
    "foe.flow": {"f32", "f64"},
    "foe.gate": {"gate64", "gate32"},                  # the |flow2| gate of a frame-0 pair runs in float32
    "ransac": {"wg-1", "wg", "wg+1", "wave-1", "wave", "wave+1", "bound"},
    "render": {"tail", "straddle"},
    "window_max": {"none", "one", "nwx<=256", "nwx>256"},
    "bbox": {"gx1", "gx>1"},
    "batch": {"batch<=64", "batch>64"},
}
# Not reached, on purpose.  Each needs a device pointer that is not 4-byte aligned; every buffer the host entry points stage is
# aligned, only a caller's own misaligned device pointer could select these, and tests do not hand kernels misaligned pointers:
#   k_phi_mask<*, 1, *> at W % 4 == 0 (launch_phi_mask_t: `vec` also asks the sky and mask pointers to be dword aligned)
#   k_render's byte-by-byte store of a whole group of four pixels (`((uintptr_t)o & 3) == 0` fails)
UNTESTED = {"phi.vec": {"vec1:misaligned"}, "render": {"bytewise:misaligned"}}


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------
def phi_vec(W: int) -> int:
    """launch_phi_mask_t: `vec = W % 4 == 0 && ...aligned`; staging blocks are aligned."""
    return 4 if W % 4 == 0 else 1


def phi_gx(W: int) -> int:
    """launch_phi_mask_t: `gx = vec ? (W / 4 + 63) / 64 : (W + 63) / 64`."""
    return (W // 4 + 63) // 64 if phi_vec(W) == 4 else (W + 63) // 64


def phi_nby(H: int) -> int:
    """launch_phi_mask_t: `nby = (H + 15) / 16`."""
    return (H + 15) // 16


def phi_yloop(W: int, H: int, B: int, option: int = 0) -> int:
    """launch_phi_mask_t: option "phi_yloop" when >= 1, else `want = 4096 / (gx * B); yloop = want > 0 ? ceil(nby / want) : nby`."""
    if option >= 1:
        return option
    nby = phi_nby(H)
    want = 4096 // max(phi_gx(W) * B, 1)
    return (nby + want - 1) // want if want > 0 else nby


def phi_steps(W: int, H: int, B: int, option: int = 0) -> int:
    """Steps of k_phi_mask's row-block loop for the workgroup with blockIdx.y = 0: grid.y = ceil(nby / yloop), the loop strides by it."""
    nby = phi_nby(H)
    gy = (nby + phi_yloop(W, H, B, option) - 1) // phi_yloop(W, H, B, option)
    return (nby + gy - 1) // gy


def foe_chunks(n_pairs: int) -> int:
    """k_foe_candidates: `for (int i0 = 0; i0 < N; i0 += 1024)`."""
    return (n_pairs + 1023) // 1024


def ransac_forms(count: int) -> set:
    """k_ransac: a workgroup scores 16 candidates, a wave 4 (launch_ransac_only: grid (count + 15) / 16); mav_ransac: count <= 4096."""
    out = set()
    for name, q in (("wg", 16), ("wave", 4)):
        if count % q == q - 1:
            out.add(name + "-1")
        if count % q == 0:
            out.add(name)
        if count % q == 1:
            out.add(name + "+1")
    if count == 4096:
        out.add("bound")
    return out


def render_forms(W: int, H: int, B: int) -> set:
    """k_render: four consecutive pixels of the flattened (B, H, W) index per thread; `if (p >= total) continue` is the tail, a thread
    whose pixels have different `p / npx` straddles two pairs."""
    out = set()
    if (B * W * H) % 4:
        out.add("tail")
    if (W * H) % 4 and B > 1:
        out.add("straddle")
    return out


def window_form(W: int, H: int) -> str:
    """launch_window_max: nwx = (W - 64) / 16 + 1 windows per row (0 below 64 px); k_window_max: `for (wx = tid; wx < nwx; wx += 256)`."""
    nwx = (W - 64) // 16 + 1 if W >= 64 else 0
    nwy = (H - 64) // 16 + 1 if H >= 64 else 0
    if nwx == 0 or nwy == 0:
        return "none"
    if nwx * nwy == 1:
        return "one"
    return "nwx>256" if nwx > 256 else "nwx<=256"


def bbox_form(W: int) -> str:
    """launch_bbox_u8: grid.x = (W + 255) / 256 column tiles of k_u8_extents."""
    return "gx>1" if (W + 255) // 256 > 1 else "gx1"


def batch_form(B: int) -> str:
    """launch_box_init / launch_box_finalize / launch_window_max: grids of (B + 63) / 64 workgroups of 64 threads."""
    return "batch>64" if (B + 63) // 64 > 1 else "batch<=64"


# ---- phi / mask / box -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PhiCall:
    """One way into k_phi_mask: the entry point, the flow type, whether rates are passed and which pairs are frame-0 pairs."""
    name: str
    entry: str                 # "stage" (mav_stage_phi_mask), "host" (mav_phi_mask / mav_phi_mask_f32), "detect" (mav_detect)
    flow: str                  # "f32" | "f64"
    rates: bool = False
    frame0: tuple = ()

    def mode(self, b: int) -> str:
        if self.frame0 and self.frame0[b % len(self.frame0)]:
            return "frame0"
        return "derotate" if self.rates else "plain"

    def rot(self) -> bool:
        """detect_dev passes `derot` whenever upload_derot saw rates or frame-0 flags; mav_phi_mask_f32 passes frame0_params."""
        return self.rates or bool(self.frame0)


PHI_CALLS = [
    PhiCall("stage_plain", "stage", "f32"),
    PhiCall("stage_derot", "stage", "f32", rates=True),
    PhiCall("host_f64", "host", "f64"),
    PhiCall("host_f32", "host", "f32", frame0=(1,)),
    PhiCall("detect_mixed", "detect", "f32", rates=True, frame0=(1, 0, 0)),
]
PHI_B = 3
OMEGA = np.array([[0.31, -0.17, 0.23], [-0.42, 0.28, -0.11], [0.13, 0.36, -0.29]])
DT = np.array([1 / 30.0, 1 / 25.0, 0.05])
DETECT_PAIRS = 64              # line pairs of the mav_detect calls of the phi cases
DETECT_GATE = 0.5              # their |flow2| gate: the noise fields are a pixel or so strong, the default 2.5 would leave no candidate


def phi_forms(W: int, H: int, B: int, call: PhiCall, want_phi: bool, sky: bool, yloop_option: int = 0, screen_option: int = 1) -> set:
    out = {("phi.flow", call.flow), ("phi.vec", f"vec{phi_vec(W)}"), ("phi.rot", "rot" if call.rot() else "norot"),
           ("phi.tiles", "gx>1" if phi_gx(W) > 1 else "gx1"), ("phi.sky", "sky" if sky else "nosky"), ("phi.masks", "both"),
           ("batch", batch_form(B))}
    steps = phi_steps(W, H, B, yloop_option)
    out.add(("phi.yloop", "yloop1" if steps == 1 else ("yloop>1:option" if yloop_option >= 1 else "yloop>1:auto")))
    for b in range(B):
        m = call.mode(b)
        out.add(("phi.pair", m))
        # k_phi_mask: `screen = scr.enabled && !f32_pair`; phi_screen(): enabled only when neither phi nor max(phi) is requested
        out.add(("phi.path", "screen" if (not want_phi and screen_option and m != "frame0") else "exact"))
    return out


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    B: int = PHI_B
    expects: frozenset = field(default_factory=frozenset)     # forms this case is here to reach
    yloop_options: tuple = ()                                  # values of option "phi_yloop" a second context runs the case with


def _f(*names):
    return frozenset(names)


PHI_CASES = [
    Case("1x1", 1, 1, expects=_f("vec1", "gx1", "yloop1")),
    Case("3x5", 3, 5, expects=_f("vec1")),
    Case("5x3", 5, 3, expects=_f("vec1")),                                        # fewer rows than a wave's four
    Case("7x1", 7, 1, expects=_f("vec1")),
    Case("63x17", 63, 17, expects=_f("vec1", "gx1")),                             # two row blocks
    Case("66x33", 66, 33, expects=_f("vec1", "gx>1", "yloop>1:option"), yloop_options=(1, 2, 8)),      # three row blocks
    Case("257x19", 257, 19, expects=_f("vec1", "gx>1")),                          # five column tiles
    Case("260x15", 260, 15, expects=_f("vec4", "gx>1")),                          # H < 16
    Case("516x37", 516, 37, expects=_f("vec4", "gx>1", "yloop>1:option"), yloop_options=(1, 2, 8)),    # three tiles x three row blocks
]
PHI_IDS = [c.name for c in PHI_CASES]
# 8 x 32 x 3000 pairs through mav_detect: gx * B * nby = 6000 > 4096, the launcher gives every workgroup two row blocks
AUTO_CASE = Case("8x32x3000", 8, 32, B=3000, expects=_f("vec4", "yloop>1:auto", "batch>64"))
AUTO_PAIRS = 8


def case_forms(c: Case) -> set:
    out = set()
    if c is AUTO_CASE:
        call = PhiCall("detect_auto", "detect", "f32", rates=True, frame0=(1, 0, 0, 0, 0, 0, 0))
        return phi_forms(c.W, c.H, c.B, call, False, True) | {("foe.chunks", "chunks1"), ("foe.flow", "f32"), ("bbox", bbox_form(c.W))}
    for call in PHI_CALLS:
        for want_phi in (False, True):
            for sky in (False, True):
                out |= phi_forms(c.W, c.H, c.B, call, want_phi, sky)
    for y in c.yloop_options:
        out |= phi_forms(c.W, c.H, c.B, PHI_CALLS[0], False, True, yloop_option=y)
    out |= phi_forms(c.W, c.H, c.B, PHI_CALLS[0], False, True, screen_option=0)
    return out


def foes(W: int, H: int) -> np.ndarray:
    """in the middle, far outside the frame, on a pixel centre"""
    return np.array([[0.55 * W + 0.3, 0.45 * H - 0.2], [-3.3 * W - 1.7, H + 250.5], [float(W // 2), float(H // 2)]])


NOISE_SEED = 44              # 40 puts one float32 pixel of 516x37 on its dynamic threshold to the last bit


@functools.lru_cache(maxsize=None)
def noise_fields(W: int, H: int) -> np.ndarray:
    """(3, H, W, 2) float32: a different radial-plus-noise field per pair"""
    from mavflow import synth
    out = np.stack([synth.synthetic_flow(W, H, seed=NOISE_SEED + b, noise=0.5) for b in range(PHI_B)])
    out.setflags(write=False)
    return out


def sky_masks(W: int, H: int, B: int = PHI_B) -> np.ndarray:
    """(B, H, W) bool, a different one per pair: the top rows, a lattice, the right-hand columns"""
    sky = np.zeros((B, H, W), bool)
    for b in range(B):
        k = b % 3
        if k == 0:
            sky[b, : H // 4] = True
        elif k == 1:
            sky[b, ::3, 1::2] = True
        else:
            sky[b, :, W - W // 5:] = True
    return sky


def detect_samples(W: int, H: int, B: int, n_pairs: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    smp = np.zeros((B, 2 * n_pairs, 2), np.uint32)
    smp[..., 0] = rng.integers(0, H, (B, 2 * n_pairs))
    smp[..., 1] = rng.integers(0, W, (B, 2 * n_pairs))
    return smp


def seen_field(flow32: np.ndarray, mode: str, omega=None, dt=None) -> np.ndarray:
    """The field the kernel's arithmetic sees: the float32 field itself for a frame-0 pair (detector.py:80-81), the oracle's
    derotation of it, or its exact promotion to double."""
    if mode == "frame0":
        return flow32
    if mode == "derotate":
        return fo.derotate(flow32, omega, dt)
    return flow32.astype(np.float64)


def reference(seen: np.ndarray, foe, sky=None) -> dict:
    """phi, both masks and the box of one pair from the oracle alone"""
    foe = (float(foe[0]), float(foe[1]))
    with np.errstate(all="ignore"):
        phi, mag = fo.get_phi(seen, foe), fo.get_magnitude(seen)
        fixed, total = fo.threshold_masks(phi, mag, sky)
    return dict(phi=phi, mag=mag, fixed=fixed, total=total, box=fo.simple_bounding_box(fixed), foe=foe)


def band_pixels(ref: dict) -> int:
    """Pixels whose phi lies inside the band in which device and oracle may decide differently: ARCCOS_ULPS float32 ulps of the deciding
    threshold for a float32 (frame-0) pair (tests/test_frame0.py assert_masks), PHI_ATOL for a float64 pair (tests/test_gpu_detect.py)."""
    phi, mag = ref["phi"], ref["mag"]
    with np.errstate(all="ignore"):
        if phi.dtype == np.float32:
            thr = thresholds32(mag)
            near_f = ulps32(phi, np.full_like(phi, 15.0)) <= ARCCOS_ULPS
            near_d = np.isfinite(thr) & (ulps32(phi, np.where(np.isfinite(thr), thr, 0).astype(np.float32)) <= ARCCOS_ULPS)
        else:
            near_f = np.abs(phi - 15.0) <= PHI_ATOL
            near_d = np.abs(phi - (0.25 + (0.5 + 8 / mag))) <= PHI_ATOL
    return int(near_f.sum() + near_d.sum())


def phi_close(got: np.ndarray, ref_phi: np.ndarray) -> bool:
    """phi (or max(phi)) within the project's own bars: PHI_ATOL for float64 pairs, ARCCOS_ULPS float32 ulps for float32 pairs"""
    if ref_phi.dtype == np.float32:
        g = np.asarray(got)
        return bool(np.array_equal(g.astype(np.float32), g) and ulps32(g, ref_phi).max() <= ARCCOS_ULPS)
    return bool(np.abs(np.asarray(got, np.float64) - ref_phi).max() <= PHI_ATOL)


def noise_reference(W: int, H: int, call: PhiCall, with_sky: bool) -> list:
    """the oracle's answer for each of the three noise pairs under `call` (mav_detect: the FoE is the oracle's own RANSAC result)"""
    fl, sky, fe = noise_fields(W, H), sky_masks(W, H), foes(W, H)
    smp = detect_samples(W, H, PHI_B, DETECT_PAIRS)
    out = []
    for b in range(PHI_B):
        seen = seen_field(fl[b], call.mode(b), OMEGA[b], DT[b])
        foe = fe[b]
        if call.entry == "detect":
            with np.errstate(all="ignore"):
                foe = fo.get_foe_dense(seen, smp[b], DETECT_GATE, 30.0)
        out.append(reference(seen, foe, sky[b] if with_sky else None))
    return out


# ---- planted fields: exactly radial flow (phi ~ 0, empty fixed mask) with one rectangle turned by 90 degrees ---------------------------
def _spans(n: int) -> list:
    """Inclusive spans on an axis of n pixels whose ends fall on, and on either side of: 63|64 (a wave's lanes at one pixel per lane),
    255|256 (a new column tile at four pixels per lane), 15|16 (a new row block), a multiple of 4 plus 1, 2, 3 (the nibble-to-extent
    code, __ffs / __clz of f4) and the last pixel."""
    out = []
    for k in (16, 64, 256):
        out += [(k - 5, k - 1), (k - 6, k), (k - 1, k + 6), (k, k + 5)]
    base = 4 * ((n // 2) // 4)
    out += [(base + 1, base + 1), (base + 2, base + 7), (base + 3, base + 5), (base + 5, base + 6), (1, 1), (2, 3), (1, 2), (3, 6)]
    out += [(n - 1, n - 1), (n - 3, n - 1), (0, 0), (0, n - 1), (n - 2, n - 2)]
    seen, keep = set(), []
    for a, b in out:
        if 0 <= a <= b <= n - 1 and (a, b) not in seen:
            seen.add((a, b))
            keep.append((a, b))
    return keep


@dataclass(frozen=True)
class Plant:
    rect: tuple | None         # (x0, y0, x1, y1) inclusive; None: nothing planted (box all -1)
    sky_all: bool = False      # the sky mask covers the whole frame

    def box(self) -> tuple:
        return (-1, -1, -1, -1) if self.rect is None or self.sky_all else self.rect


def plants(W: int, H: int) -> list:
    xs, ys = _spans(W), _spans(H)
    n = max(len(xs), len(ys))
    out = [Plant((xs[i % len(xs)][0], ys[i % len(ys)][0], xs[i % len(xs)][1], ys[i % len(ys)][1])) for i in range(n)]
    out += [Plant(None), Plant(out[0].rect, sky_all=True), Plant((W - 1, H - 1, W - 1, H - 1))]
    return out


def plant_foes(W: int, H: int, B: int) -> np.ndarray:
    """never on a pixel centre (phi would be 90 degrees there): in the middle, far outside, off centre"""
    three = np.array([[0.55 * W + 0.3, 0.45 * H - 0.2], [-3.3 * W - 1.7, H + 250.5], [0.31 * W - 0.4, 0.62 * H + 0.35]])
    return three[np.arange(B) % 3]


@functools.lru_cache(maxsize=None)
def planted_fields(W: int, H: int):
    """((B, H, W, 2) float32 flows, (B, 2) FoEs, (B, H, W) bool sky masks, [expected box]) for B = len(plants(W, H)) pairs"""
    pl = plants(W, H)
    B = len(pl)
    fe = plant_foes(W, H, B)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.empty((B, H, W, 2), np.float32)
    sky = np.zeros((B, H, W), bool)
    for b, p in enumerate(pl):
        dx, dy = xs - fe[b, 0], ys - fe[b, 1]
        r = np.hypot(dx, dy)
        u, v = 2.0 * dx / r, 2.0 * dy / r
        if p.rect is not None:
            x0, y0, x1, y1 = p.rect
            inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
            u, v = np.where(inside, -3.0 * dy / r, u), np.where(inside, 3.0 * dx / r, v)
        flow[b] = np.stack([u, v], axis=-1)
        sky[b] = p.sky_all
    flow.setflags(write=False)
    return flow, fe, sky, [p.box() for p in pl]


# calls the planted fields go through: no true derotation (it would bend the radial field), but the ROT instance with zero rates
PLANT_CALLS = [PHI_CALLS[0], PhiCall("stage_zero_rates", "stage", "f32", rates=True), PHI_CALLS[2], PHI_CALLS[3]]


# ---- the large batch on tiny frames ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def auto_inputs():
    """8 x 32 x 3000: pair b's field is a uniform flow of direction 0.37 b and strength 1 + (b mod 5) plus unit noise; every seventh pair
    is a frame-0 pair; the sky mask leaves a window of its own to each pair."""
    c = AUTO_CASE
    rng = np.random.default_rng(77)
    b = np.arange(c.B, dtype=np.float64)[:, None, None]
    flow = rng.normal(0.0, 1.0, (c.B, c.H, c.W, 2))
    flow[..., 0] += (1.0 + b % 5) * np.cos(0.37 * b)
    flow[..., 1] += (1.0 + b % 5) * np.sin(0.37 * b)
    flow = flow.astype(np.float32)
    omega = rng.normal(0.0, 0.3, (c.B, 3))
    dt = rng.uniform(0.02, 0.05, c.B)
    frame0 = (np.arange(c.B) % 7 == 0).astype(np.uint8)
    # sky: everything outside a window that depends on b (so that the box does), and a fifth of the pixels inside it
    bb = np.arange(c.B)[:, None, None]
    ys, xs = np.mgrid[0:c.H, 0:c.W][:, None]
    sky = (ys < bb % 13) | (ys > c.H - 1 - bb % 11) | (xs < bb % 3) | (xs > c.W - 1 - bb % 2) | (rng.random((c.B, c.H, c.W)) < 0.2)
    smp = detect_samples(c.W, c.H, c.B, AUTO_PAIRS, seed=5)
    return flow, omega, dt, frame0, sky, smp


@functools.lru_cache(maxsize=None)
def auto_reference() -> list:
    flow, omega, dt, frame0, sky, smp = auto_inputs()
    out = []
    for b in range(AUTO_CASE.B):
        seen = seen_field(flow[b], "frame0" if frame0[b] else "derotate", omega[b], dt[b])
        with np.errstate(all="ignore"):
            foe = fo.get_foe_dense(seen, smp[b], DETECT_GATE, 30.0)
        out.append(reference(seen, foe, sky[b]))
    return out


# ---- FoE: several chunks of 1024 line pairs ----------------------------------------------------------------------------------------------
FOE_W, FOE_H = 66, 33
FOE_COUNTS = (1024, 1025, 2047, 2500, 4096)
# kind -> (|flow2| gate, RANSAC radius)
FOE_KINDS = {"integer": (1.5, 1.0), "normal": (2.5, 30.0), "synthetic": (0.5, 5.0)}
FOE_SEED = 0


@functools.lru_cache(maxsize=None)
def foe_inputs(kind: str, n_pairs: int):
    """(float32 flow (H, W, 2), samples (2 n, 2) uint32) -- integer-valued flows in [-3, 3] (exactly parallel lines, exactly coincident
    intersections: ties), N(0, 1.2) flows, and the radial-plus-noise field of the phi cases"""
    from mavflow import synth
    rng = np.random.default_rng([FOE_SEED, n_pairs, sorted(FOE_KINDS).index(kind)])
    if kind == "integer":
        flow = rng.integers(-3, 4, (FOE_H, FOE_W, 2)).astype(np.float32)
    elif kind == "normal":
        flow = rng.normal(0.0, 1.2, (FOE_H, FOE_W, 2)).astype(np.float32)
    else:
        flow = synth.synthetic_flow(FOE_W, FOE_H, seed=n_pairs, noise=0.5)
    smp = np.zeros((2 * n_pairs, 2), np.uint32)
    smp[:, 0] = rng.integers(0, FOE_H, 2 * n_pairs)
    smp[:, 1] = rng.integers(0, FOE_W, 2 * n_pairs)
    flow.setflags(write=False)
    return flow, smp


def foe_trace(flow: np.ndarray, samples: np.ndarray, gate: float, radius: float) -> dict:
    """fo.get_foe_dense, opened up: the survivor count, the winner's original line-pair index and how many survivors share the best score"""
    with np.errstate(all="ignore"):
        inter = fo.line_intersections(flow, samples, gate)
        alive = np.flatnonzero(inter[:, 0] != 0.0)
        est = inter[alive]
        foe = fo.ransac(est, radius)
        if est.shape[0] == 0:
            return dict(foe=foe, survivors=0, winner=-1, ties=0)
        dx = est[:, None, 0] - est[None, :, 0]
        dy = est[:, None, 1] - est[None, :, 1]
        score = (np.sqrt(dx * dx + dy * dy) < radius).sum(axis=1) - 1
    best = int(np.argmax(score))
    won = score[best] > 0
    return dict(foe=foe, survivors=int(est.shape[0]), winner=int(alive[best]) if won else -1, ties=int((score == score[best]).sum()) if won else 0)


# ---- RANSAC on caller-supplied estimates ---------------------------------------------------------------------------------------------------
RANSAC_COUNTS = (15, 16, 17, 63, 64, 65, 1025, 4095, 4096)
RANSAC_RADIUS = 30.0
STAR_LAST, STAR_FIRST = (1.5, -2.5), (-5e3, 0.5)   # centres of the planted stars; (0, 0) is what "no winner" returns


def _star(cx: float, cy: float, r: float = RANSAC_RADIUS) -> np.ndarray:
    """five points on a circle of radius 0.9 r: each within r of the centre, more than r (1.058 r) from its neighbours"""
    a = 2 * np.pi * np.arange(5) / 5
    return np.stack([cx + 0.9 * r * np.cos(a), cy + 0.9 * r * np.sin(a)], axis=1)


def ransac_set(count: int, kind: str) -> np.ndarray:
    """(count, 2) estimates.  "random": a cluster in uniform clutter.  "last": isolated points and one star whose centre is the LAST
    estimate (score 5, every other at most 1).  "tie": two such stars, the first centre at index 3 (workgroup 0), the second centre
    last (another workgroup once count > 16): equal best scores, the earlier must win."""
    rng = np.random.default_rng([count, ("random", "last", "tie").index(kind)])
    if kind == "random":
        k = (2 * count) // 3
        return np.concatenate([rng.normal(200, 10, (k, 2)), rng.uniform(-500, 900, (count - k, 2))])
    # isolated: a lattice 100 apart, far from the stars
    idx = np.arange(count)
    est = np.stack([1e4 + 100.0 * (idx % 64), 1e4 + 100.0 * (idx // 64)], axis=1)
    est[count - 6:count - 1] = _star(*STAR_LAST)
    est[count - 1] = STAR_LAST
    if kind == "tie":
        est[4:9] = _star(*STAR_FIRST)
        est[3] = STAR_FIRST
    return est


# ---- the remaining kernels -----------------------------------------------------------------------------------------------------------------
RENDER_SHAPES = ((1, 1), (3, 5), (7, 1), (63, 17), (66, 33))
RENDER_BATCHES = (1, 3)
WINDOW_SHAPES = ((64, 64), (80, 63), (63, 80), (96, 80), (4176, 64))
WINDOW_BATCH = (80, 64, 70)                      # W, H, B
BBOX_SHAPES = ((1, 1), (257, 5), (513, 3))
DEROT_SHAPES = ((1, 1), (66, 33), (257, 19))
TPR_SHAPES = ((37, 29), (64, 48))
TPR_VALUES = (2, 128, 65535)


def other_forms() -> set:
    """the forms the cases outside PHI_CASES / AUTO_CASE reach"""
    out = set()
    for n in FOE_COUNTS:
        out |= {("foe.chunks", "chunks1" if foe_chunks(n) == 1 else "chunks>1"), ("foe.flow", "f32"), ("foe.flow", "f64"),
                ("foe.gate", "gate64"), ("foe.gate", "gate32")}            # every count runs as float64, float32 and a frame-0 pair of mav_detect
    for n in RANSAC_COUNTS:
        out |= {("ransac", f) for f in ransac_forms(n)}
    for W, H in RENDER_SHAPES:
        for B in RENDER_BATCHES:
            out |= {("render", f) for f in render_forms(W, H, B)}
    out |= {("window_max", window_form(W, H)) for W, H in WINDOW_SHAPES}
    out |= {("window_max", window_form(*WINDOW_BATCH[:2])), ("batch", batch_form(WINDOW_BATCH[2]))}
    out |= {("bbox", bbox_form(W)) for W, _ in BBOX_SHAPES}
    out |= {("phi.masks", "fixed-only"), ("phi.masks", "dyn-only")}        # test_a_null_mask_output, through ctx.lib.mav_stage_phi_mask
    return out

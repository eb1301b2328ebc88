"""TEST INFRASTRUCTURE -- the inputs at which the threshold sweep (mav_roc_sweep, csrc/kernels_detect.hip k_roc_sweep / k_roc_suffix) is
held to the existing detection path and to the numpy reference (tests/roc_ref.py): the threshold grids, the ground-truth images, the
noise fields of tests/detect_cases.py under its four non-detect calls, planted fields and one large batch of tiny frames.

The sweep takes the float32 field; `host_f64` (mav_phi_mask on the field promoted to double) sees the same numbers as the plain call.
"""
from __future__ import annotations

import functools

import numpy as np

import detect_cases as dc
from oracle import foe_oracle as fo

ANG = [0.5, 1, 2, 3.5, 5, 7.5, 10, 12.5, 15, 17.5, 20, 25, 30, 40, 50, 60, 75, 89, 91, 120, 150, 179]
MAG = [0.25, 0.5, 0.75, 1, 1.5, 2, 3]
MAG_PLANTED = MAG + [5.0]                                # the (3, 4) field's magnitude is exactly 5.0: on a threshold
MAX_ANGLES, MAX_MAGS = 64, 16                             # MAV_ROC_MAX_ANGLES / MAV_ROC_MAX_MAGS

# name -> (angles, mags).  "full" and "one" are subsets of ANG x MAG, for which tests/test_roc_ref_cpu.py keeps the band condition
# true: they are compared with the oracle.  The others are compared device against device only (their thresholds -- 0, 90, 180, the
# 64 x 16 lattice -- sit where oracle pixels may lie: zero flow gives phi = 90, anti-radial flow 180).
GRIDS = {
    "full": (ANG, MAG),
    "one": ([15.0], [1.0]),
    "max": (list(np.linspace(0.25, 179.75, MAX_ANGLES)), list(np.linspace(0.125, 4.0, MAX_MAGS))),
    "zero": ([0.0, 2.0, 15.0], [0.0, 1.0]),
    "collapse": ([10.0, 15.0, float(np.nextafter(15.0, 16.0)), 20.0], [0.5, 1.0]),      # two doubles, one float32
    "right": ([45.0, 90.0, 135.0, 180.0], [1.0, 2.0]),
}
REF_GRIDS = ("full", "one")
DEVICE_ONLY_GRIDS = ("zero", "collapse", "right")
MAX_GRID_CASE = "66x33"                                   # the 64 x 16 grid runs there only

CALLS = [c for c in dc.PHI_CALLS if c.entry != "detect"]  # plain, derotate, float64 host, frame-0
GT_VALUES = (0, 1, 127, 128, 254, 255)                    # either side of every comparison of calculate_tpr_fpr at mask value 255
LARGE = (8, 32, 70)                                       # W, H, pairs: more than 64 pairs of tiny frames
PLANTED_SHAPES = ((66, 33), (260, 15))
PLANTED = ("int345", "zero", "naninf", "antiradial", "allsky")


def lists_valid(angles, mags) -> bool:
    """the ABI's rules: 1 .. max entries, finite, >= 0, strictly increasing"""
    for v, cap in ((np.asarray(angles, np.float64), MAX_ANGLES), (np.asarray(mags, np.float64), MAX_MAGS)):
        if v.ndim != 1 or not 1 <= v.size <= cap or not np.all(np.isfinite(v)) or np.any(v < 0) or np.any(np.diff(v) <= 0):
            return False
    return True


# what the ABI refuses: name -> (angles, mags)
BAD_LISTS = {
    "unsorted": ([1.0, 3.0, 2.0], [1.0]),
    "repeated": ([1.0, 2.0], [0.5, 0.5]),
    "negative": ([-1.0, 2.0], [1.0]),
    "nan": ([1.0, float("nan")], [1.0]),
    "inf": ([1.0], [1.0, float("inf")]),
    "empty": ([], [1.0]),
    "empty_mags": ([1.0], []),
    "oversized": (list(range(MAX_ANGLES + 1)), [1.0]),
    "oversized_mags": ([1.0], list(range(MAX_MAGS + 1))),
}


@functools.lru_cache(maxsize=None)
def gt_images(W: int, H: int, B: int = dc.PHI_B) -> np.ndarray:
    """(B, H, W) u8 of GT_VALUES, a different image per pair; every value occurs where the frame has six pixels"""
    rng = np.random.default_rng(700 + 31 * W + H)
    g = np.asarray(GT_VALUES, np.uint8)[rng.integers(0, len(GT_VALUES), (B, H, W))]
    flat = g.reshape(B, -1)
    n = min(flat.shape[1], len(GT_VALUES))
    for b in range(B):
        flat[b, :n] = np.roll(GT_VALUES, b)[:n]
    g.setflags(write=False)
    return g


def sweep_kwargs(call: dc.PhiCall, B: int) -> dict:
    """Context.roc_sweep's keywords that put its pairs into the call's mode"""
    kw = {}
    if call.rates:
        kw.update(omega=dc.OMEGA[np.arange(B) % len(dc.OMEGA)], dt=dc.DT[np.arange(B) % len(dc.DT)])
    if call.frame0:
        kw["frame0"] = [call.frame0[b % len(call.frame0)] for b in range(B)]
    return kw


def oracle_fields(flow32: np.ndarray, mode: str, foe, omega=None, dt=None):
    """(phi, mag) of one pair from the oracle: float32 arrays for a frame-0 pair, float64 otherwise"""
    seen = dc.seen_field(flow32, mode, omega, dt)
    with np.errstate(all="ignore"):
        return fo.get_phi(seen, (float(foe[0]), float(foe[1]))), fo.get_magnitude(seen)


@functools.lru_cache(maxsize=None)
def planted(W: int, H: int) -> dict:
    """One batch of planted pairs (PLANTED order): flow (P, H, W, 2) float32, foe (P, 2), sky (P, H, W) bool."""
    P = len(PLANTED)
    ys, xs = np.mgrid[0:H, 0:W]
    flow = np.zeros((P, H, W, 2), np.float32)
    foe = np.tile(np.array([[0.55 * W + 0.3, 0.45 * H - 0.2]]), (P, 1))
    sky = np.zeros((P, H, W), bool)
    flow[0, ..., 0], flow[0, ..., 1] = 3.0, 4.0                                   # |flow| = 5.0 exactly, in float32 and in double
    flow[0, ::2, 1::3] = (-4.0, 3.0)
    # pair 1: zero flow -- the norm floor, arg = 0, phi = 90; no gate passes (mag = 0) ...
    flow[1, ::2, ::2] = (1e-9, -2e-9)                                             # ... and specks that pass a 0.0 gate under the floor
    nf = dc.noise_fields(W, H)[0].copy()                                          # pair 2: NaN and inf vectors among noise
    nf[::3, ::4, 0] = np.nan
    nf[1::3, 1::4, 1] = np.inf
    nf[2::3, 2::4] = (-np.inf, np.nan)
    nf[::5, 3::4] = (np.inf, np.inf)
    flow[2] = nf
    foe[3] = (-10.5, -7.25)                                                       # pair 3: exactly anti-radial, |flow| >= 12.7: every
    flow[3, ..., 0], flow[3, ..., 1] = -(xs - foe[3, 0]), -(ys - foe[3, 1])       # pixel lands in the top bin (179 degrees, 5.0 px)
    flow[4] = dc.noise_fields(W, H)[1]                                            # pair 4: all sky
    sky[4] = True
    sky[0, : H // 3] = True
    for a in (flow, foe, sky):
        a.setflags(write=False)
    return dict(flow=flow, foe=foe, sky=sky)


@functools.lru_cache(maxsize=None)
def large_batch() -> dict:
    W, H, B = LARGE
    k = np.arange(B) % dc.PHI_B
    flow = np.ascontiguousarray(dc.noise_fields(W, H)[k])
    flow *= (1.0 + 0.01 * (np.arange(B) // dc.PHI_B))[:, None, None, None].astype(np.float32)      # 70 different fields
    return dict(flow=flow, foe=dc.foes(W, H)[k], sky=dc.sky_masks(W, H, B), gt=gt_images(W, H, B))

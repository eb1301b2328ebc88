"""The C oracle's Farneback stages (oracle/farneback_oracle.c) against the float64 restatement of tests/stage_ref64.py, at the frames
and parameters of tests/stage_cases.py.  No GPU: this pins the oracle itself, which every GPU flow test trusts and which nothing the
reference holds can check (cv2 is not available).

A stage of the oracle evaluates the stage's expression in float32 (the sweep's window sums and solve in float64, as OpenCV does);
the restatement evaluates it in float64 from the definition.  Each comparison allows the oracle float32 rounding of the expression
and nothing more: |oracle - ref64| <= K x (roundings on the longest path) x 2^-24 x magnitude, magnitude = the same expression on
absolute values (stage_ref64 magnitude=True).  A wrong tap, weight, border rule, ig constant, sample position or solve moves a stage
by orders of magnitude more.

K (one per stage) is 4x the worst ratio measured over every case, layer and input here (printed by each test with -s; the
measurement is quoted next to each K), except where the bound is exact (the sweep's sums and solve)."""
import numpy as np
import pytest

import stage_ref64 as ref
from stage_cases import CASES, CASE_IDS, REF64_MAX_PIXELS, crafted_flow, images, smooth_flow

EPS = ref.EPS32
TINY = 2.0 ** -126 * 16
# 4x the worst |oracle - ref64| / (roundings x 2^-24 x magnitude) measured over all cases, layers and inputs of stage_cases:
K_BLUR = 0.75             # measured 0.186 (3840x2160, levels 5)
K_POLY = 0.42             # measured 0.104 (16x12, poly_n 3)
K_UPDATE = 2.2            # measured 0.533 (1000x562); also the sweep's M' (measured 0.489)
K_UPSAMPLE = 2.1          # measured 0.511 (3840x2160)
# not measured but exact: the sweep's window sums against _sliding_sum_bound (measured up to 0.68 of it) and its flow against the
# float32 rounding of the float64 solve (half an ulp <= 2^-24 |d|: measured 1.000 of it, as a correct rounding reaches)
K_FLOW = 1.0


def _layers(orc, c):
    p = c.oracle_params()
    for k in range(orc.num_layers(c.W, c.H, p)):
        w, h, sigma, ks = orc.layer_dims(c.W, c.H, p, k)
        if w * h <= REF64_MAX_PIXELS:
            yield k, w, h, sigma, ks


def _ratio(d, unit):
    """the worst |d| / unit; unit carries an absolute floor of float32's smallest normal (results far below it underflow)"""
    return float(np.max(np.abs(d) / (unit + TINY)))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_blur_resize_against_ref64(fb_oracle, case):
    worst = 0.0
    for img in images(case):
        for k, w, h, sigma, ks in _layers(fb_oracle, case):
            got = fb_oracle.blur_resize(img, w, h, ks, sigma).astype(np.float64)
            exp = ref.blur_resize(img, w, h, ks, sigma)
            unit = (2 * ks + 8) * EPS * 255.0                       # row taps, column taps, the bilinear resize; values <= 255
            r = _ratio(got - exp, unit)
            worst = max(worst, r)
            assert r <= K_BLUR, (case.name, k, r)
    print(f"\n[ref64] blur {case.name}: worst ratio {worst:.3f}")


def _expansions(orc, c, k, w, h, sigma, ks):
    return [orc.blur_resize(img, w, h, ks, sigma) for img in images(c)]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_polyexp_against_ref64(fb_oracle, case):
    worst = 0.0
    n = case.poly_n
    for k, w, h, sigma, ks in _layers(fb_oracle, case):
        for I in _expansions(fb_oracle, case, k, w, h, sigma, ks):
            got = fb_oracle.polyexp(I, n, case.poly_sigma).astype(np.float64)
            exp = ref.polyexp(I, n, case.poly_sigma)
            mag = ref.polyexp(I, n, case.poly_sigma, magnitude=True)
            unit = (4 * n + 4) * EPS * mag                          # 2n + 1 vertical and 2n + 1 horizontal taps, the ig products
            r = _ratio(got - exp, unit)
            worst = max(worst, r)
            assert r <= K_POLY, (case.name, k, r)
    print(f"\n[ref64] polyexp {case.name}: worst ratio {worst:.3f}")


def _stage_inputs(orc, c, k, w, h, sigma, ks):
    R = [orc.polyexp(I, c.poly_n, c.poly_sigma) for I in _expansions(orc, c, k, w, h, sigma, ks)]
    return R, [smooth_flow(w, h), crafted_flow(w, h)]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_update_matrices_against_ref64(fb_oracle, case):
    worst = 0.0
    for k, w, h, sigma, ks in _layers(fb_oracle, case):
        R, flows = _stage_inputs(fb_oracle, case, k, w, h, sigma, ks)
        for flow in flows:
            got = fb_oracle.update_matrices(R[0], R[1], flow).astype(np.float64)
            exp, mag = ref.update_matrices(R[0], R[1], flow, magnitude=True)
            unit = 16 * EPS * mag                                   # bilinear sample, averages, border weight, products: 16 roundings
            r = _ratio(got - exp, unit)
            worst = max(worst, r)
            assert r <= K_UPDATE, (case.name, k, r)
    print(f"\n[ref64] update_matrices {case.name}: worst ratio {worst:.3f}")


def _sliding_sum_bound(M, winsize):
    """How far the oracle's window sums may lie from exact ones: OpenCV slides its column sums down the image in double, but each
    step adds srow1[x] - srow0[x], a FLOAT difference of two M rows, rounded to float32 -- half an ulp per step, accumulating over all
    rows above -- and the sums start from srow0[x] * (m + 2), a float product.  Bound: 2^-24 x (that start plus the running sum of
    |srow1 - srow0| down each column), summed over the window's columns, / winsize^2."""
    m = winsize // 2
    M = np.asarray(M, np.float64)
    h, w = M.shape[:2]
    y = np.arange(h)
    steps = np.abs(M[np.minimum(y + m, h - 1)] - M[np.maximum(y - m - 1, 0)])
    col = np.cumsum(steps, axis=0) + (m + 2) * np.abs(M[:1])
    win = sum(col[:, np.clip(np.arange(w) + t, 0, w - 1)] for t in range(-m, m + 1))
    return EPS * win / float(winsize * winsize) + 2.0 ** -40 * ref.box_sums(np.abs(M), m) / float(winsize * winsize)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sweep_against_ref64(fb_oracle, case):
    """One FarnebackUpdateFlow_Blur sweep: the window sums the oracle solved from (its want_sys record) are the float64 box sums of
    M / winsize^2 up to the float32 row differences of OpenCV's sliding sum (_sliding_sum_bound); its flow is the float64 solve of
    that system rounded to float32; its M' is UpdateMatrices of that flow."""
    worst_sys = worst_flow = worst_m = 0.0
    for k, w, h, sigma, ks in _layers(fb_oracle, case):
        R, flows = _stage_inputs(fb_oracle, case, k, w, h, sigma, ks)
        for flow in flows:
            M = fb_oracle.update_matrices(R[0], R[1], flow)
            gflow, gM, sys = fb_oracle.blur_iter(R[0], R[1], flow, M, case.winsize, True, want_sys=True)
            G = ref.sweep_system(M, case.winsize)
            rs = _ratio(sys[..., :5] - G, _sliding_sum_bound(M, case.winsize))
            d = ref.solve(sys[..., :5])                             # the oracle's own system, solved in float64
            rf = _ratio(gflow - d, EPS * np.abs(d))                 # its flow: that solve rounded to float32, no more
            exp, mag = ref.update_matrices(R[0], R[1], gflow, magnitude=True)
            rm = _ratio(gM - exp, 16 * EPS * mag)
            worst_sys, worst_flow, worst_m = max(worst_sys, rs), max(worst_flow, rf), max(worst_m, rm)
            assert rs <= 1 and rf <= K_FLOW and rm <= K_UPDATE, (case.name, k, rs, rf, rm)
    print(f"\n[ref64] sweep {case.name}: worst ratios sums {worst_sys:.3f} flow {worst_flow:.3f} M' {worst_m:.3f}")


@pytest.mark.parametrize("case", [c for c in CASES if c.levels > 0 and c.W * c.H > 1000], ids=lambda c: c.name)
def test_flow_upsample_against_ref64(fb_oracle, case):
    worst = 0.0
    p = case.oracle_params()
    L = fb_oracle.num_layers(case.W, case.H, p)
    for k in range(L - 1):
        w, h = fb_oracle.layer_dims(case.W, case.H, p, k)[:2]
        pw, ph = fb_oracle.layer_dims(case.W, case.H, p, k + 1)[:2]
        for fc in (smooth_flow(pw, ph), crafted_flow(pw, ph)):
            got = fb_oracle.resize_flow(fc, w, h, 1.0 / case.pyr_scale).astype(np.float64)
            exp = ref.upsample_flow(fc, w, h, 1.0 / case.pyr_scale)
            mag = ref.upsample_flow(np.abs(fc), w, h, 1.0 / case.pyr_scale)
            r = _ratio(got - exp, 8 * EPS * mag)                    # two bilinear passes and the multiply
            worst = max(worst, r)
            assert r <= K_UPSAMPLE, (case.name, k, r)
    print(f"\n[ref64] upsample {case.name}: worst ratio {worst:.3f}")

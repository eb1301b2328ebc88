"""tests/gauss_window_ref.py, the numpy restatement the Gaussian-window kernels are held to bit for bit, checked on the CPU against
what its definition says: the taps' values, a constant field, float32 against float64, the symmetry of the two passes -- and that
the Gaussian flow is far enough from the box flow for the GPU tests to tell the two windows apart."""
import numpy as np
import pytest

import gauss_window_ref as gw

K12 = (0.15359142, 0.13162737, 0.08284836)       # k_0, k_1, k_2 for winsize 12 and 13
SUM12 = 0.69281721                               # k_0 + 2 sum_{i >= 1} k_i: the taps deliberately do not sum to 1
EPS = 2.0 ** -24


@pytest.mark.parametrize("winsize", [12, 13])
def test_taps_of_winsize_12(winsize):
    k = gw.taps(winsize)
    assert k.dtype == np.float32 and k.shape == (7,)
    for got, want in zip(k[:3], K12):
        assert got == np.float32(want), (got, want)
    # the sum as float32 arithmetic gives it; the exact sum of the seven float32 taps lies one float32 step (6e-8) below
    assert k[0] + np.float32(2) * k[1:].sum(dtype=np.float32) == np.float32(SUM12)
    assert abs(float(k[0]) + 2 * float(k[1:].astype(np.float64).sum()) - SUM12) <= 2.0 ** -24 + 5e-9     # (+ the 8 digits SUM12 is written to)
    assert np.all(np.diff(k) < 0)


def test_taps_sizes():
    for winsize in (2, 5, 9, 15, 31, 64):
        k = gw.taps(winsize)
        assert k.shape == (winsize // 2 + 1,) and np.all(k > 0) and np.all(np.diff(k) < 0)


def test_constant_field_is_scaled_by_the_taps_sum_squared():
    vals = np.array([1.0, -3.5, 0.25, 1000.0, 1e-3], np.float32)
    M = np.broadcast_to(vals, (40, 53, 5)).copy()
    S = gw.window_sums(M, 12)
    want = vals.astype(np.float64) * SUM12 ** 2
    # 2 passes of 13 products and 12 sums each, every one within 2^-24 relative
    assert np.all(np.abs(S - want) <= 2 * 15 * EPS * np.abs(want)), float(np.abs(S / want - 1).max())
    assert np.all(S == S[0, 0])                   # borders replicate: every pixel sees the same numbers in the same order


@pytest.mark.parametrize("winsize", [5, 12, 13, 31])
def test_float32_sums_stay_within_their_rounding_bound(winsize):
    rng = np.random.default_rng(5)
    M = (rng.normal(0, 1, (45, 70, 5)) * rng.choice([1e-3, 1.0, 300.0], (45, 70, 1))).astype(np.float32)
    m = winsize // 2
    S32 = gw.window_sums(M, winsize)
    S64 = gw.window_sums(M, winsize, np.float64)
    assert S32.dtype == np.float32 and S64.dtype == np.float64
    bound = (2 * m + 3) * EPS * gw.window_sums(np.abs(M), winsize, np.float64)
    ratio = float((np.abs(S32 - S64) / bound).max())
    print(f"\n[gauss ref] winsize {winsize}: max |f32 - f64| / bound = {ratio:.3g}")
    assert ratio <= 1.0


def test_transposed_field_with_swapped_passes():
    rng = np.random.default_rng(6)
    M = rng.normal(0, 10, (33, 47)).astype(np.float32)
    assert np.array_equal(gw.window_sums(M.T, 12, horizontal_first=True), gw.window_sums(M, 12).T)
    assert not np.array_equal(gw.window_sums(M, 12, horizontal_first=True), gw.window_sums(M, 12))   # the order of the passes is part of the bits


def test_solve_matches_its_formula_pixel_by_pixel():
    rng = np.random.default_rng(7)
    S = rng.normal(0, 5, (6, 7, 5)).astype(np.float32)
    S[0, 0] = 0                                   # a singular system: the 1e-3 regulariser alone
    f = gw.solve(S)
    assert f.dtype == np.float32 and f.shape == (6, 7, 2)
    for y in range(6):
        for x in range(7):
            g11, g12, g22, h1, h2 = (np.float32(v) for v in S[y, x])
            d = np.float32(np.float32(g11 * g22) - np.float32(g12 * g12))
            idet = 1.0 / (float(d) + 1e-3)
            u = np.float32(float(np.float32(np.float32(g11 * h2) - np.float32(g12 * h1))) * idet)
            v = np.float32(float(np.float32(np.float32(g22 * h1) - np.float32(g12 * h2))) * idet)
            assert (f[y, x, 0], f[y, x, 1]) == (u, v)
    assert tuple(f[0, 0]) == (0.0, 0.0)


@pytest.mark.parametrize("W,H,pair", [(96, 64, 1), (640, 480, 0)])
def test_gaussian_flow_differs_from_box_flow(fb_oracle, W, H, pair):
    """The windows must be distinguishable end to end: mean EPE above 1e-2 px (measured 0.147 px at 96x64, 0.047 px at 640x480),
    a hundred times the strict flow gate's mean."""
    from mavflow import synth
    from oracle import fb_oracle as fbo, tolerances
    prev, nxt = synth.make_pair(W, H, pair)[:2]
    p = fbo.default_params()
    e = tolerances.epe(gw.calc(fb_oracle, prev, nxt, p), fb_oracle.calc(prev, nxt, p))
    print(f"\n[gauss ref] {W}x{H}: mean EPE gaussian vs box = {float(e.mean()):.4g} px")
    assert e.mean() > 1e-2

"""The golden files of the Fourier transform (tests/golden/fft*.npz, written by tools/gen_golden_fft.py from the reference's own get_fft
and from scipy's longdouble transform) against tests/fft_ref.py: the numpy restatement of get_fft equals the reference's uint8 output
BY EQUALITY and its float outputs to the bounds a device form is to be held to; an independent O(n^2) DFT-matrix transform in longdouble agrees
with the stored truth; and the conditions on the inputs (no empty bin, no spectrum value within 1e-6 of an integer) hold for every
stored case, so that no pixel has to be set aside anywhere.  Runs without a GPU."""
import os

import numpy as np
import pytest

import fft_cases as fc
import fft_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return {k: np.load(os.path.join(GOLDEN, f), allow_pickle=False) for k, f in (("u8", "fft.npz"), ("f32", "fft_f32.npz"), ("f64", "fft_f64.npz"))}


def test_every_case_is_stored_with_its_seed_and_shape(gold):
    for c in fc.CASES:
        for k, seed in enumerate(c.seeds):
            key = f"{c.name}/{k}/"
            assert int(gold["u8"][key + "seed"]) == seed and gold["u8"][key + "shape"].tolist() == [c.H, c.W]
            assert gold["u8"][key + "truth_half"].shape == (c.H, c.W // 2 + 1) and gold["u8"][key + "truth_half"].dtype == np.complex128
            assert gold["u8"][key + "ref"].shape == (c.H, c.W) and gold["u8"][key + "ref"].dtype == np.uint8
    for c in fc.FLOAT_CASES:
        assert gold["f32"][f"{c.name}/ref"].dtype == np.float32 and gold["f64"][f"{c.name}/ref"].dtype == np.float64
    for f in ("fft.npz", "fft_f32.npz", "fft_f64.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20)


def test_conditions_on_the_inputs_hold_for_every_stored_case(gold):
    worst = 1.0
    for c in fc.CASES:
        for k in range(len(c.seeds)):
            F = fr.full_from_half(gold["u8"][f"{c.name}/{k}/truth_half"], c.W)
            assert (np.abs(F) > 0).all(), c.name
            s = fr.spectrum(F)
            frac = float(np.abs(s - np.rint(s)).min())
            assert frac > fc.INTEGER_MARGIN, (c.name, frac)
            assert abs(frac - float(gold["u8"][f"{c.name}/{k}/min_frac"])) < 1e-9          # the float64 logarithm against the longdouble one
            assert 59 < s.min() and s.max() < 305
            worst = min(worst, frac)
    assert 1.3e-5 < worst < 1.5e-5                                                         # 31 x 62, seed 7
    for kind in ("f32", "f64"):
        for c in fc.FLOAT_CASES:
            assert np.isfinite(gold[kind][f"{c.name}/s_half"]).all(), c.name              # no bin with |F| = 0


def test_restatement_equals_the_reference_on_uint8_frames_by_equality(gold):
    for c in fc.CASES:
        for k, seed in enumerate(c.seeds):
            frame = fc.frame_u8(seed, c.H, c.W)
            out = fr.get_fft(frame)
            assert out.dtype == np.uint8 and out.shape == frame.shape and not out[..., 1:].any()
            assert np.array_equal(out[..., 0], gold["u8"][f"{c.name}/{k}/ref"]), c.name
            # and both are the truth's spectrum truncated: the bytes are decided by the mathematics
            F = fr.full_from_half(gold["u8"][f"{c.name}/{k}/truth_half"], c.W)
            assert np.array_equal(out[..., 0], fr.to_uint8(fr.spectrum(F))), c.name


def _truth_spectrum(g, c):
    return fr.shift(fr.full_from_half(g[f"{c.name}/s_half"], c.W))


def test_restatement_and_reference_agree_on_float_frames_to_the_devices_bounds(gold):
    for c in fc.FLOAT_CASES:
        # float64 frames: per bin 20 g rms|F| / |F| + 64 ulp, with g = 4 x numpy's own stored error on this field
        g64 = gold["f64"]
        frame = fc.frame_float(c.seeds[0], c.H, c.W, np.float64)
        s_true = _truth_spectrum(g64, c)
        bound = 20.0 * fr.complex_bound(float(g64[f"{c.name}/numpy_err"])) * np.sqrt(float(g64[f"{c.name}/sum_sq"])) / np.exp(s_true / 20.0) \
            + 64 * np.spacing(np.abs(s_true))
        for what, out in (("restatement", fr.get_fft(frame)[..., 0]), ("reference", g64[f"{c.name}/ref"])):
            assert out.dtype == np.float64 and (np.abs(out - s_true) <= bound).all(), (c.name, what, float((np.abs(out - s_true) / bound).max()))
        # float32 frames: numpy transforms them in complex64; the reference's own distance from the truth rounded once is stored
        g32 = gold["f32"]
        frame = fc.frame_float(c.seeds[0], c.H, c.W, np.float32)
        once = _truth_spectrum(g32, c).astype(np.float32)
        allowed = int(g32[f"{c.name}/ref_ulps"])
        assert int(fr.ulps_f32(g32[f"{c.name}/ref"], once).max()) == allowed
        out = fr.get_fft(frame)
        assert out.dtype == np.float32 and not out[..., 1:].any()
        assert int(fr.ulps_f32(out[..., 0], g32[f"{c.name}/ref"]).max()) <= 2 * allowed, c.name     # two complex64 transforms, each that far from the truth


def test_dft_matrix_transform_agrees_with_the_stored_truth(gold):
    """an independent transform (no factorisation, no library) for the shapes up to 64 x 64.  Per bin the truth's own rounding to
    complex128 is 2^-52 |F|; the O(n^2) sums in longdouble (2^-64 per operation, H + W terms per bin, inputs up to 255) stay below
    2^-56 rms|F| at these sizes."""
    ran = 0
    for c in fc.CASES:
        if c.H > fc.DFT_MATRIX_MAX or c.W > fc.DFT_MATRIX_MAX:
            continue
        for k, seed in enumerate(c.seeds):
            F = fr.dft2_longdouble(fc.frame_u8(seed, c.H, c.W)[..., 0])
            T = fr.full_from_half(gold["u8"][f"{c.name}/{k}/truth_half"], c.W)
            err = np.abs(F - T.astype(np.clongdouble)).astype(np.float64)
            assert (err <= 2.0 ** -52 * np.abs(T) + 2.0 ** -56 * fr.rms(T)).all(), (c.name, float(err.max()))
            ran += 1
    assert ran >= 6


def test_numpys_stored_error_is_numpys_error_here(gold):
    """the bound of a device form is 4 x this figure: it is a property of numpy's transform on this input, reproduced here"""
    for c in fc.CASES:
        T = fr.full_from_half(gold["u8"][f"{c.name}/0/truth_half"], c.W)
        err = float(np.abs(np.fft.fft2(fc.frame_u8(c.seeds[0], c.H, c.W)[..., 0]) - T).max() / fr.rms(T))
        stored = float(gold["u8"][f"{c.name}/0/numpy_err"])
        assert 7e-18 < stored < 5e-15 and abs(err - stored) <= 2.0 ** -52 * 64, (c.name, err, stored)

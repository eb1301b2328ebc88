#!/usr/bin/env python3
"""Generate tests/golden/fft.npz, fft_f32.npz and fft_f64.npz: the REFERENCE's own im_helpers.get_fft on the seeded inputs of
tests/fft_cases.py, and the truth they are held to.

Run on the build machine only (it needs the reference tree and scipy):   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fft.py
The reference is imported in place with the placeholder modules of SURVEY.md section 8c (tools/gen_golden.py's recipe); nothing of it is
copied.  Per case the files hold results only -- the inputs are seeded (tests/fft_cases.py):

  fft.npz      per uint8 frame "<case>/<k>/": truth_half = scipy.fft.fft2 of the frame's channel 0 in longdouble, rounded to complex128,
               columns 0 .. W // 2 (the rest is the conjugate mirror); ref = channel 0 of the reference's uint8 output (channels 1, 2
               are asserted zero, the dtype uint8); numpy_err = max |F_numpy - F_true| / rms |F_true|; min_frac = the smallest
               distance of 20 ln|F_true| to an integer; seed, shape.
  fft_f32.npz  per float32 field "<case>/": s_half = 20 ln|F_true| in longdouble rounded to float64, unshifted, columns 0 .. W // 2;
               ref = channel 0 of the reference's float32 output; ref_ulps = its largest distance in float32 ulp from s_true rounded
               once (numpy transforms float32 in complex64: this is the reference's own error); sum_sq = sum x^2 (rms|F|^2 by Parseval).
  fft_f64.npz  per float64 field: s_half, ref (float64), numpy_err, sum_sq.

The generator ASSERTS the conditions of tests/fft_cases.py on every uint8 frame (no bin with |F_true| = 0, no 20 ln|F_true| within
INTEGER_MARGIN of an integer) and refuses to write a case that misses them, naming the first seed from the case's own on that does."""
import sys

sys.dont_write_bytecode = True
import os
import types

import numpy as np
import scipy.fft

REF = "/root/reference/src"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _placeholders():
    import matplotlib
    matplotlib.use("Agg")
    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_EPS = 2
    cv2.TERM_CRITERIA_COUNT = 1
    cv2.COLORMAP_JET = 2
    for name, mod in (("cv2", cv2), ("imutils", types.ModuleType("imutils")), ("flow_vis", types.ModuleType("flow_vis"))):
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, REF)


def truth(plane):
    """(F in clongdouble, 20 ln|F| in longdouble), unshifted"""
    F = scipy.fft.fft2(plane.astype(np.longdouble))
    assert F.dtype == np.clongdouble
    with np.errstate(divide="ignore"):
        return F, 20 * np.log(np.abs(F))


def conditions(plane, margin):
    F, s = truth(plane)
    if not (np.abs(F) > 0).all():
        return False, 0.0
    frac = float(np.abs(s - np.rint(s)).min())
    return frac > margin, frac


def rel_err(F, F_true):
    return float(np.abs(F.astype(np.clongdouble) - F_true).max() / np.sqrt(np.mean(np.abs(F_true) ** 2)))


def main():
    _placeholders()
    import im_helpers as ref_im
    import fft_cases as fc
    import fft_ref as fr

    u8, f32, f64 = {}, {}, {}
    for case in fc.CASES:
        H, W, Wh = case.H, case.W, case.W // 2 + 1
        for k, seed in enumerate(case.seeds):
            frame = fc.frame_u8(seed, H, W)
            ok, frac = conditions(frame[..., 0], fc.INTEGER_MARGIN)
            if not ok:
                good = next(s for s in range(seed + 1, seed + 1000) if conditions(fc.frame_u8(s, H, W)[..., 0], fc.INTEGER_MARGIN)[0])
                raise SystemExit(f"{case.name}: seed {seed} misses the conditions (smallest distance to an integer {frac:.3g}); "
                                 f"the next seed that meets them is {good}: put it into tests/fft_cases.py")
            out = ref_im.get_fft(frame)
            assert out.dtype == np.uint8 and out.shape == frame.shape and not out[..., 1:].any()
            F_true, s_true = truth(frame[..., 0])
            assert np.array_equal(out[..., 0], (np.trunc(np.fft.fftshift(s_true)).astype(np.int64) & 255).astype(np.uint8)), case.name
            key = f"{case.name}/{k}/"
            u8[key + "truth_half"] = F_true[:, :Wh].astype(np.complex128)
            u8[key + "ref"] = out[..., 0].copy()
            u8[key + "numpy_err"] = np.float64(rel_err(np.fft.fft2(frame[..., 0]), F_true))
            u8[key + "min_frac"] = np.float64(frac)
            u8[key + "seed"] = np.int64(seed)
            u8[key + "shape"] = np.array([H, W], np.int64)
            print(f"{key:18s} seed {seed}: s in [{float(s_true.min()):.1f}, {float(s_true.max()):.1f}], min distance to an integer {frac:.3g}, "
                  f"numpy's error {float(u8[key + 'numpy_err']):.3g}")
    for case in fc.FLOAT_CASES:
        H, W, Wh = case.H, case.W, case.W // 2 + 1
        for dtype, store in ((np.float32, f32), (np.float64, f64)):
            frame = fc.frame_float(case.seeds[0], H, W, dtype)
            F_true, s_true = truth(frame[..., 0])
            assert (np.abs(F_true) > 0).all(), case.name
            out = ref_im.get_fft(frame)
            assert out.dtype == dtype and out.shape == frame.shape and not out[..., 1:].any()
            key = f"{case.name}/"
            store[key + "s_half"] = s_true[:, :Wh].astype(np.float64)
            store[key + "ref"] = out[..., 0].copy()
            store[key + "sum_sq"] = np.float64((frame[..., 0].astype(np.longdouble) ** 2).sum())
            if dtype == np.float32:
                once = np.fft.fftshift(s_true).astype(np.float32)
                store[key + "ref_ulps"] = np.int64(fr.ulps_f32(out[..., 0], once).max())
                print(f"{key:18s} float32: the reference lies up to {int(store[key + 'ref_ulps'])} float32 ulp from the truth rounded once")
            else:
                store[key + "numpy_err"] = np.float64(rel_err(np.fft.fft2(frame[..., 0]), F_true))
    os.makedirs(OUT, exist_ok=True)
    for name, store in (("fft.npz", u8), ("fft_f32.npz", f32), ("fft_f64.npz", f64)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **store)
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < (1 << 20), "a committed file may not exceed 1 MiB"


if __name__ == "__main__":
    main()

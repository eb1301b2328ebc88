"""TEST INFRASTRUCTURE -- the numpy reference of the threshold sweep, brute force: for every (angle, magnitude) pair the oracle's
threshold block (oracle/foe_oracle.py threshold_masks) on the oracle's phi and magnitude, then calculate_tpr_fpr's four integer sums
with 255 * mask.  A frame-0 pair has float32 phi and magnitude and is compared against float32 thresholds, as numpy does there.
model_counts() restates the kernel's binning rule (strict counts, exact bins, a 2-D suffix sum) for tests/test_roc_ref_cpu.py."""
from __future__ import annotations

import numpy as np

from oracle import foe_oracle as fo


def sums(gt: np.ndarray, mask: np.ndarray) -> tuple:
    """im_helpers.calculate_tpr_fpr's sums (src/im_helpers.py:244-252) for img = 255 * mask: positives, negatives, tp, fp"""
    img = 255 * mask
    return (int(np.sum(gt > 127)), int(np.sum((255 - gt) > 127)), int(np.sum((gt * img) > 127)), int(np.sum(((255 - gt) * img) > 127)))


def ref_counts(phi: np.ndarray, mag: np.ndarray, sky, gt: np.ndarray, angles, mags) -> np.ndarray:
    """(Ka, Km, 4) int64 of one pair"""
    T = np.float32 if phi.dtype == np.float32 else np.float64
    out = np.empty((len(angles), len(mags), 4), np.int64)
    for i, a in enumerate(angles):
        for j, m in enumerate(mags):
            with np.errstate(all="ignore"):
                fixed, _ = fo.threshold_masks(phi, mag, sky, fixed_deg=T(a), fixed_min_mag=T(m))
            out[i, j] = sums(gt, fixed)
    return out


def model_counts(phi: np.ndarray, mag: np.ndarray, sky, gt: np.ndarray, angles, mags) -> np.ndarray:
    """The kernel's rule: ia = #{angles < phi}, im = #{mags < mag} (a NaN magnitude: 0), the exact bin (ia, im) per set pixel, tp where
    gt >= 1 and fp where gt <= 254, cell[i][j] = the sum of the bins (a > i, b > j)."""
    T = np.float32 if phi.dtype == np.float32 else np.float64
    a, m = np.asarray(angles, np.float64).astype(T), np.asarray(mags, np.float64).astype(T)
    ka, km = a.size, m.size
    ia = np.searchsorted(a, phi, side="left")
    im = np.where(np.isnan(mag), 0, np.searchsorted(m, mag, side="left"))
    live = (ia > 0) & (im > 0)
    if sky is not None:
        live &= ~np.asarray(sky, bool)
    out = np.empty((ka, km, 4), np.int64)
    out[..., 0], out[..., 1] = np.sum(gt > 127), np.sum(gt < 128)
    for k, sel in ((2, gt >= 1), (3, gt <= 254)):
        hist = np.zeros((ka + 1, km + 1), np.int64)
        np.add.at(hist, (ia[live & sel], im[live & sel]), 1)
        cum = hist[::-1, ::-1].cumsum(axis=0).cumsum(axis=1)[::-1, ::-1]          # cum[a][b] = sum of the bins (>= a, >= b)
        out[..., k] = cum[1:, 1:]
    return out

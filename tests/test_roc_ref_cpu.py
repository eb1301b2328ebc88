"""The threshold sweep without a GPU: the kernel's binning rule (tests/roc_ref.py model_counts: strict counts, exact bins, a 2-D suffix
sum) equals the brute-force reference on every case of tests/roc_cases.py, every case list obeys the ABI's rules, and the band condition
under which the GPU tests compare the device with the oracle by array_equal holds: no oracle pixel lies within PHI_ATOL (float64 pairs)
or ARCCOS_ULPS float32 ulps (frame-0 pairs) of an angle of ANG.  A condition, not a tolerance: the GPU comparison excuses nothing."""
import numpy as np
import pytest

import detect_cases as dc
import roc_cases as rc
import roc_ref as R
from test_frame0 import ARCCOS_ULPS, ulps32
from test_gpu_detect import PHI_ATOL


def _noise_pairs(case):
    """(call, b, phi, mag, sky, gt) for the nine shapes x four calls x three pairs"""
    fl, fe, sky, gt = dc.noise_fields(case.W, case.H), dc.foes(case.W, case.H), dc.sky_masks(case.W, case.H), rc.gt_images(case.W, case.H)
    for call in rc.CALLS:
        for b in range(dc.PHI_B):
            phi, mag = rc.oracle_fields(fl[b], call.mode(b), fe[b], dc.OMEGA[b], dc.DT[b])
            yield call, b, phi, mag, sky[b], gt[b]


def _planted_pairs(W, H):
    pl, gt = rc.planted(W, H), rc.gt_images(W, H, len(rc.PLANTED))
    for mode in ("plain", "frame0"):
        for k, name in enumerate(rc.PLANTED):
            phi, mag = rc.oracle_fields(pl["flow"][k], mode, pl["foe"][k])
            yield mode, name, phi, mag, pl["sky"][k], gt[k]


def _large_pairs():
    lb = rc.large_batch()
    for b in range(rc.LARGE[2]):
        phi, mag = rc.oracle_fields(lb["flow"][b], "plain", lb["foe"][b])
        yield b, phi, mag, lb["sky"][b], lb["gt"][b]


def _band(phi, angles) -> int:
    """oracle pixels inside the band around any of the angles"""
    n = 0
    for a in angles:
        if phi.dtype == np.float32:
            n += int((ulps32(phi, np.full_like(phi, np.float32(a))) <= ARCCOS_ULPS).sum())
        else:
            n += int((np.abs(phi - a) <= PHI_ATOL).sum())
    return n


def test_case_lists_obey_the_abi():
    for name, (a, m) in rc.GRIDS.items():
        assert rc.lists_valid(a, m), name
    assert rc.lists_valid(rc.ANG, rc.MAG_PLANTED)
    a, m = rc.GRIDS["max"]
    assert (len(a), len(m)) == (rc.MAX_ANGLES, rc.MAX_MAGS)
    a, _ = rc.GRIDS["collapse"]
    assert a[1] != a[2] and np.float32(a[1]) == np.float32(a[2])
    for name, (a, m) in rc.BAD_LISTS.items():
        assert not rc.lists_valid(a, m), name
    for W, H in [(c.W, c.H) for c in dc.PHI_CASES] + [rc.LARGE[:2]]:
        if W * H >= len(rc.GT_VALUES):
            assert all(set(np.unique(g)) == set(rc.GT_VALUES) for g in rc.gt_images(W, H)), (W, H)


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_model_equals_brute_force_on_the_noise_cases(case):
    grids = [g for g in rc.GRIDS if g != "max" or case.name == rc.MAX_GRID_CASE]
    for call, b, phi, mag, sky, gt in _noise_pairs(case):
        for g in grids:
            if g == "max" and call is not rc.CALLS[0] and call is not rc.CALLS[-1]:
                continue                                          # (the brute force of 1024 cells: one float64 and the float32 call)
            a, m = rc.GRIDS[g]
            assert np.array_equal(R.model_counts(phi, mag, sky, gt, a, m), R.ref_counts(phi, mag, sky, gt, a, m)), (case.name, call.name, b, g)
        assert np.array_equal(R.model_counts(phi, mag, None, gt, rc.ANG, rc.MAG), R.ref_counts(phi, mag, None, gt, rc.ANG, rc.MAG))


@pytest.mark.parametrize("shape", rc.PLANTED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_equals_brute_force_on_the_planted_fields(shape):
    seen = set()
    for mode, name, phi, mag, sky, gt in _planted_pairs(*shape):
        for a, m in ((rc.ANG, rc.MAG_PLANTED), rc.GRIDS["zero"], rc.GRIDS["right"], rc.GRIDS["collapse"]):
            got = R.model_counts(phi, mag, sky, gt, a, m)
            assert np.array_equal(got, R.ref_counts(phi, mag, sky, gt, a, m)), (shape, mode, name)
        seen.add(name)
        full = R.model_counts(phi, mag, sky, gt, rc.ANG, rc.MAG_PLANTED)
        if name == "int345":        # strictness: a magnitude exactly on the 5.0 threshold passes no 5.0 gate, and passes the 3.0 gate
            assert np.all(mag == 5.0) and not full[:, -1, 2:].any() and full[0, -2, 2:].any()
        if name == "antiradial":    # every pixel in the top bin: every cell holds the same counts
            assert np.all(full[..., 2:] == full[-1, -1, 2:]) and full[-1, -1, 2] == np.sum(gt >= 1) and full[-1, -1, 3] == np.sum(gt <= 254)
        if name in ("allsky", "zero"):
            assert not full[..., 2:].any()
        if name == "naninf":
            assert np.isnan(mag).any() and np.isinf(mag).any() and not np.isnan(phi).any()
    assert seen == set(rc.PLANTED)


def test_strictness_on_an_angle_threshold():
    """phi exactly on a threshold is not above it, in either arithmetic"""
    for T in (np.float32, np.float64):
        phi = np.array([[15.0, np.nextafter(T(15.0), T(16.0)), 0.0, 180.0]], T)
        mag = np.array([[2.0, 2.0, 2.0, np.nan]], T)
        gt = np.array([[255, 255, 255, 255]], np.uint8)
        got = R.model_counts(phi, mag, None, gt, [10.0, 15.0, 20.0], [1.0])
        assert np.array_equal(got, R.ref_counts(phi, mag, None, gt, [10.0, 15.0, 20.0], [1.0]))
        assert got[:, 0, 2].tolist() == [2, 1, 0]


def test_model_equals_brute_force_on_the_large_batch():
    for b, phi, mag, sky, gt in _large_pairs():
        assert np.array_equal(R.model_counts(phi, mag, sky, gt, rc.ANG, rc.MAG), R.ref_counts(phi, mag, sky, gt, rc.ANG, rc.MAG)), b


def test_band_condition():
    """what lets the GPU tests compare with the oracle by equality on ANG (x MAG, x MAG_PLANTED): 0 pixels in the band"""
    n = 0
    for case in dc.PHI_CASES:
        for call, b, phi, mag, sky, gt in _noise_pairs(case):
            n += _band(phi, rc.ANG)
    for shape in rc.PLANTED_SHAPES:
        for mode, name, phi, mag, sky, gt in _planted_pairs(*shape):
            gate = ~sky & (mag > 0.25)                            # a pixel no gate of the grid lets through decides nothing
            n += _band(phi[gate], rc.ANG)
    for b, phi, mag, sky, gt in _large_pairs():
        n += _band(phi, rc.ANG)
    assert n == 0

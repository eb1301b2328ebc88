"""tests/validation_ref.py against tests/golden/validation.npz, bit for bit: what the REFERENCE's own Dataset.validate_sky_segment,
im_helpers.calculate_tpr_fpr / get_simple_bounding_box, Detector.derotate and np.average gave for the stored inputs
(tools/gen_golden_validation.py) is what the restatement's records say.  And the two numpy rules for the depth threshold: equal on the
golden's maxima, different on the field tests/validation_cases.py builds for that.  Runs without a GPU."""
import os

import numpy as np
import pytest

import validation_cases as T
import validation_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validation.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLDEN["cases"]]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _nan_canonical(a):
    a = np.array(a)
    a[np.isnan(a)] = np.nan
    return a


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_references_results(name):
    g = {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}
    seg, index = g["seg"], int(g["index"])
    H, W = seg.shape
    flags = R.FRAME0 if index < 1 else 0
    for legacy in (False, True):                                   # the golden's maxima are 100.0: 80.0 by either rule
        rec, idx = R.gt_stats(seg, g["gt"], g["sky"], g["depth"], g["omega"], float(g["dt"]), flags | (R.THR_F64 if legacy else 0), max_pixels=seg.size)
        assert rec["drone_pixels"] == g["size"] == rec["listed"]
        rows, cols = np.nonzero(seg > 127)
        assert np.array_equal(idx[:rows.size], rows * W + cols) and (idx[rows.size:] == -1).all()
        pos, neg, tp, fp = (int(v) for v in rec["sky"])
        with np.errstate(all="ignore"):
            rates = np.array([np.float64(tp) / np.float64(pos), np.float64(fp) / np.float64(neg)])
        assert _same_bits(_nan_canonical(rates), _nan_canonical(g["sky_rates"]))
        assert pos + neg == seg.size and rec["depth_max"] == np.float32(100.0) and rec["flags"] == 0
        x0, y0, x1, y1 = (int(v) for v in rec["box"])
        assert _same_bits(np.array([x0, y0, x0 + (x1 - x0), y0 + (y1 - y0)], np.float64), g["box"])
        assert _same_bits(np.array([x0 + (x1 - x0) / 2, y0 + (y1 - y0) / 2], np.float64), g["center"])
        avg = R.drone_flow_avg_frame0(rec) if index < 1 else R.drone_flow_avg(rec)
        assert avg.dtype == g["avg"].dtype
        assert _same_bits(_nan_canonical(avg), _nan_canonical(g["avg"])), (name, avg, g["avg"])
        if index >= 1 and rows.size:
            assert _same_bits(R.derotated_at(g["gt"][rows, cols], rows, cols, W, H, g["omega"], float(g["dt"])), g["derotated"][rows, cols])


def test_golden_covers_the_shapes_it_is_there_for():
    shapes = {GOLDEN[f"{n}_seg"].shape for n in NAMES}
    assert {(71, 97), (1, 1), (2, 65)} <= shapes and max(h * w for h, w in shapes) <= 97 * 71
    assert any(int(GOLDEN[f"{n}_index"]) == 0 for n in NAMES) and any(int(GOLDEN[f"{n}_size"]) == 0 for n in NAMES)
    assert any(int(GOLDEN[f"{n}_size"]) == GOLDEN[f"{n}_seg"].size for n in NAMES)
    assert all(np.max(GOLDEN[f"{n}_depth"]) == 100.0 for n in NAMES)


def test_sequential_sum_is_numpys_average():
    """np.average(a, axis=0) of an (n, 2) array is the row-by-row sum from 0 divided by n -- float64 and float32 rows alike"""
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 8, 9, 127, 128, 129, 1000, 4099):
        for dtype in (np.float64, np.float32):
            a = (rng.normal(0, 3, (n, 2)) * 10.0 ** rng.integers(-3, 4, (n, 2))).astype(dtype)
            assert _same_bits(np.average(a, axis=0), R.sequential_sum(a) / dtype(n)), (n, dtype)


def test_the_two_threshold_rules():
    assert R.fraction_as_given(np.float32(0.8)) == 0.8 and R.fraction_as_given(np.float32(0.5)) == 0.5
    assert R.fraction_as_given(np.float32(0.123456789)) == 0.12345679            # the shortest decimal that rounds to the float32
    assert R.depth_threshold(100.0, 0.8, False) == R.depth_threshold(100.0, 0.8, True) == np.float32(80.0)
    m, a, b = T.parting_depth_max()
    assert a != b and a == np.float32(0.8) * m and b == np.float32(0.8 * np.float64(m))
    # the installed numpy's own rule is one of the two
    d = np.array([m, a, b], np.float32)
    own = int(np.sum(d > 0.80 * np.max(d)))
    new, old = int(np.sum(d > a)), int(np.sum(d > b))
    assert new != old
    assert own == (new if np.lib.NumpyVersion(np.__version__) >= "2.0.0" else old)
    x = T.inputs("thresholds part")
    y = T.inputs("thresholds part, legacy")
    assert np.array_equal(x["depth"], y["depth"]) and not np.array_equal(x["ref"][0]["sky"], y["ref"][0]["sky"])
    assert x["ref"][0]["sky"][0][0] != y["ref"][0]["sky"][0][0]                         # another number of pixels above the threshold

"""tests/truth_ref.py against arrays the reference's own functions produced (tests/golden/truth.npz, tools/gen_golden_truth.py): the
ground-truth flow bit for bit (NaN by position), its float32 form as the float64 one rounded, and the histogram restatement against
numpy.histogram2d of what analyze_radial_error saved.  Runs without a GPU."""
import os

import numpy as np
import pytest

import truth_cases as T
import truth_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truth.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN, allow_pickle=False)


def test_fixture_holds_the_cases_the_tests_need(g):
    assert set(g["cases"]) >= {"p97", "p13", "one", "p5", "ident", "zero", "allmav", "wcross"} and set(g["hist_cases"]) == {"h53", "h97"}
    for name in g["cases"]:
        H, W = g[f"{name}_depth"].shape
        assert W <= 97 and H <= 71 and g[f"{name}_result"].shape == (W, H, 2) and g[f"{name}_result"].dtype == np.float64
        assert g[f"{name}_depth"].dtype == np.float32 and g[f"{name}_seg"].dtype == np.uint8
    assert os.path.getsize(GOLDEN) < 1 << 20
    w = g["wcross_result"]
    assert np.isinf(w).any() and np.isnan(w).any() and np.isfinite(w).any()
    assert (g["allmav_seg"] > 0).all() and not g["zero_depth"].any() and np.array_equal(g["ident_vp1"], np.eye(4))


def test_gt_flow_restatement_equals_the_reference_bit_for_bit(g):
    for name in g["cases"]:
        x = T.fixture_inputs(g, str(name))
        got = R.gt_flow(x["depth"][0], x["seg"][0], x["vp1"][0], x["inv"][0], x["disp"][0], x["scale"])
        assert got.dtype == np.float64 and R.same_bits(got, x["ref64"][0]), name
        # the inverse the fixture stores is what numpy.linalg.inv gives here too (a different LAPACK would only move this line)
        assert np.array_equal(np.linalg.inv(x["vp2"][0]), x["inv"][0]), name


def test_float32_output_is_the_float64_one_rounded(g):
    for name in g["cases"]:
        x = T.fixture_inputs(g, str(name))
        got = R.gt_flow_f32(x["depth"][0], x["seg"][0], x["vp1"][0], x["inv"][0], x["disp"][0], x["scale"])
        with np.errstate(all="ignore"):
            want = x["ref64"][0].astype(np.float32)
        assert got.dtype == np.float32 and R.same_bits(got, want), name


def test_depth_scale_is_a_float32_product(g):
    x = T.fixture_inputs(g, "p97")
    assert x["scale"] == 100.0
    pre = x["depth"][0] * np.float32(100)
    assert pre.dtype == np.float32
    assert R.same_bits(R.gt_flow(pre, x["seg"][0], x["vp1"][0], x["inv"][0], x["disp"][0], 1.0), x["ref64"][0])


def test_histogram_restatement_equals_histogram2d_of_what_the_reference_saved(g):
    for name in g["hist_cases"]:
        flow, gt, sky = g[f"{name}_flow"], g[f"{name}_gt"], g[f"{name}_sky"]
        mag, err = R.radial_values(flow, gt, sky)
        saved = g[f"{name}_saved"]
        assert mag.dtype == err.dtype == np.float32 and np.array_equal(mag, saved[0]) and np.array_equal(err, saved[1]), name
        h = R.radial_hist(flow, gt, sky)
        assert np.array_equal(h["counts"], g[f"{name}_counts"]) and h["counts"].dtype == np.int64, name
        assert h["non_sky"] == int((~sky).sum()) and h["in_range"] == int(g[f"{name}_counts"].sum()), name
        counts, _, _ = np.histogram2d(saved[0], saved[1], bins=(R.DEFAULT_MAG_EDGES, R.DEFAULT_ERR_EDGES))
        assert np.array_equal(counts, h["counts"]), name


def test_bin_rule_at_the_edges():
    e = np.array([0.0, 1.0, 2.5])
    k, ok = R.bin_index(np.array([0.0, 0.999, 1.0, 2.5, 2.5000001, -1e-9, np.nan, np.inf]), e)
    assert list(ok) == [True, True, True, True, False, False, False, False] and list(k[:4]) == [0, 0, 1, 1]

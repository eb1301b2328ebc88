"""tests/kmeans_ref.py's paint held to tests/golden/clustering.npz by equality: what the reference's OWN Detector.clustering lines
(src/detector.py:414-428) produce behind a placeholder cv2.kmeans that returns given labels and centres (tools/gen_golden_clustering.py):
res, rgb and mask for enable_raw both ways, an all-zero centre table (max_mag -> 1.0), and centres whose scaled values land on x.999 and
x.0 either side of an integer and of the mask's 225.  Runs without a GPU."""
import os

import numpy as np
import pytest

import kmeans_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clustering.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLDEN["cases"]]


def test_the_golden_cases_are_the_ones_promised():
    assert NAMES == ["plain", "zero", "edge", "bright"]
    assert not GOLDEN["zero_centers"].any() and not GOLDEN["zero_res"].any() and not GOLDEN["zero_mask"].any()
    c = GOLDEN["edge_centers"].astype(np.float64)
    frac = c - np.floor(c)
    assert c.max() == 255.0 and np.sum(np.isclose(frac, 0.999, atol=2e-4)) >= 6 and np.sum(frac == 0.0) >= 6
    assert {224, 225} <= set(GOLDEN["edge_res"].reshape(-1).tolist())            # either side of the mask's threshold
    for n in NAMES:
        assert GOLDEN[f"{n}_mask"].any() == (n != "zero")


@pytest.mark.parametrize("name", NAMES)
def test_paint_equals_the_references_lines(name):
    labels, centers, shape = GOLDEN[f"{name}_labels"], GOLDEN[f"{name}_centers"], tuple(GOLDEN[f"{name}_shape"])
    assert labels.shape == (shape[0] * shape[1] // 3, 1) and labels.dtype == np.int32 and centers.dtype == np.float32
    res, empty = R.paint_image(labels, centers, shape, enable_raw=True)
    assert res.dtype == np.uint8 and np.array_equal(res, GOLDEN[f"{name}_res"]) and empty.shape == (0,)
    rgb, mask = R.paint_image(labels, centers, shape)
    assert rgb.dtype == np.uint8 and mask.dtype == bool
    assert np.array_equal(rgb, GOLDEN[f"{name}_rgb"]) and np.array_equal(mask, GOLDEN[f"{name}_mask"])
    flat, m = R.paint(labels, centers)                                            # the C call's form: per sample
    assert np.array_equal(flat.reshape(shape), GOLDEN[f"{name}_res"])
    assert np.array_equal(m.astype(bool), GOLDEN[f"{name}_mask"].reshape(-1, 3)[:, 0])


def test_a_size_not_divisible_by_three_is_numpys_error():
    with pytest.raises(ValueError):
        np.zeros((4, 5), np.float32).reshape((-1, 3))

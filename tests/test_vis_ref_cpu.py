"""tests/vis_ref.py, the numpy side of include/mavflow_vis.h, held to what it restates: the reference-made fixture (tests/golden/vis.npz,
tools/gen_vis_fixtures.py) bit for bit; BGR -> HSV to colorsys' float definition; the line iterator to the definition of an 8-connected
line independently of its stepping; the clip to the image.  No GPU."""
import colorsys
import os

import numpy as np
import pytest

import vis_cases as vc
import vis_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis.npz")
KEYS = ("66x33", "131x67")


@pytest.fixture(scope="module")
def fixture():
    return vc.load_fixture(GOLDEN)


@pytest.mark.parametrize("key", KEYS)
def test_draw_hsv_stage_equals_the_reference_made_image(fixture, key):
    flow = fixture[f"flow_{key}"]
    assert flow.dtype == np.float32 and (flow < 0).any()
    assert np.array_equal(R.draw_hsv_stage(flow), fixture[f"hsv_{key}"])
    assert not vc.in_band(R.draw_hue_float(flow)).any()                  # the margin the GPU test relies on


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("step", (8, 1))
def test_flow_lines_equal_the_reference_made_lines_and_centres(fixture, key, step):
    flow = fixture[f"flow_{key}"]
    H, W = flow.shape[:2]
    lines = R.flow_lines(flow, step, 1.0)
    want = fixture[f"lines_{key}_step{step}"]
    assert lines.dtype == np.int32 and want.dtype == np.int16 and np.array_equal(lines, want) and len(lines) > 10      # (stored in two bytes each)
    if step == 8:
        centres = fixture[f"centres_{key}_step{step}"]
        assert np.array_equal(centres[:, :2], lines[:, 0]) and (centres[:, 2] == 1).all() and (centres[:, 3] == -1).all()
    else:                                          # the generator held the centres to lines[:, 0]: count, the one radius, the one thickness
        assert list(fixture[f"circles_{key}_step{step}"]) == [len(lines), 1, -1]
    ends = lines[:, 1]
    assert (ends[:, 0] < 0).any() and (ends[:, 0] >= W).any() and (ends[:, 1] < 0).any() and (ends[:, 1] >= H).any()     # across every border
    assert len(lines) < len(R.grid_points(W, H, step)[0])                # and some points below the threshold


def test_bgr2hsv_against_the_float_definition():
    """within 1 hue step (mod 180) and 1 saturation level of colorsys.rgb_to_hsv on the stride-3 lattice (255 is on it); V exact"""
    tri = vc.lattice()
    got = R.bgr2hsv(tri).astype(np.int64)
    assert got[:, 0].max() < 180
    b, g, r = (tri[:, k].astype(np.float64) / 255.0 for k in range(3))
    hsv = np.array([colorsys.rgb_to_hsv(*p) for p in zip(r.tolist(), g.tolist(), b.tolist())])
    dh = np.abs(got[:, 0] - hsv[:, 0] * 180.0)
    dh = np.minimum(dh, 180.0 - dh)
    assert dh.max() <= 1.0, dh.max()
    assert np.abs(got[:, 1] - hsv[:, 1] * 255.0).max() <= 1.0
    assert np.array_equal(got[:, 2], tri.max(axis=1))
    sdiv, hdiv = R.div_tables()
    assert sdiv[0] == hdiv[0] == 0 and sdiv[255] == 4096 and hdiv[255] == 482 and sdiv[1] == 255 << 12


def _check_line(p1, p2):
    px = R.line_pixels(p1, p2)
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    n = max(abs(dx), abs(dy)) + 1
    assert len(px) == n and len(set(px)) == n, (p1, p2)
    assert tuple(p1) in px and tuple(p2) in px, (p1, p2)
    for a, b in zip(px, px[1:]):
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1, (p1, p2)            # 8-connected
    for x, y in px:                                                                # within half a pixel of the ideal line along the minor axis
        if abs(dx) >= abs(dy):
            assert n == 1 or 2 * abs((y - p1[1]) * dx - (x - p1[0]) * dy) <= abs(dx), (p1, p2, x, y)
        else:
            assert 2 * abs((x - p1[0]) * dy - (y - p1[1]) * dx) <= abs(dy), (p1, p2, x, y)
    assert set(px) == set(R.line_pixels(p2, p1)), (p1, p2)                        # the same set from either direction


def test_line_pixels_is_an_8_connected_line():
    rng = np.random.default_rng(5)
    W, H = 67, 131
    for x1, y1, x2, y2 in zip(rng.integers(0, W, 2000), rng.integers(0, H, 2000), rng.integers(0, W, 2000), rng.integers(0, H, 2000)):
        _check_line((int(x1), int(y1)), (int(x2), int(y2)))
    for a in range(81):
        for b in range(81):
            _check_line((a % 9, a // 9), (b % 9, b // 9))


def test_clip_line_keeps_a_segment_inside_and_rejects_what_is_outside():
    rng = np.random.default_rng(6)
    W, H = 67, 131
    accepted = rejected = 0
    for _ in range(3000):
        p1 = (int(rng.integers(-80, W + 80)), int(rng.integers(-80, H + 80)))
        p2 = (int(rng.integers(-80, W + 80)), int(rng.integers(-80, H + 80)))
        ok, q1, q2 = R.clip_line(W, H, p1, p2)
        inside = lambda p: 0 <= p[0] < W and 0 <= p[1] < H
        if ok:
            accepted += 1
            assert all(inside(p) for p in R.line_pixels(q1, q2)), (p1, p2, q1, q2)
            if inside(p1):
                assert q1 == p1
            if inside(p2):
                assert q2 == p2
        else:
            rejected += 1
            assert not inside(p1) and not inside(p2)
        for lo, hi, k in ((None, -1, 0), (W, None, 0), (None, -1, 1), (H, None, 1)):         # both ends beyond one side: rejected
            beyond = lambda p: (p[k] <= hi) if lo is None else (p[k] >= lo)
            if beyond(p1) and beyond(p2):
                assert not ok, (p1, p2)
    assert accepted > 500 and rejected > 500


def test_draw_flow_ref_draws_the_circles_and_clipped_lines():
    img = np.zeros((9, 12, 3), np.uint8)
    flow = np.zeros((9, 12, 2), np.float32)
    flow[4, 4] = (100.0, -2.0)                               # step 8: the one grid point (4, 4); its line leaves through the right border
    out = R.draw_flow(img, flow, 8, 1.0, (1, 2, 3))
    assert not img.any()                                     # a copy is drawn into
    on = out.any(axis=2)
    assert on[4, 3:6].all() and on[3, 4] and on[5, 4] and on[:, 11].any() and (out[on] == (1, 2, 3)).all()
    assert np.array_equal(R.draw_flow(img, flow, 8, 200.0), img)          # below the threshold: unchanged
    assert np.array_equal(R.draw_flow(img, flow, 8, float("nan")), img)   # a NaN threshold draws nothing

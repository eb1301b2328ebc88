"""tests/lk_ref.py (the CPU restatement of the corner detector and the pyramidal LK tracker) against things it was not written from:
constant and ramp images, exact integer translations, a rectangle's four vertices, the synthetic pairs' analytic flow -- and the C-ABI
of the sparse path as far as it can be exercised without a GPU."""
import ctypes as C

import numpy as np
import pytest

import lk_ref

F = np.float32


def blurred_noise(W, H, seed, sigma=2.0):
    """Wrap-around Gaussian blur (radius 4 sigma) of uniform noise, stretched to 0 .. 255: a periodic texture with corners everywhere."""
    rng = np.random.default_rng(seed)
    a = rng.random((H, W))
    r = int(4 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        a = sum(k[i + r] * np.roll(a, i, axis=axis) for i in range(-r, r + 1))
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def test_pyrdown_of_a_constant_is_that_constant():
    for v in (0, 1, 127, 255):
        for shape in ((48, 64), (37, 51)):
            out = lk_ref.pyr_down(np.full(shape, v, np.uint8))
            assert out.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) and np.all(out == v)


def test_scharr_of_a_unit_ramp():
    img = np.tile(np.arange(100, dtype=np.uint8), (40, 1))
    d = lk_ref.scharr(img)
    assert d.dtype == np.int16 and d.shape == (40, 100, 2)
    assert np.all(d[1:-1, 1:-1, 0] == 32) and np.all(d[1:-1, 1:-1, 1] == 0)
    d = lk_ref.scharr(img.T.copy())
    assert np.all(d[1:-1, 1:-1, 0] == 0) and np.all(d[1:-1, 1:-1, 1] == 32)


def test_pyramid_stops_by_the_window_rule():
    img = np.zeros((240, 320), np.uint8)
    assert [p.shape for p in lk_ref.build_pyramid(img, (21, 21), 3)] == [(240, 320), (120, 160), (60, 80), (30, 40)]
    assert len(lk_ref.build_pyramid(img, (21, 21), 5)) == 4            # (15, 20) is not larger than the window
    assert len(lk_ref.build_pyramid(img, (31, 31), 5)) == 3
    assert len(lk_ref.build_pyramid(img, (21, 21), 0)) == 1


@pytest.mark.parametrize("shift", [(2, 3), (5, -4), (0, 1)])
def test_integer_translation_is_tracked(shift):
    """A frame and its exact integer translate: every corner at least 40 px inside tracks to the translation within 0.05 px, status 1.
    (The restatement leaves at most 7e-4 px here; 0.05 is a sanity bound, not a fit.)"""
    a = blurred_noise(320, 240, 1)
    b = np.roll(a, shift, axis=(0, 1))
    pts = lk_ref.good_features(a)
    pts = pts[(pts[:, 0] > 40) & (pts[:, 0] < 280) & (pts[:, 1] > 40) & (pts[:, 1] < 200)]
    assert len(pts) > 100
    out, status = lk_ref.lk_track(a, b, pts)
    err = np.hypot(out[:, 0] - pts[:, 0] - shift[1], out[:, 1] - pts[:, 1] - shift[0])
    print(f"shift {shift}: {len(pts)} points, max error {err.max():.2e} px")
    assert np.all(status == 1)
    assert err.max() < 0.05


def test_rectangle_has_four_corners():
    img = np.zeros((120, 160), np.uint8)
    img[40:80, 50:110] = 255                       # 60 x 40, vertices (50, 40) (109, 40) (50, 79) (109, 79)
    pts = lk_ref.good_features(img)
    assert len(pts) == 4
    for vx, vy in ((50, 40), (109, 40), (50, 79), (109, 79)):
        d = np.hypot(pts[:, 0] - vx, pts[:, 1] - vy)
        assert (d <= 3).sum() == 1, (vx, vy, pts)


@pytest.mark.parametrize("min_distance", [1, 7])
def test_corner_spacing_and_order(min_distance):
    img = blurred_noise(320, 240, 3)
    pts, vals, _ = lk_ref.good_features(img, min_distance=min_distance, want_values=True)
    assert len(pts) > 50 and np.all(np.diff(vals) <= 0)
    d = pts[:, None, :] - pts[None, :, :]
    d2 = (d * d).sum(-1) + np.eye(len(pts)) * 1e9
    assert d2.min() >= min_distance * min_distance
    assert pts[:, 0].min() >= 1 and pts[:, 0].max() <= 318 and pts[:, 1].min() >= 1 and pts[:, 1].max() <= 238


@pytest.mark.parametrize("W,H", [(320, 240), (640, 480)])
def test_synthetic_pair_against_its_analytic_flow(W, H, mav):
    """Corners of synth.make_pair(W, H, 0), tracked, against the pair's analytic flow at the corner.
    The restatement's own figures: 320x240: 574 corners (1 516 candidates), 573 with status 1, 0.9215 of those within 0.1 px;
    640x480: 2 000 corners (5 700 candidates), 1 978 with status 1, 0.9226 within 0.1 px (the rest sit on the periodic texture's aliases
    and on the moving patch).  Gates: status-1 share >= 0.98, share within 0.1 px >= 0.90."""
    from mavflow import synth
    f0, f1, truth = synth.make_pair(W, H, 0)
    pts = lk_ref.good_features(f0)
    assert (len(pts) < 2000) if W == 320 else (len(pts) == 2000)         # one shape ends below maxCorners, one hits it
    out, status = lk_ref.lk_track(f0, f1, pts)
    tr = truth[pts[:, 1].astype(int), pts[:, 0].astype(int)]
    err = np.hypot(*(out - pts - tr).T)
    ok = status == 1
    print(f"{W}x{H}: {len(pts)} corners, {ok.sum()} status 1, share within 0.1 px {(err[ok] < 0.1).mean():.4f}")
    assert ok.mean() >= 0.98
    assert (err[ok] < 0.1).mean() >= 0.90


def test_non_finite_and_outside_points_fail_without_indexing():
    img = blurred_noise(160, 120, 5)
    pts = np.array([[np.nan, 10], [10, np.inf], [-500, 50], [1e30, 50], [80, 60]], F)
    out, status = lk_ref.lk_track(img, img, pts)
    assert status.tolist() == [0, 0, 0, 0, 1]
    assert np.allclose(out[4], (80, 60), atol=1e-3)


# ---- the C-ABI without a GPU ----------------------------------------------------------------------------------------------------------
def test_sparse_defaults_are_the_references(mav):
    from mavflow import _lib
    g = _lib.gftt_defaults()
    assert (g.max_corners, g.quality_level, g.min_distance, g.block_size) == (2000, 0.2, 7.0, 7)
    k = _lib.lk_defaults()
    assert (k.win_w, k.win_h, k.max_level, k.max_count, k.epsilon, k.min_eig_threshold) == (21, 21, 3, 30, 0.01, 1e-4)
    k = _lib.lk_defaults(winSize=(15, 17), maxLevel=2, criteria=(3, 10, 0.03), minEigThreshold=1e-3)
    assert (k.win_w, k.win_h, k.max_level, k.max_count, k.epsilon, k.min_eig_threshold) == (15, 17, 2, 10, 0.03, 1e-3)


def test_sparse_argument_errors_need_no_device(mav):
    """Parameter errors are refused before the context or a device is looked at: MAV_ERR_ARG with a message that names the bound."""
    from mavflow import _lib
    lib = _lib.load()
    n = C.c_int()

    def track(n_pts=0, **kw):
        return lib.mav_lk_track(None, None, None, None, n_pts, C.byref(_lib.lk_defaults(**kw)), None, None)

    def corners(**kw):
        return lib.mav_good_features(None, None, C.byref(_lib.gftt_defaults(**kw)), None, C.byref(n))

    for kw, word in (({"winSize": (20, 21)}, b"odd"), ({"winSize": (21, 0)}, b"odd"), ({"winSize": (35, 35)}, b"33 x 33"),
                     ({"max_level": -1}, b"max_level"), ({"max_level": 8}, b"max_level")):
        assert track(**kw) == _lib.MAV_ERR_ARG, kw
        assert word in lib.mav_last_error(), (kw, lib.mav_last_error())
    assert track(-1) == _lib.MAV_ERR_ARG and b"points" in lib.mav_last_error()
    assert track(_lib.LK_MAX_POINTS + 1) == _lib.MAV_ERR_ARG and str(_lib.LK_MAX_POINTS).encode() in lib.mav_last_error()
    for kw, word in (({"block_size": 6}, b"odd"), ({"block_size": 17}, b"15"), ({"max_corners": 0}, b"max_corners"),
                     ({"quality_level": 0.0}, b"quality_level"), ({"min_distance": -1.0}, b"min_distance")):
        assert corners(**kw) == _lib.MAV_ERR_ARG, kw
        assert word in lib.mav_last_error(), (kw, lib.mav_last_error())
    # good parameters, no context: still an argument error, not a crash
    assert track() == _lib.MAV_ERR_ARG and corners() == _lib.MAV_ERR_ARG
    assert lib.mav_lk_level_dims(None, 0, None, None) == _lib.MAV_ERR_ARG


def test_lucas_kanade_constructor_touches_no_gpu(mav):
    """The reference's fields and its one draw from the global RNG (lucas_kanade.py:13-32)."""
    from mavflow.detector import LucasKanade
    frame = np.zeros((48, 64, 3), np.uint8)
    np.random.seed(7)
    lk = LucasKanade(frame)
    after = np.random.randint(0, 1 << 30)
    np.random.seed(7)
    color = np.random.randint(0, 255, (2666, 3))
    assert np.random.randint(0, 1 << 30) == after
    assert np.array_equal(lk.color, color)
    assert (lk.num_corners, lk.minimum_num_corners, lk.total_num_corners, lk.num_features, lk.features) == (2000, 666, 2666, 0, [])
    assert lk.corners.shape == (2666, 2) and lk.old_frame is frame
    assert lk.feature_params == dict(maxCorners=2000, qualityLevel=0.2, minDistance=7, blockSize=7)
    assert lk.lk_params == dict(winSize=(21, 21), criteria=(3, 30, 0.01))
    assert callable(lk.get_features)

"""tests/lk_err_ref.py (the restatement of calcOpticalFlowPyrLK's err output, its two flags and the Harris score) against
tests/lk_ref.py where the two must agree, and against things it was not written from: the bound of the error sum, a construction whose
final positions leave the bounds, flat and step images.  No GPU."""
import numpy as np
import pytest

import gftt_pick_model as gm
import lk_err_cases as ec
import lk_err_ref as er
import lk_ref
import sparse_cases as sc
from test_lk_ref_cpu import blurred_noise

F = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- agreement with lk_ref ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.CASES, ids=sc.CASE_IDS)
def test_without_err_the_restatement_is_lk_ref(c):
    """flags = 0, want_err = False: out, status, histogram and exits of lk_ref.lk_track, on every track but the 65 536-point one"""
    for i, t in ec.tracks_of(c):
        pts, r_out, r_status, r_hist, r_exits = sc.reference(c.name, i)
        out, status, err, hist, exits, sums = ec.reference(c.name, i, 0, False)
        assert same(out, r_out) and same(status, r_status) and same(hist, r_hist), (c.name, t.label)
        assert exits.pop("outside-final") == 0 and exits == r_exits, (c.name, t.label)
        exits["outside-final"] = 0
        assert not err.any() and (sums == -1).all()


# ---- the error output -----------------------------------------------------------------------------------------------------------------
def test_error_sum_is_an_exact_float32():
    """the largest |J - I| is (255 * 16384 + 256) >> 9 = 8160, so S <= 8160 * 33 * 33 < 2^24: every S is a float32, and float32
    accumulation of the same terms is exact in any order"""
    top = (255 * (1 << lk_ref.W_BITS) + 256) >> 9
    assert top == 8160 and er.S_MAX_33 == top * 33 * 33 == 8_886_240 < 1 << 24
    flat0, flat255 = np.zeros((40, 40), np.uint8), np.full((40, 40), 255, np.uint8)
    pts = np.array([[20, 20], [19.5, 20.25]], F)
    out, status, err, hist, exits, sums = er.lk_track_err(flat0, flat255, pts, win=(33, 33), max_level=0, min_eig_threshold=-1, max_count=0,
                                                          want_sums=True)
    # a flat pair fails Dt < FLT_EPSILON whatever the threshold: status 0, no error
    assert not status.any() and not err.any() and (sums == -1).all()
    # the extreme reached: a textured previous frame that tracks, against itself, then the windows by hand
    a = blurred_noise(80, 80, 3)
    out, status, err, hist, exits, sums = er.lk_track_err(a, 255 - a, np.array([[40, 40]], F), win=(33, 33), max_level=0, max_count=0,
                                                          want_sums=True)
    assert status[0] == 1 and 0 < sums[0] <= er.S_MAX_33
    w = lk_ref._weights(np.zeros(1, F), np.zeros(1, F))
    Iw = lk_ref._window(a, np.array([24]), np.array([24]), (33, 33), w, 9, False)
    Jw = lk_ref._window(255 - a, np.array([24]), np.array([24]), (33, 33), w, 9, False)
    assert sums[0] == np.abs(Jw - Iw).sum() and err[0] == F(sums[0]) / F(32 * 33 * 33)


@pytest.mark.parametrize("W,H", ec.GPU_CASES)
def test_err_is_the_float32_quotient_of_its_sum(W, H):
    c = sc.case_of(W, H)
    seen = 0
    for i, t in ec.tracks_of(c):
        out, status, err, hist, exits, sums = ec.reference(c.name, i)
        has = sums >= 0
        assert np.array_equal(has, status == 1), t.label                       # a sum exactly for the points that end with status 1
        assert (sums[has] < 1 << 24).all() and np.array_equal(sums[has].astype(F).astype(np.int64), sums[has])
        assert same(err[has], sums[has].astype(F) / F(32 * t.win[0] * t.win[1])), t.label
        assert not err[~has].any(), t.label
        seen += int(has.sum())
        # the error pass touches neither the positions nor the histogram, and clears status only through the final test
        r_out, r_status, _, r_hist, r_exits, _ = ec.reference(c.name, i, 0, False)
        assert same(out, r_out) and same(hist, r_hist)
        assert int(r_status.sum()) - int(status.sum()) == exits["outside-final"] and not (status & ~r_status).any()
    assert seen > 0


# ---- the final bounds test ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift,max_level", ec.FINAL_RUNS)
def test_the_final_bounds_test_is_reached(shift, max_level):
    a, b = ec.final_frames(shift)
    pts = ec.final_points()
    assert pts.shape == (80, 2)
    r_out, r_status = lk_ref.lk_track(a, b, pts, max_level=max_level, **ec.FINAL_KW)
    out, status, err, hist, exits, sums = ec.final_reference(shift, max_level)
    # which of lk_ref's status-1 points end outside: stated from the positions alone
    q = r_out - F(10)
    fx, fy, ok = lk_ref._floor_in(q[:, 0], q[:, 1], ec.FINAL_WIN, ec.FINAL_W, ec.FINAL_H)
    outside = (r_status == 1) & ~ok
    print(f"shift {shift} max_level {max_level}: {int(r_status.sum())} at status 1, {int(outside.sum())} of them end outside")
    assert int(outside.sum()) == ec.FINAL_OUTSIDE[(shift, max_level)]
    assert exits["outside-final"] >= 1 and exits["outside-final"] == int(outside.sum())
    assert not status[outside].any() and not err[outside].any()
    assert same(out, r_out) and same(status[~outside], r_status[~outside])
    assert (err[status == 1] > 0).all() and not err[status == 0].any()


# ---- OPTFLOW_LK_GET_MIN_EIGENVALS -----------------------------------------------------------------------------------------------------
def level0_min_eig(a, pts, win):
    """(passes the first bounds test at level 0, its minEig) from lk_ref's pieces"""
    halfx, halfy = F((win[0] - 1) * 0.5), F((win[1] - 1) * 0.5)
    px, py = pts[:, 0] - halfx, pts[:, 1] - halfy
    fx, fy, ok = lk_ref._floor_in(px, py, win, a.shape[1], a.shape[0])
    sel = np.nonzero(ok)[0]
    val = np.zeros(len(pts), F)
    if len(sel):
        d = lk_ref.scharr(a)
        wts = lk_ref._weights(px[sel] - fx[sel], py[sel] - fy[sel])
        ix, iy = fx[sel].astype(np.int64), fy[sel].astype(np.int64)
        dx, dy = lk_ref._window(d[..., 0], ix, iy, win, wts, 14, True), lk_ref._window(d[..., 1], ix, iy, win, wts, 14, True)
        SC = F(1.0 / (1 << 20))
        A11, A12, A22 = ((p * q).sum(axis=(1, 2)).astype(F) * SC for p, q in ((dx, dx), (dx, dy), (dy, dy)))
        val[sel] = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win[0] * win[1])
    return ok, val


@pytest.mark.parametrize("W,H", [(17, 9), (43, 43), (320, 240)])
def test_min_eigenvalue_flag(W, H):
    c = sc.case_of(W, H)
    for i, t in ec.tracks_of(c):
        a, b = c.frames(t)
        pts = c.points(t)
        out, status, err, hist, exits, sums = ec.reference(c.name, i, er.GET_MIN_EIGENVALS)
        r_out, r_status, _, r_hist, r_exits, _ = ec.reference(c.name, i, 0, False)
        assert same(out, r_out) and same(status, r_status) and same(hist, r_hist) and exits == r_exits, t.label
        ok, val = level0_min_eig(a, pts, t.win)
        assert same(err, np.where(ok, val, F(0))), t.label
        assert (sums == -1).all()
        # without an err buffer the flag changes nothing
        quiet = er.lk_track_err(a, b, pts, flags=er.GET_MIN_EIGENVALS, want_err=False, **t.params())
        assert same(quiet[0], r_out) and same(quiet[1], r_status) and not quiet[2].any()
    # a point the threshold rejects at level 0 carries its eigenvalue all the same
    t = next(t for t in c.tracks if dict(t.kw).get("min_eig_threshold")) if (W, H) == (320, 240) else None
    if t is not None:
        out, status, err, *_ = ec.reference(c.name, c.tracks.index(t), er.GET_MIN_EIGENVALS)
        assert ((status == 0) & (err > 0)).any()


# ---- OPTFLOW_USE_INITIAL_FLOW ---------------------------------------------------------------------------------------------------------
def test_initial_flow():
    c = sc.case_of(161, 123)
    t = c.tracks[0]
    a, b = c.frames(t)
    pts = c.points(t)
    plain = ec.reference(c.name, 0)
    warm = er.lk_track_err(a, b, pts, next_pts0=pts, flags=er.USE_INITIAL_FLOW, **t.params())
    assert all(same(x, y) for x, y in zip(warm[:4], plain[:4])) and warm[4] == plain[4]
    # NaN and inf guesses: status 0, nothing indexed (numpy would raise on an index from them)
    guess = pts.copy()
    bad = np.arange(0, 60, 7)
    guess[bad[0::3], 0] = np.nan
    guess[bad[1::3], 1] = np.inf
    guess[bad[2::3]] = (-np.inf, np.nan)
    out, status, err, hist, exits = er.lk_track_err(a, b, pts, next_pts0=guess, flags=er.USE_INITIAL_FLOW, **t.params())
    assert plain[1][bad].all() and not status[bad].any() and not err[bad].any()
    rest = np.setdiff1d(np.arange(len(pts)), bad)
    assert same(out[rest], plain[0][rest]) and same(status[rest], plain[1][rest]) and same(err[rest], plain[2][rest])
    # a guess at the true motion of a large shift recovers what the cold start loses
    a2 = blurred_noise(161, 123, 3)
    b2 = np.roll(a2, 40, axis=1)
    p2 = sc.inside_points(161, 123, 40)
    p2 = p2[(p2[:, 0] > 30) & (p2[:, 0] < 90) & (p2[:, 1] > 30) & (p2[:, 1] < 93)]
    cold = er.lk_track_err(a2, b2, p2, max_level=0)
    hot = er.lk_track_err(a2, b2, p2, next_pts0=p2 + F((40, 0)), flags=er.USE_INITIAL_FLOW, max_level=0)
    d_hot = np.hypot(*(hot[0] - p2 - F((40, 0))).T)
    d_cold = np.hypot(*(cold[0] - p2 - F((40, 0))).T)
    assert len(p2) >= 5 and hot[1].all() and d_hot.max() < 0.05 and (d_cold[cold[1] == 1] > 1).all()
    assert hot[2].max() < cold[2][cold[1] == 1].min() if cold[1].any() else True


# ---- Harris -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", sc.BLOCK_SIZES)
def test_harris_finds_no_corner_on_a_flat_frame_or_an_edge(bs):
    flat = np.full((ec.STEP_H, ec.STEP_W), 200, np.uint8)
    r = er.harris_response(flat, bs, 0.04)
    assert r.dtype == F and not r.any()
    assert er.good_features_score(flat, block_size=bs, use_harris=True).shape == (0, 2)
    step = ec.step_image()
    r = er.harris_response(step, bs, 0.04)
    assert (r <= 0).all() and r.max() == 0 and r.min() < 0
    assert er.good_features_score(step, block_size=bs, use_harris=True).shape == (0, 2)
    assert er.good_features_score(step, mask=sc.mask_of(ec.STEP_W, ec.STEP_H), block_size=bs, use_harris=True, min_distance=1).shape == (0, 2)
    # the min-eigenvalue score agrees on both
    assert len(er.good_features_score(step, block_size=bs)) == 0


def test_harris_corners_on_a_texture():
    img = blurred_noise(161, 123, 3)
    h = er.good_features_score(img, use_harris=True, k=0.04)
    m = er.good_features_score(img)
    assert same(m, lk_ref.good_features(img))                         # use_harris = False is the min-eigenvalue detector
    assert (len(h), len(m)) == (20, 127) and not same(h, m[:len(h)])
    # the pick is the sequential rule on the same keys
    resp = er.harris_response(img, 7, 0.04)
    v, idx = gm.masked_candidates(resp, None, 0.2)
    assert same(h, gm.sequential(gm.keys_of(v, idx), 161, 2000, 7)) and (v > 0).all()
    # every corner is an interior local maximum above max * quality
    xs, ys = h[:, 0].astype(int), h[:, 1].astype(int)
    assert (resp[ys, xs] > F(np.float64(resp.max()) * 0.2)).all() and np.all(np.diff(resp[ys, xs]) <= 0)
    # mostly negative responses: k = 0.15 at block size 3
    r = er.harris_response(img, 3, 0.15)
    hh = er.good_features_score(img, block_size=3, use_harris=True, k=0.15)
    print(f"k=0.15 block 3: {(r < 0).mean():.3f} of the responses negative, {len(hh)} corners")
    assert (r < 0).mean() > 0.5 and len(hh) == 39
    # k is rounded to float32 once: the double product differs somewhere on this map
    a = er.harris_response(img, 7, 0.04)
    assert same(a, er.harris_response(img, 7, float(F(0.04))))


def test_harris_a_rectangle_has_four_corners():
    img = np.zeros((120, 160), np.uint8)
    img[40:80, 50:110] = 255
    pts = er.good_features_score(img, use_harris=True, block_size=3)
    assert len(pts) == 4
    for vx, vy in ((50, 40), (109, 40), (50, 79), (109, 79)):
        assert (np.hypot(pts[:, 0] - vx, pts[:, 1] - vy) <= 3).sum() == 1, (vx, vy, pts)

"""The tracker's `err` form (mav_lk_track_err, OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS), the Harris score
(mav_good_features_score, mav_stage_corner_response) and the cv2-signature shims of mavflow.lucas_kanade on the GPU against the numpy
restatement tests/lk_err_ref.py: EQUAL BYTES throughout, no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import lk_err_cases as ec
import lk_err_ref as er
import lk_ref
import sparse_cases as sc
from test_gpu_gftt_device import PATTERN, Outputs, untouched
from test_gpu_lk import same

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = {"win": "winSize", "max_level": "maxLevel"}


def cv_params(kw):
    return {NAMES.get(k, k): v for k, v in kw.items()}


def check_err_track(ctx, a, b, pts, ref, label, flags=0, next_pts=None, **kw):
    """out, status, err and the iteration histogram of one host call against the restatement's"""
    out, status, err = ctx.lk_track_err(a, b, pts, next_pts=next_pts, flags=flags, **cv_params(kw))
    r_out, r_status, r_err, r_hist = ref[:4]
    bad = np.nonzero((out.view(np.uint32) != r_out.view(np.uint32)).any(axis=1) | (status != r_status) | (err.view(np.uint32) != r_err.view(np.uint32)))[0]
    assert not len(bad), (label, len(bad), len(pts), [(pts[i].tolist(), out[i].tolist(), r_out[i].tolist(), int(status[i]), int(r_status[i]),
                                                      float(err[i]), float(r_err[i])) for i in bad[:5]])
    assert same(out, r_out) and same(status, r_status) and same(err, r_err), label
    assert same(ctx.lk_last_iterations(), r_hist), (label, ctx.lk_last_iterations()[:12], r_hist[:12])
    return out, status, err


class ErrOutputs(Outputs):
    """test_gpu_gftt_device.Outputs and an err buffer, all pre-filled with the sentinel"""

    def __init__(self, ctx, mc):
        self.err = ctx.alloc(mc * 4)
        super().__init__(ctx, mc)

    def fill(self):
        super().fill()
        self.err.upload(np.full(self.err.nbytes, PATTERN, np.uint8))

    def read_err(self):
        _, _, out, status = self.read()
        return out, status, self.err.download(F, (self.mc,))


# ---- 1. the tracker against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, er.GET_MIN_EIGENVALS], ids=["err", "min-eig"])
@pytest.mark.parametrize("W,H", ec.GPU_CASES, ids=[f"{w}x{h}" for w, h in ec.GPU_CASES])
def test_err_tracker_on_the_case_table(mav, W, H, flags):
    """every track of the case but the 65 536-point one: on 161 x 123 every window form and the point counts 1 and 61 .. 64, on
    320 x 240 the baseline tracks that take every exit"""
    from mavflow import _lib
    c = sc.case_of(W, H)
    if (W, H) == (161, 123):
        wins = {t.win for _, t in ec.tracks_of(c)}
        counts = {len(c.points(t)) for _, t in ec.tracks_of(c)}
        assert {(3, 3), (9, 9), (33, 33), (33, 5), (5, 33)} <= wins and {1, 61, 62, 63, 64} <= counts
    with _lib.Context(W, H, 1) as ctx:
        nonzero = 0
        for i, t in ec.tracks_of(c):
            a, b = c.frames(t)
            ref = ec.reference(c.name, i, flags)
            _, _, err = check_err_track(ctx, a, b, c.points(t), ref, (c.name, t.label, flags), flags=flags, **t.params())
            nonzero += int(np.count_nonzero(err))
        assert nonzero > 0


@pytest.mark.parametrize("shift,max_level", ec.FINAL_RUNS)
def test_the_final_bounds_test_clears_status(mav, shift, max_level):
    """points lk_track keeps at status 1 whose last position lies outside the bounds: status 0 and err 0 once err is asked for"""
    from mavflow import _lib
    a, b = ec.final_frames(shift)
    pts = ec.final_points()
    ref = ec.final_reference(shift, max_level)
    kw = dict(max_level=max_level, **ec.FINAL_KW)
    with _lib.Context(ec.FINAL_W, ec.FINAL_H, 1) as ctx:
        out, status, err = check_err_track(ctx, a, b, pts, ref, ("final", shift, max_level), **kw)
        p_out, p_status = ctx.lk_track(a, b, pts, **cv_params(kw))
        cleared = (p_status == 1) & (status == 0)
        assert int(cleared.sum()) == ref[4]["outside-final"] == ec.FINAL_OUTSIDE[(shift, max_level)] >= 1
        assert same(out, p_out) and not err[cleared].any() and same(status[~cleared], p_status[~cleared])
        # with the minimum-eigenvalue flag there is no final test
        check_err_track(ctx, a, b, pts, ec.final_reference(shift, max_level, er.GET_MIN_EIGENVALS), ("final", "min-eig"),
                        flags=er.GET_MIN_EIGENVALS, **kw)


# ---- 2. the plain form -----------------------------------------------------------------------------------------------------------------
def test_without_flags_and_err_it_is_mav_lk_track(mav):
    from mavflow import _lib
    c = sc.case_of(161, 123)
    with _lib.Context(c.W, c.H, 1) as ctx:
        for i, t in ec.tracks_of(c)[:3] + ec.tracks_of(c)[8:15]:
            a, b = c.frames(t)
            pts = np.ascontiguousarray(c.points(t))
            n = len(pts)
            p = _lib.lk_defaults(**cv_params(t.params()))
            out, status = np.full((n, 2), 7, F), np.full(n, 7, np.uint8)
            _lib.check(ctx.lib.mav_lk_track_err(ctx.h, _lib._ptr(a), _lib._ptr(b), _lib._ptr(pts), n, C.byref(p), 0, _lib._ptr(out), _lib._ptr(status),
                                                None))
            hist = ctx.lk_last_iterations()
            p_out, p_status = ctx.lk_track(a, b, pts, **cv_params(t.params()))
            assert same(out, p_out) and same(status, p_status) and same(hist, ctx.lk_last_iterations()), t.label
            # the minimum-eigenvalue flag without an err buffer changes nothing
            _lib.check(ctx.lib.mav_lk_track_err(ctx.h, _lib._ptr(a), _lib._ptr(b), _lib._ptr(pts), n, C.byref(p), er.GET_MIN_EIGENVALS, _lib._ptr(out),
                                                _lib._ptr(status), None))
            assert same(out, p_out) and same(status, p_status), t.label


# ---- 3. OPTFLOW_USE_INITIAL_FLOW -------------------------------------------------------------------------------------------------------
def test_initial_flow(mav):
    from mavflow import _lib
    from test_lk_ref_cpu import blurred_noise
    W, H = 161, 123
    c = sc.case_of(W, H)
    t = c.tracks[0]
    a, b = c.frames(t)
    pts = c.points(t)
    n = len(pts)
    plain = ec.reference(c.name, 0)
    with _lib.Context(W, H, 1) as ctx:
        # a guess equal to the points is the cold start
        check_err_track(ctx, a, b, pts, plain, "guess = pts", flags=er.USE_INITIAL_FLOW, next_pts=pts, **t.params())
        # NaN and inf guesses: status 0, no fault
        guess = pts.copy()
        bad = np.arange(0, 60, 7)
        guess[bad[0::3], 0] = np.nan
        guess[bad[1::3], 1] = np.inf
        guess[bad[2::3]] = (-np.inf, np.nan)
        ref = er.lk_track_err(a, b, pts, next_pts0=guess, flags=er.USE_INITIAL_FLOW, **t.params())
        _, status, _ = check_err_track(ctx, a, b, pts, ref, "non-finite guesses", flags=er.USE_INITIAL_FLOW, next_pts=guess, **t.params())
        assert not status[bad].any() and plain[1][bad].all()
        # both flags at once
        ref = er.lk_track_err(a, b, pts, next_pts0=guess, flags=er.USE_INITIAL_FLOW | er.GET_MIN_EIGENVALS, **t.params())
        check_err_track(ctx, a, b, pts, ref, "both flags", flags=er.USE_INITIAL_FLOW | er.GET_MIN_EIGENVALS, next_pts=guess, **t.params())
        # a guess at the true motion, 40 px, at level 0 alone
        a2 = blurred_noise(W, H, 3)
        b2 = np.roll(a2, 40, axis=1)
        p2 = sc.inside_points(W, H, 40)
        p2 = p2[(p2[:, 0] > 30) & (p2[:, 0] < 90) & (p2[:, 1] > 30) & (p2[:, 1] < 93)]
        g2 = p2 + F((40, 0))
        ref = er.lk_track_err(a2, b2, p2, next_pts0=g2, flags=er.USE_INITIAL_FLOW, max_level=0)
        out, status, _ = check_err_track(ctx, a2, b2, p2, ref, "true shift", flags=er.USE_INITIAL_FLOW, next_pts=g2, max_level=0)
        assert status.all() and np.hypot(*(out - g2).T).max() < 0.05
        # in place on the device: pts_dev == next_pts_dev, the guess being the points themselves; then without the flag
        da, db = ctx.alloc(W * H).upload(a), ctx.alloc(W * H).upload(b)
        o = ErrOutputs(ctx, n)
        for flags in (er.USE_INITIAL_FLOW, 0):
            o.fill()
            o.out.upload(pts)
            ctx.lk_track_err_enqueue(da.ptr, db.ptr, o.out.ptr, n, None, o.out.ptr, o.status.ptr, o.err.ptr, flags=flags, **cv_params(t.params()))
            out, status, err = o.read_err()
            assert same(out, plain[0]) and same(status, plain[1]) and same(err, plain[2]), flags
            assert same(ctx.lk_last_iterations(), plain[3])


# ---- 4. the count on the device --------------------------------------------------------------------------------------------------------
def test_device_count_leaves_the_rest_untouched(mav):
    from mavflow import _lib
    W, H = sc.N_DEV_FRAME
    c = sc.case_of(W, H)
    a, b = c.frames()
    room = max(max(m, n) for m, n in sc.N_DEV_CALLS)
    pts = np.concatenate([sc.inside_points(W, H, room - 15, seed=21), sc.border_points(W, H)[-15:]])
    order = np.roll(np.arange(room), 7)                     # the points outside the frame come first, so that every call sees some
    with _lib.Context(W, H, 1) as ctx:
        da, db = ctx.alloc(W * H).upload(a), ctx.alloc(W * H).upload(b)
        o = ErrOutputs(ctx, room)
        for n_dev, n_max in sc.N_DEV_CALLS:
            o.fill()
            o.corners.upload(pts[order])
            o.count.upload(np.array([n_dev], np.int32))
            ctx.lk_track_err_enqueue(da.ptr, db.ptr, o.corners.ptr, n_max, o.count.ptr, o.out.ptr, o.status.ptr, o.err.ptr)
            out, status, err = o.read_err()
            m = min(max(n_dev, 0), n_max)
            assert untouched(out, m) and untouched(status, m) and untouched(err, m), (n_dev, n_max)
            if m:
                r_out, r_status, r_err, r_hist, _ = er.lk_track_err(a, b, pts[order][:m])
                assert same(out[:m], r_out) and same(status[:m], r_status) and same(err[:m], r_err), (n_dev, n_max)
                assert same(ctx.lk_last_iterations(), r_hist), (n_dev, n_max)
                assert 0 < r_status.sum() < m and np.count_nonzero(r_err)
            else:
                assert ctx.lk_last_iterations().sum() == 0
        # no count on the device: n_max points run
        o.fill()
        o.corners.upload(pts[order])
        ctx.lk_track_err_enqueue(da.ptr, db.ptr, o.corners.ptr, 37, None, o.out.ptr, o.status.ptr, o.err.ptr)
        out, status, err = o.read_err()
        r_out, r_status, r_err, _, _ = er.lk_track_err(a, b, pts[order][:37])
        assert same(out[:37], r_out) and same(status[:37], r_status) and same(err[:37], r_err)
        assert untouched(out, 37) and untouched(status, 37) and untouched(err, 37)


# ---- 5. Harris -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ec.HARRIS_FRAMES, ids=[f"{w}x{h}" for w, h in ec.HARRIS_FRAMES])
def test_stage_corner_response(mav, W, H):
    from mavflow import _lib
    f = sc.frame(W, H)
    with _lib.Context(W, H, 1) as ctx:
        for kind, img in f.images().items():
            for bs in sc.BLOCK_SIZES:
                for k in ec.HARRIS_KS:
                    assert same(ctx.stage_corner_response(img, bs, True, k), ec.harris(kind, W, H, bs, k)), (kind, bs, k)
                plain = ctx.stage_min_eigen(img, bs)
                assert same(ctx.stage_corner_response(img, bs, False, 0.15), plain) and same(plain, sc.eigen(kind, W, H, bs)), (kind, bs)


def enqueue_corners(ctx, o, gray_ptr, mask_ptr, **kw):
    o.fill()
    ctx.good_features_enqueue(gray_ptr, o.corners.ptr, o.count.ptr, mask_ptr, max_corners=o.mc, **kw)
    corners, n, _, _ = o.read()
    assert n >= 0 and untouched(corners, n), "entries beyond the count were written"
    return corners[:n].copy()


@pytest.mark.parametrize("W,H", [(17, 9), (43, 41), (161, 123), (320, 240)])
def test_harris_corners_host_and_enqueue_forms(mav, W, H):
    from mavflow import _lib
    f = sc.frame(W, H)
    mask = sc.mask_of(W, H)
    total = 0
    with _lib.Context(W, H, 1) as ctx:
        o = Outputs(ctx, 2000)
        dmask = ctx.alloc(W * H).upload(mask)
        for kind in f.kinds[:3]:
            img = sc.image(kind, W, H)
            dev = ctx.alloc(W * H).upload(img)
            for bs, k, md in ((7, 0.04, 7), (3, 0.15, 2.5), (15, 0.04, 1)):
                kw = dict(block_size=bs, min_distance=md)
                for m, mp in ((None, None), (mask, dmask.ptr)):
                    ref = er.good_features_score(img, m, use_harris=True, k=k, **kw)
                    assert same(ctx.good_features(img, mask=m, useHarrisDetector=True, k=k, **kw), ref), (kind, bs, k, m is None, len(ref))
                    assert same(ctx.good_features(None, mask=m, useHarrisDetector=True, k=k, **kw), ref), (kind, "resident")
                    assert same(enqueue_corners(ctx, o, dev.ptr, mp, useHarrisDetector=True, k=k, **kw), ref), (kind, "enqueue")
                    total += len(ref)
                # use_harris = 0 through the score entry points is the existing detector
                sc0 = _lib.corner_score(False, k)
                p = _lib.gftt_defaults(**kw)
                out, n = np.empty((2000, 2), F), C.c_int()
                _lib.check(ctx.lib.mav_good_features_score(ctx.h, _lib._ptr(img), None, C.byref(p), C.byref(sc0), _lib._ptr(out), C.byref(n)))
                assert same(out[:n.value], ctx.good_features(img, **kw)), (kind, bs)
            dev.free()
    assert total > 0 or (W, H) == (17, 9)


def test_an_edge_is_no_harris_corner(mav):
    from mavflow import _lib
    step = ec.step_image()
    with _lib.Context(ec.STEP_W, ec.STEP_H, 1) as ctx:
        for bs in sc.BLOCK_SIZES:
            r = ctx.stage_corner_response(step, bs, True, 0.04)
            assert same(r, er.harris_response(step, bs, 0.04)) and r.max() == 0 and r.min() < 0
            got = ctx.good_features(step, useHarrisDetector=True, block_size=bs)
            assert got.shape == (0, 2) and got.dtype == np.float32
            assert ctx.good_features(np.full_like(step, 200), useHarrisDetector=True, block_size=bs).shape == (0, 2)


# ---- 6. the cv2-signature shims --------------------------------------------------------------------------------------------------------
def test_cv2_signature_shims(mav):
    from mavflow import lucas_kanade as lkm
    from mavflow.detector import LucasKanade
    assert lkm.LucasKanade is LucasKanade
    c = sc.case_of(161, 123)
    a, b = c.frames()
    corners = lkm.goodFeaturesToTrack(a, 2000, 0.2, 7, blockSize=7)
    assert corners.shape[1:] == (1, 2) and corners.dtype == np.float32
    assert same(corners.reshape(-1, 2), lk_ref.good_features(a))
    assert same(lkm.goodFeaturesToTrack(a, 50, 0.05, 3).reshape(-1, 2), lk_ref.good_features(a, 50, 0.05, 3, 3))       # cv2's default blockSize
    h = lkm.goodFeaturesToTrack(a, 2000, 0.2, 7, mask=sc.mask_of(161, 123), blockSize=7, useHarrisDetector=True, k=0.04)
    assert same(h.reshape(-1, 2), er.good_features_score(a, sc.mask_of(161, 123), use_harris=True))
    assert lkm.goodFeaturesToTrack(np.full((123, 161), 9, np.uint8), 100, 0.2, 7) is None
    assert lkm.goodFeaturesToTrack(ec.step_image(), 100, 0.2, 7, useHarrisDetector=True) is None
    with pytest.raises(ValueError, match="gradientSize"):
        lkm.goodFeaturesToTrack(a, 100, 0.2, 7, gradientSize=5)
    r_out, r_status, r_err, _, _ = er.lk_track_err(a, b, corners.reshape(-1, 2))
    for shape in ((-1, 1, 2), (-1, 2)):
        out, status, err = lkm.calcOpticalFlowPyrLK(a, b, corners.reshape(shape), None)
        assert out.shape == corners.reshape(shape).shape and status.shape == err.shape == (len(corners), 1)
        assert (out.dtype, status.dtype, err.dtype) == (np.float32, np.uint8, np.float32)
        assert same(out.reshape(-1, 2), r_out) and same(status[:, 0], r_status) and same(err[:, 0], r_err)
    kw = dict(winSize=(9, 9), maxLevel=2, criteria=(3, 10, 0.03), minEigThreshold=1e-3)
    ref = er.lk_track_err(a, b, corners.reshape(-1, 2), next_pts0=r_out, flags=4 | 8, win=(9, 9), max_level=2, max_count=10, epsilon=0.03,
                          min_eig_threshold=1e-3)
    out, status, err = lkm.calcOpticalFlowPyrLK(a, b, corners, r_out.reshape(-1, 1, 2), flags=lkm.OPTFLOW_USE_INITIAL_FLOW | lkm.OPTFLOW_LK_GET_MIN_EIGENVALS,
                                                **kw)
    assert same(out[:, 0], ref[0]) and same(status[:, 0], ref[1]) and same(err[:, 0], ref[2])
    with pytest.raises(ValueError):
        lkm.calcOpticalFlowPyrLK(a, b, corners, None, flags=lkm.OPTFLOW_USE_INITIAL_FLOW)
    with pytest.raises(ValueError):
        lkm.calcOpticalFlowPyrLK(a, b, corners.astype(np.float64), None)


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(mav):
    from mavflow import _lib
    import test_abi
    test_abi.test_library_exports_every_declared_symbol(mav)          # the new names on both sides: the header and EXPORTS
    W, H = 161, 123
    c = sc.case_of(W, H)
    a, b = c.frames()
    pts = c.points(c.tracks[0])
    n = len(pts)
    with _lib.Context(W, H, 1) as ctx:
        da, db = ctx.alloc(W * H).upload(a), ctx.alloc(W * H).upload(b)
        o = ErrOutputs(ctx, n)
        good = ctx.lk_track_err(a, b, pts)
        hist = ctx.lk_last_iterations()

        def nothing_ran():
            out, status, err = o.read_err()
            corners, count, _, _ = o.read()
            assert untouched(out, 0) and untouched(status, 0) and untouched(err, 0) and untouched(corners, 0) and count == 0xA5A5A5A5 - (1 << 32)
            assert same(ctx.lk_last_iterations(), hist)

        o.corners.upload(pts)
        p = _lib.lk_defaults()
        for flags in (1, 2, 16, 4 | 8 | 256, -1):
            with pytest.raises(ValueError, match="flags"):
                ctx.lk_track_err(a, b, pts, next_pts=pts, flags=flags)
            with pytest.raises(ValueError, match="flags"):
                ctx.lk_track_err_enqueue(da.ptr, db.ptr, o.corners.ptr, n, None, o.out.ptr, o.status.ptr, o.err.ptr, flags=flags)
        with pytest.raises(ValueError, match="next_pts"):
            ctx.lk_track_err(a, b, pts, flags=er.USE_INITIAL_FLOW)
        for fn, args in ((ctx.lib.mav_lk_track_err, (ctx.h, da.ptr, db.ptr, o.corners.ptr, n, C.byref(p), 4, None, o.status.ptr, o.err.ptr)),
                         (ctx.lib.mav_lk_track_err_dev, (ctx.h, da.ptr, db.ptr, o.corners.ptr, n, None, C.byref(p), 4, None, o.status.ptr, o.err.ptr))):
            assert fn(*args) == _lib.MAV_ERR_ARG and b"next_pts" in ctx.lib.mav_last_error()
        for k in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="k "):
                ctx.good_features(a, useHarrisDetector=True, k=k)
            with pytest.raises(ValueError, match="k "):
                ctx.good_features_enqueue(da.ptr, o.corners.ptr, o.count.ptr, useHarrisDetector=True, k=k)
            with pytest.raises(ValueError, match="k "):
                ctx.stage_corner_response(a, 7, True, k)
        o.fill()
        with pytest.raises(ValueError, match="flags"):
            ctx.lk_track_err_enqueue(da.ptr, db.ptr, o.corners.ptr, n, None, o.out.ptr, o.status.ptr, o.err.ptr, flags=32)
        with pytest.raises(ValueError, match="k "):
            ctx.good_features_enqueue(da.ptr, o.corners.ptr, o.count.ptr, useHarrisDetector=True, k=np.nan)
        nothing_ran()
        # and the context still works
        again = ctx.lk_track_err(a, b, pts)
        assert all(same(x, y) for x, y in zip(good, again))

"""The sparse optical-flow path on the GPU (mav_good_features / mav_lk_track and what the Python layer builds on them) against the CPU
restatement tests/lk_ref.py: EXACT equality throughout (the bytes).  Both keep every window sum in integers and do the same few
float32 operations in the same order, so there is no tolerance to argue about; a difference is a fused multiply-add, an approximate
sqrt / division or a sum that left the integers."""
import numpy as np
import pytest

import lk_ref
from test_lk_ref_cpu import blurred_noise

pytestmark = pytest.mark.gpu
F = np.float32
MB = 1 << 20


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def ref_track(a, b, pts, **kw):
    out, status, hist = lk_ref.lk_track(a, b, pts, want_hist=True, **kw)
    return out, status, hist


def check_track(ctx, a, b, pts, label, prev_resident=False, **kw):
    names = {"win": "winSize", "max_level": "maxLevel"}
    params = {names.get(k, k): v for k, v in kw.items()}
    out, status = ctx.lk_track(None if prev_resident else a, b, pts, **params)
    r_out, r_status, r_hist = ref_track(a, b, pts, **kw)
    bad = np.nonzero((out.view(np.uint32) != r_out.view(np.uint32)).any(axis=1) | (status != r_status))[0]
    assert not len(bad), (label, len(bad), len(pts), [(pts[i].tolist(), out[i].tolist(), r_out[i].tolist(), int(status[i]), int(r_status[i])) for i in bad[:5]])
    assert same(out, r_out) and same(status, r_status), label
    assert same(ctx.lk_last_iterations(), r_hist), (label, ctx.lk_last_iterations()[:12], r_hist[:12])
    return out, status


# ---- stage hooks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(161, 123), (320, 240), (640, 480), (1283, 721)])
def test_stage_hooks_are_exact(mav, W, H):
    from mavflow import _lib
    img = noise(W, H, W)
    img[H // 3:H // 2, W // 4:W // 2] = blurred_noise(W, H, 2)[H // 3:H // 2, W // 4:W // 2]      # a smooth region among the noise
    with _lib.Context(W, H, 1) as ctx:
        level, l = img, 0
        while True:
            assert ctx.lk_level_dims(l) == (level.shape[1], level.shape[0])
            assert same(ctx.stage_lk_pyramid(img, l), level), ("pyramid", l)
            assert same(ctx.stage_lk_scharr(img, l), lk_ref.scharr(level)), ("scharr", l)
            if l == _lib.LK_MAX_LEVEL or level.shape == (1, 1):
                break
            level, l = lk_ref.pyr_down(level), l + 1
        assert l >= 6
        with pytest.raises(ValueError):
            ctx.lk_level_dims(l + 1)
        for bs in (3, 7, 15):
            assert same(ctx.stage_min_eigen(img, bs), lk_ref.min_eigen(img, bs)), ("min_eigen", bs)
        with pytest.raises(ValueError, match="odd"):
            ctx.stage_min_eigen(img, 4)


# ---- corners -----------------------------------------------------------------------------------------------------------------------
def border_maximum_image(W, H):
    """Weak texture everywhere, one full-contrast checker at the top row: the eigenvalue map's maximum lies on row 0."""
    img = (blurred_noise(W, H, 4) // 8 + 100).astype(np.uint8)
    img[0:3, 100:103] = 255
    img[0:3, 103:106] = 0
    img[3:6, 100:103] = 0
    img[3:6, 103:106] = 255
    return img


def test_good_features_are_exact(mav):
    from mavflow import _lib, synth
    W, H = 320, 240
    images = {"synth0": synth.make_pair(W, H, 0)[0], "synth1": synth.make_pair(W, H, 1)[1], "blurred": blurred_noise(W, H, 3),
              "border": border_maximum_image(W, H)}
    eig = lk_ref.min_eigen(images["border"])
    assert np.unravel_index(np.argmax(eig), eig.shape)[0] == 0              # the case is what its name says
    with _lib.Context(W, H, 1) as ctx:
        for name, img in images.items():
            for mc in (1, 50, 2000):
                for md in (1, 7):
                    got = ctx.good_features(img, max_corners=mc, min_distance=md)
                    ref = lk_ref.good_features(img, max_corners=mc, min_distance=md)
                    assert same(got, ref), (name, mc, md, len(got), len(ref))
            assert len(ctx.good_features(img)) >= (1 if name == "border" else 100), name
        # other block sizes and quality levels, cv2's keyword names
        for bs, ql in ((3, 0.05), (5, 0.5), (15, 0.01)):
            assert same(ctx.good_features(images["blurred"], blockSize=bs, qualityLevel=ql),
                        lk_ref.good_features(images["blurred"], block_size=bs, quality_level=ql)), (bs, ql)
        # a flat image: no corner, no error
        for v in (0, 200):
            got = ctx.good_features(np.full((H, W), v, np.uint8))
            assert got.shape == (0, 2) and got.dtype == np.float32
        # the resident frame: the frame given last
        ref = lk_ref.good_features(images["synth0"])
        assert same(ctx.good_features(images["synth0"]), ref) and same(ctx.good_features(None), ref)


def test_good_features_on_the_larger_synthetic_pair(mav):
    from mavflow import _lib, synth
    W, H = 640, 480
    f0 = synth.make_pair(W, H, 0)[0]
    with _lib.Context(W, H, 1) as ctx:
        got = ctx.good_features(f0)
        assert len(got) == 2000 and same(got, lk_ref.good_features(f0))


def test_candidate_overflow_is_an_error_not_a_cut(mav):
    """A checkerboard of 2 x 2 squares is one local maximum per square corner: more candidates than the buffer holds."""
    from mavflow import _lib
    W, H = 1600, 1400
    yy, xx = np.mgrid[0:H, 0:W]
    img = ((((yy // 2) + (xx // 2)) & 1) * 255).astype(np.uint8)
    _, idx = lk_ref.corner_candidates(lk_ref.min_eigen(img), 0.2)
    assert len(idx) > _lib.GFTT_MAX_CANDIDATES
    with _lib.Context(W, H, 1) as ctx:
        with pytest.raises(ValueError, match=str(len(idx))):
            ctx.good_features(img)


# ---- tracker -----------------------------------------------------------------------------------------------------------------------
def planted_points(W, H):
    rng = np.random.default_rng(11)
    pts = [rng.random((60, 2)) * (W - 1, H - 1)]                                    # fractional coordinates anywhere
    for x0, x1, y0, y1 in ((0, 12, 0, H - 1), (W - 13, W - 1, 0, H - 1), (0, W - 1, 0, 12), (0, W - 1, H - 13, H - 1)):
        pts.append(np.stack([rng.uniform(x0, x1, 12), rng.uniform(y0, y1, 12)], axis=1))   # within a window of each border
    pts.append(np.array([[0, 0], [W - 1, H - 1], [W - 1, 0], [0.5, H - 1.5], [W / 2, H / 2], [W / 2 + 0.25, H / 2 + 0.75]]))
    pts.append(np.array([[-5.5, 20], [-11, -11], [-40, 50], [W + 9.9, 30], [W + 40, H + 40], [30, -10.01], [30, H + 10.2], [1e7, 5],
                         [-3e9, 4e9], [1e30, 1e30]]))                                # outside the image, near and far
    pts.append(np.array([[np.nan, 10], [10, np.nan], [np.nan, np.nan], [np.inf, 10], [10, -np.inf]]))
    return np.concatenate(pts).astype(F)


def test_lk_track_is_exact_on_detected_and_planted_points(mav):
    from mavflow import _lib, synth
    W, H = 320, 240
    f0, f1, _ = synth.make_pair(W, H, 0)
    flat0, flat1 = f0.copy(), f1.copy()
    flat0[60:140, 100:220] = 90                                  # a flat region: the min-eigenvalue test rejects points inside it
    flat1[60:140, 100:220] = 90
    with _lib.Context(W, H, 1) as ctx:
        with pytest.raises(_lib.MavflowError, match="resident"):
            ctx.lk_track(None, f1, np.zeros((1, 2), F))          # MAV_ERR_STATE on a fresh context
        with pytest.raises(_lib.MavflowError, match="resident"):
            ctx.good_features(None)
        corners = ctx.good_features(f0)
        out, status = check_track(ctx, f0, f1, corners, "corners")
        assert status.mean() > 0.98
        pts = planted_points(W, H)
        out, status = check_track(ctx, f0, f1, pts, "planted")
        assert status[-15:].sum() <= 5 and np.all(status[-5:] == 0) and 40 < status.sum() < len(pts)
        flat_pts = np.array([[160, 100], [150.5, 90.25], [101, 61], [160, 100.5]], F)
        out, status = check_track(ctx, flat0, flat1, np.concatenate([flat_pts, corners[:40]]), "flat")
        assert np.all(status[:2] == 0)
        # 40 px of motion: beyond the pyramid's reach, points run into maxCount
        far = np.roll(f0, (0, 40), axis=(0, 1))
        check_track(ctx, f0, far, corners[:200], "40 px")
        assert ctx.lk_last_iterations()[30] > 0
        # other windows and pyramid depths (5 is clamped by the size rule), a rectangular window, other criteria
        for kw in ({"win": (15, 15)}, {"win": (31, 31)}, {"max_level": 0}, {"max_level": 5}, {"win": (9, 33), "max_level": 2},
                   {"max_count": 3}, {"max_count": 0}, {"epsilon": 0.3}, {"min_eig_threshold": 0.05}, {"max_count": 1000, "epsilon": 0.0}):
            check_track(ctx, f0, f1, np.concatenate([corners[:150], pts[:100], pts[-20:]]), str(kw), **kw)
        assert ctx.lk_track(f0, f1, np.zeros((0, 2), F))[0].shape == (0, 2)
        with pytest.raises(ValueError, match="33"):
            ctx.lk_track(f0, f1, corners, winSize=(35, 35))
        with pytest.raises(ValueError):
            ctx.lk_track(f0, f1[:100], corners)


def test_the_resident_frame_is_the_previous_next(mav):
    from mavflow import _lib, synth
    W, H = 320, 240
    seq = synth.make_sequence(W, H, 4, seed=3)
    with _lib.Context(W, H, 1) as a, _lib.Context(W, H, 1) as b:
        pts = a.good_features(seq[0])
        pa, pb = pts, pts
        for i in range(3):
            na, sa = a.lk_track(seq[i] if i == 0 else None, seq[i + 1], pa)          # the video idiom: every frame goes up once
            nb, sb = b.lk_track(seq[i], seq[i + 1], pb)
            assert same(na, nb) and same(sa, sb), i
            assert same(a.good_features(None, max_corners=300), b.good_features(seq[i + 1], max_corners=300)), i
            pa, pb = na, nb
        r_out, r_status = lk_ref.lk_track(seq[2], seq[3], lk_ref.lk_track(seq[1], seq[2], lk_ref.lk_track(seq[0], seq[1], pts)[0])[0])
        assert same(pa, r_out) and same(sa, r_status)
        # a deeper pyramid than the resident frame was built with, a stage hook in between (it drops the resident frame)
        check_track(a, seq[3], seq[0], pts[:100], "deeper", prev_resident=True, win=(9, 9), max_level=5)
        a.stage_lk_pyramid(seq[0], 1)
        with pytest.raises(_lib.MavflowError, match="resident"):
            a.lk_track(None, seq[1], pts)


def test_full_size_frame_with_2000_points(mav):
    from mavflow import _lib, synth
    W, H = 1920, 1080
    f0, f1, _ = synth.make_pair(W, H, 0)
    with _lib.Context(W, H, 1) as ctx:
        corners = ctx.good_features(f0)
        assert len(corners) == 2000 and same(corners, lk_ref.good_features(f0))
        check_track(ctx, f0, f1, corners, "1080p", prev_resident=True)


def test_memory_comes_with_the_first_sparse_call(mav):
    from mavflow import _lib, synth
    W, H = 640, 480
    f0, f1, _ = synth.make_pair(W, H, 0)
    with _lib.Context(W, H, 1) as ctx:
        base = ctx.mem_info()
        ctx.bbox(f0)
        after_bbox = ctx.mem_info()
        pts = ctx.good_features(f0)
        m1 = ctx.mem_info()
        grown = m1["ctx_bytes"] - after_bbox["ctx_bytes"]
        print(f"sparse workspace at {W}x{H}: {grown / MB:.2f} MB")
        # two u8 pyramids, one int16-pair pyramid, the float32 eigenvalue map: 12 bytes per pixel; candidates and points: 3.2 MB
        assert 12 * W * H < grown < 12.2 * W * H + 4 * MB and m1["workspace_bytes"] == 0
        assert after_bbox["ctx_bytes"] - base["ctx_bytes"] < MB                      # nothing of it before the first sparse call
        ctx.lk_track(None, f1, pts)
        ctx.lk_track(None, f0, pts, winSize=(31, 31), maxLevel=5)
        assert ctx.mem_info()["ctx_bytes"] == m1["ctx_bytes"]                         # allocated once
        free_open = ctx.mem_info()["dev_free"]
    with _lib.Context(W, H, 1) as ctx:                                                # and given back by close()
        again = ctx.mem_info()
        assert again["ctx_bytes"] == base["ctx_bytes"]
        assert again["dev_free"] > free_open


# ---- the reference's classes -------------------------------------------------------------------------------------------------------
def bgr_of(gray, tint):
    """A BGR frame whose channels differ (so that the gray conversion matters)."""
    g = gray.astype(np.int32)
    return np.stack([np.clip(g + tint, 0, 255), g, np.clip(g - tint, 0, 255)], axis=-1).astype(np.uint8)


def ref_get_features(state, old_gray, frame_gray):
    """lucas_kanade.py:34-63 over lk_ref; state = {"features": list}."""
    if np.sum(old_gray) < 1:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    if len(state["features"]) < 666:
        state["features"] += list(lk_ref.good_features(old_gray))
    old = np.array(state["features"]).astype(F).reshape(-1, 2)
    new, status = lk_ref.lk_track(old_gray, frame_gray, old)
    state["features"] = new.tolist()
    return old, new, status.reshape(-1, 1)


def test_lucas_kanade_get_features_over_a_sequence(mav):
    from mavflow import _lib, synth
    from mavflow.detector import LucasKanade
    W, H = 320, 240
    seq = synth.make_sequence(W, H, 6, seed=1)
    frames = [bgr_of(g, 9) for g in seq]
    with _lib.Context(W, H, 1) as ctx:
        grays = [ctx.bgr2gray(f)[0] for f in frames]
    lk = LucasKanade(np.zeros((H, W, 3), np.uint8))
    o, n, s = lk.get_features(frames[0])                          # all-black previous frame: three empty arrays
    assert o.shape == n.shape == s.shape == (0,) and lk.features == [] and lk.old_frame is frames[0]
    state = {"features": []}
    for i in range(1, 6):
        if i == 4:                                                # most features lost: the next call re-detects and APPENDS
            lk.features = lk.features[:500]
            state["features"] = state["features"][:500]
            kept = np.array(lk.features, F)
        o, n, s = lk.get_features(frames[i])
        ro, rn, rs = ref_get_features(state, grays[i - 1], grays[i])
        assert same(o, ro) and same(n, rn) and same(s, rs), i
        assert o.dtype == np.float32 and o.ndim == 2 and s.shape == (len(o), 1) and s.dtype == np.uint8
        assert lk.features == state["features"] and lk.old_frame is frames[i]
        if i == 4:
            assert len(o) > 666 and same(o[:500], kept)
    # a previous frame the context does not hold (old_frame replaced by the caller) is uploaded again
    lk.old_frame = frames[2].copy()
    state_old = grays[2]
    o, n, s = lk.get_features(frames[3])
    ro, rn, rs = ref_get_features(state, state_old, grays[3])
    assert same(o, ro) and same(n, rn) and same(s, rs)


def ref_ransac(est, thr=30.0):
    best, foe = 0, (0.0, 0.0)
    for i in range(len(est)):
        score = int((np.linalg.norm(est - est[i], axis=-1) < thr).sum()) - 1
        if score > best:
            best, foe = score, (float(est[i, 0]), float(est[i, 1]))
    return foe


def ref_foe_sparse(trace, state, old_gray, new_gray, width, roll_back=20):
    """focus_of_expansion.py:88-148 on the host over lk_ref (the frames are never all black here)."""
    from mavflow import utils
    old_features, new_features, status = ref_get_features(state, old_gray, new_gray)
    lines = []
    inter = np.zeros((len(new_features), 2))
    u16 = lambda v: (np.trunc(v).astype(np.int64) & 0xFFFF).astype(np.uint16)
    for i, (new, old) in enumerate(zip(new_features, old_features)):
        if status[i] != 1:
            continue
        c, d = int(old[0]), int(old[1])
        l = trace[i, 0] + 1
        trace[i, l], trace[i, l + 1] = c, d
        trace[i, 0] += 2
        if l >= 3:
            k = 1 if l < 1 + roll_back * 2 else l - roll_back * 2
            a, b = trace[i, l:l + 2]
            c, d = trace[i, k:k + 2]
            diff = np.array([float(c) - float(a), float(d) - float(b)])
            xy = u16(np.array([a, b]) + diff)
            while (xy[1] < 0.0 or xy[1] > width) and diff.any():
                diff /= 2.0
                xy = u16(np.array([a, b]) + diff)
            lines.append(((a, b), (xy[0], xy[1])))
    with np.errstate(over="ignore"):
        for i, line_a in enumerate(lines):
            inter[i, :] = utils.line_intersection(line_a, lines[np.random.randint(0, len(lines))])
    return ref_ransac(inter[inter[:, 0] != 0.0, :]), len(lines)


def test_get_foe_sparse_over_a_sequence(mav):
    from mavflow import _lib, synth
    from mavflow.detector import LucasKanade
    from mavflow.focus_of_expansion import FocusOfExpansion
    W, H = 320, 240
    seq = synth.make_sequence(W, H, 6, seed=2)
    frames = [bgr_of(g, 5) for g in seq]
    with _lib.Context(W, H, 1) as ctx:
        grays = [ctx.bgr2gray(f)[0] for f in frames]
    np.random.seed(5)
    lk = LucasKanade(frames[0])
    foe = FocusOfExpansion(lk)
    assert foe.get_FOE_sparse(np.zeros((H, W, 3), np.uint8), frames[1]) == (np.nan, np.nan)       # black old frame: nothing is touched
    got = [foe.get_FOE_sparse(frames[i - 1], frames[i]) for i in range(1, 6)]
    end_state = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    np.random.randint(0, 255, (2666, 3)); np.random.randint(0, 255, (2666, 3)); np.random.randint(0, 2666, 2666)   # the constructors' draws
    trace, state, ref = np.zeros((2666, 2000), np.int32), {"features": []}, []
    n_lines = 0
    for i in range(1, 6):
        f, n_lines = ref_foe_sparse(trace, state, grays[i - 1], grays[i], W)
        ref.append(f)
    assert np.random.randint(0, 1 << 30) == end_state                                             # the RNG is left in the same state
    assert got == ref, (got, ref)
    assert n_lines > 300 and np.array_equal(foe.trace, trace) and len(foe.lines) == n_lines
    assert got[0] == (0.0, 0.0) and got[-1] != (0.0, 0.0)         # first call: every trace has one point, no line yet

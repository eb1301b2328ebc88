"""Every kernel of the sparse path (csrc/kernels_lk.hip) at every case of tests/sparse_cases.py against the numpy restatement
(tests/lk_ref.py, tests/gftt_pick_model.py): EQUAL BYTES throughout -- no tolerance, no point, pixel or case set aside.  What the
cases are and which kernel form each reaches is checked without a GPU by tests/test_sparse_cases_cpu.py."""
import numpy as np
import pytest

import gftt_pick_model as gm
import lk_ref
import sparse_cases as sc
from test_gpu_gftt_device import Outputs, untouched
from test_gpu_lk import check_track, same

pytestmark = pytest.mark.gpu
F = np.float32


def corners_of(idx, W):
    idx = np.asarray(idx, np.int64)[:sc.MAX_POINTS]
    return np.stack([idx % W, idx // W], axis=1).astype(F)


# ---- stage hooks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sc.FRAMES, ids=sc.FRAME_IDS)
def test_stage_hooks_on_every_frame(mav, f):
    from mavflow import _lib
    dims = sc.level_dims(f.W, f.H)
    with _lib.Context(f.W, f.H, 1) as ctx:
        for l, d in enumerate(dims):
            assert ctx.lk_level_dims(l) == d, l
        with pytest.raises(ValueError):
            ctx.lk_level_dims(len(dims))
        for kind, img in f.images().items():
            level = img
            for l in range(len(dims)):
                assert same(ctx.stage_lk_pyramid(img, l), level), (kind, "pyramid", l)
                assert same(ctx.stage_lk_scharr(img, l), lk_ref.scharr(level)), (kind, "scharr", l)
                level = lk_ref.pyr_down(level)
            for bs in sc.BLOCK_SIZES:
                assert same(ctx.stage_min_eigen(img, bs), sc.eigen(kind, f.W, f.H, bs)), (kind, "min_eigen", bs)


# ---- candidates as a set, both mask forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sc.FRAMES, ids=sc.FRAME_IDS)
def test_candidates_as_a_set(mav, f):
    """max_corners at the buffer's size and min_distance 0: every candidate, in key order (value descending, ties by index descending)"""
    from mavflow import _lib
    mask = sc.mask_of(f.W, f.H)
    with _lib.Context(f.W, f.H, 1) as ctx:
        for kind, img in f.images().items():
            v, idx = sc.candidates(kind, f.W, f.H)
            got = ctx.good_features(img, max_corners=sc.MAX_POINTS, min_distance=0)
            assert same(got, corners_of(idx, f.W)), (kind, len(got), len(idx))
            if not len(idx):
                assert got.shape == (0, 2) and got.dtype == np.float32
            for m in (mask, np.zeros_like(mask)):
                mv, midx = gm.masked_candidates(sc.eigen(kind, f.W, f.H), m)
                got = ctx.good_features(img, mask=m, max_corners=sc.MAX_POINTS, min_distance=0)
                assert same(got, corners_of(midx, f.W)), (kind, "mask", len(got), len(midx))
                assert same(ctx.good_features(None, mask=m, max_corners=sc.MAX_POINTS, min_distance=0), got), (kind, "resident")
            # other block sizes: the candidates of another map
            for bs in (1, 15):
                v2, idx2 = lk_ref.corner_candidates(sc.eigen(kind, f.W, f.H, bs))
                assert same(ctx.good_features(img, max_corners=sc.MAX_POINTS, min_distance=0, block_size=bs), corners_of(idx2, f.W)), (kind, bs)


# ---- corners ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sc.FRAMES, ids=sc.FRAME_IDS)
def test_corners_on_every_frame(mav, f):
    """the defaults and other minimum distances; gm.sequential over lk_ref's candidates is lk_ref.good_features's loop
    (tests/test_sparse_cases_cpu.py test_the_pick_model_is_lk_refs_loop)"""
    from mavflow import _lib
    mask = sc.mask_of(f.W, f.H)
    with _lib.Context(f.W, f.H, 1) as ctx:
        for kind, img in f.images().items():
            v, idx = sc.candidates(kind, f.W, f.H)
            keys = gm.keys_of(v, idx)
            ref = gm.sequential(keys, f.W, 2000, 7)
            got = ctx.good_features(img)
            assert same(got, ref), (kind, len(got), len(ref))
            if not len(idx):
                assert got.shape == (0, 2) and got.dtype == np.float32            # no corner, no error
            for md in sc.MIN_DISTANCES:
                got = ctx.good_features(None, min_distance=md)
                assert same(got, gm.sequential(keys, f.W, 2000, md)), (kind, md, len(got))
            mv, midx = gm.masked_candidates(sc.eigen(kind, f.W, f.H), mask)
            assert same(ctx.good_features(img, mask=mask, min_distance=2.5), gm.sequential(gm.keys_of(mv, midx), f.W, 2000, 2.5)), (kind, "mask")


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.CASES, ids=sc.CASE_IDS)
def test_tracker_on_every_case(mav, c):
    """points, status and the iteration histogram over every window, level count, point count and coordinate target of the case"""
    from mavflow import _lib
    with _lib.Context(c.W, c.H, 1) as ctx:
        for t in c.tracks:
            a, b = c.frames(t)
            out, status = check_track(ctx, a, b, c.points(t), (c.name, t.label), **t.params())
            if t.points == "coords":
                # the claims hold at level 0 whatever the coarser levels did: a point outside there has status 0
                labels = sc.coord_points(c.W, c.H, t.win)[0]
                claims = sc.coord_claims(c.W, c.H, t.win)
                for i, l in enumerate(labels):
                    assert claims[l] == "in" or status[i] == 0, (c.name, t.label, l)


# ---- the enqueue-only forms ------------------------------------------------------------------------------------------------------------
def test_enqueue_only_forms_on_a_ragged_frame(mav):
    """mav_lk_track_ex_dev with the count on the device below, above and equal to n_max, and negative: min(count, n_max) points are
    tracked, nothing beyond them is written"""
    from mavflow import _lib
    W, H = sc.N_DEV_FRAME
    c = sc.case_of(W, H)
    a, b = c.frames()
    room = max(max(m, n) for m, n in sc.N_DEV_CALLS)
    pts = np.concatenate([sc.inside_points(W, H, room - 15, seed=21), sc.border_points(W, H)[-15:]])
    with _lib.Context(W, H, 1) as ctx:
        da, db = ctx.alloc(W * H).upload(a), ctx.alloc(W * H).upload(b)
        o = Outputs(ctx, room)
        for n_dev, n_max in sc.N_DEV_CALLS:
            # the points that run: those outside the frame come first, so that every call sees some
            order = np.roll(np.arange(room), 7)
            o.fill()
            o.corners.upload(pts[order])
            o.count.upload(np.array([n_dev], np.int32))
            ctx.lk_track_enqueue(da.ptr, db.ptr, o.corners.ptr, n_max, o.count.ptr, o.out.ptr, o.status.ptr)
            _, _, out, status = o.read()
            m = min(max(n_dev, 0), n_max)
            assert untouched(out, m) and untouched(status, m), (n_dev, n_max)
            if m:
                r_out, r_status, r_hist = lk_ref.lk_track(a, b, pts[order][:m], want_hist=True)
                assert same(out[:m], r_out) and same(status[:m], r_status), (n_dev, n_max)
                assert same(ctx.lk_last_iterations(), r_hist), (n_dev, n_max)
                assert 0 < r_status.sum() < m
            else:
                assert ctx.lk_last_iterations().sum() == 0

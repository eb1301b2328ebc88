"""Every kernel of the window search (csrc/kernels_window.hip) at every case of tests/window_cases.py against
oracle/pyramid_oracle.py: bit for bit -- no tolerance, no pixel, window or case set aside.  What the cases are and which kernel form
each reaches is checked without a GPU by tests/test_window_cases_cpu.py."""
import numpy as np
import pytest

import window_cases as wc
from oracle import pyramid_oracle as po
from test_gpu_lk import same

pytestmark = pytest.mark.gpu
OPT_BATCH = 8


@pytest.mark.parametrize("c", wc.CASES, ids=wc.CASE_IDS)
def test_pyramid_levels_on_every_case(mav, c):
    from mavflow import _lib
    with _lib.Context(c.W, c.H, 1) as ctx:
        assert ctx.pyramid_dims() == c.dims()
        for kind in c.kinds:
            img = wc.image(kind, c.W, c.H)
            for l, exp in enumerate(wc.levels(kind, c.W, c.H)):
                assert same(ctx.pyramid_level(img, l), exp), (kind, l)
        with pytest.raises(ValueError):
            ctx.pyramid_level(wc.image(c.kinds[0], c.W, c.H), len(c.dims()))


@pytest.mark.parametrize("c", wc.CASES, ids=wc.CASE_IDS)
def test_analyze_pyramid_and_window_max_on_every_case(mav, c):
    """the batch in the case's order (a coarser level wins in a pair b > 0), then every image alone"""
    from mavflow import _lib
    imgs = c.batch()
    B = len(c.kinds)
    exp = np.array([wc.analysis(k, c.W, c.H)[0] for k in c.kinds], np.int64)
    exp_wm = np.array([wc.window_max_reference(k, c.W, c.H) for k in c.kinds], np.int64)
    with _lib.Context(c.W, c.H, B) as ctx:
        got = ctx.analyze_pyramid(imgs)
        assert same(got, exp), (got.tolist(), exp.tolist())
        wm = ctx.window_max(imgs)
        assert same(wm, exp_wm), (wm.tolist(), exp_wm.tolist())
        for b in reversed(range(B)):
            assert same(ctx.analyze_pyramid(imgs[b]), exp[b:b + 1]), c.kinds[b]
            assert same(ctx.window_max(imgs[b]), exp_wm[b:b + 1]), c.kinds[b]
    for b, kind in enumerate(c.kinds):
        if kind == "uniform" and exp[b, 0]:
            assert tuple(exp[b]) == (3 * 64 * 64 * 255, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("c", [c for c in wc.CASES if c.opt], ids=[c.name for c in wc.CASES if c.opt])
def test_optimize_window_on_every_case(mav, c):
    """every start window on every image, in batches (each pair its own image and window) and one at a time"""
    from mavflow import _lib
    pairs = wc.opt_pairs(c)
    starts = wc.start_windows(c.W, c.H)
    with _lib.Context(c.W, c.H, OPT_BATCH) as ctx:
        for i in range(0, len(pairs), OPT_BATCH):
            chunk = pairs[i:i + OPT_BATCH]
            imgs = np.stack([wc.image(k, c.W, c.H) for k, _ in chunk])
            wins = np.array([starts[s] for _, s in chunk], np.int32)
            score, out = ctx.optimize_window(imgs, wins)
            for j, (kind, start) in enumerate(chunk):
                es, ew = po.optimize_window(wc.image(kind, c.W, c.H), starts[start])
                assert (int(score[j]), tuple(int(v) for v in out[j])) == (es, ew), (kind, start, int(score[j]), out[j].tolist(), es, ew)
        kind, start = pairs[-1]
        score, out = ctx.optimize_window(wc.image(kind, c.W, c.H), [starts[start]])
        assert (int(score[0]), tuple(int(v) for v in out[0])) == po.optimize_window(wc.image(kind, c.W, c.H), starts[start])
        assert score.dtype == np.int64 and out.dtype == np.int32

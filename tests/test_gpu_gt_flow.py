"""mav_gt_flow on the device (csrc/kernels_truth.hip: k_gt_flow) held to tests/truth_ref.py and to the reference's own arrays
(tests/golden/truth.npz) by bytes, NaN by position (the library stores THE quiet NaN), for both output depths, on every case of
tests/truth_cases.py: host form against device form, every pair of a batch against the same pair run alone, two runs against each other,
and the float32 depth factor against a depth multiplied beforehand."""
import os

import numpy as np
import pytest

import truth_cases as T
import truth_ref as R

pytestmark = pytest.mark.gpu
GUARD = 256                    # canary bytes kept on both sides of a caller's output
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truth.npz")
QNAN = {np.dtype(np.float32): 0x7FC00000, np.dtype(np.float64): 0x7FF8000000000000}


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN, allow_pickle=False)


def _want(x, dtype):
    with np.errstate(all="ignore"):
        return x["ref64"].astype(dtype)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not R.same_bits(got, want):
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError((what, len(bad), "first differing element", bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert (got.view(u)[np.isnan(got)] == QNAN[got.dtype]).all(), (what, "a NaN that is not the canonical quiet NaN")


def _host(ctx, x, dtype):
    return ctx.gt_flow(x["depth"], x["seg"], x["vp1"], x["vp2"], x["disp"], depth_scale=x["scale"], dtype=dtype, view_proj_inv=x["inv"])


def _dev(ctx, x, dtype):
    """the enqueue-only form into the caller's own guarded buffer"""
    from mavflow import _truth
    B, H, W = x["depth"].shape
    p = _truth.gt_flow_params(x["vp1"], x["inv"], x["disp"], x["scale"], B)
    nbytes = B * H * W * 2 * np.dtype(dtype).itemsize
    bufs = [ctx.alloc(x["depth"].nbytes).upload(x["depth"]), ctx.alloc(p.nbytes).upload(p), ctx.alloc(nbytes + 2 * GUARD)]
    seg = ctx.alloc(x["seg"].nbytes).upload(x["seg"]) if x["seg"] is not None else None
    try:
        bufs[2].upload(np.full(nbytes + 2 * GUARD, 0x5A, np.uint8))
        ctx.gt_flow_enqueue(bufs[0], seg, bufs[1], B, bufs[2].ptr + GUARD, dtype=dtype)
        back = bufs[2].download(np.uint8, (nbytes + 2 * GUARD,))
        assert (back[:GUARD] == 0x5A).all() and (back[GUARD + nbytes:] == 0x5A).all(), "wrote outside its output"
        return back[GUARD:GUARD + nbytes].copy().view(dtype).reshape(B, H, W, 2)
    finally:
        for b in bufs + ([seg] if seg is not None else []):
            b.free()


@pytest.mark.parametrize("name", [c.name for c in T.GT_CASES])
def test_device_equals_the_restatement_in_both_forms_and_depths(name):
    from mavflow import _lib
    c = {k.name: k for k in T.GT_CASES}[name]
    x = T.gt_inputs(name)
    with _lib.Context(c.W, c.H, c.B) as ctx:
        for dtype in (np.float32, np.float64):
            want = _want(x, dtype)
            host = _host(ctx, x, dtype)
            _same(host, want, (name, np.dtype(dtype).name, "host form"))
            dev = _dev(ctx, x, dtype)
            _same(dev, want, (name, np.dtype(dtype).name, "device form"))
            assert dev.tobytes() == host.tobytes()
            assert _dev(ctx, x, dtype).tobytes() == dev.tobytes(), "two runs differ"


def test_device_equals_the_references_own_arrays(g):
    from mavflow import _lib
    for name in g["cases"]:
        x = T.fixture_inputs(g, str(name))
        B, H, W = x["depth"].shape
        with _lib.Context(W, H, 1) as ctx:
            for dtype in (np.float32, np.float64):
                _same(_host(ctx, x, dtype), _want(x, dtype), (str(name), np.dtype(dtype).name))
            # the binding inverts the second matrix itself, as calculate_flow does
            got = ctx.gt_flow(x["depth"][0], x["seg"][0], x["vp1"][0], x["vp2"][0], x["disp"][0], depth_scale=x["scale"], dtype=np.float64)
            _same(got, x["ref64"][0], (str(name), "inverse taken by the binding"))
    w = T.fixture_inputs(g, "wcross")["ref64"]
    assert np.isinf(w).any() and np.isnan(w).any()


def test_each_pair_of_a_batch_equals_the_pair_alone():
    from mavflow import _lib
    c = {k.name: k for k in T.GT_CASES}["batch 3"]
    x = T.gt_inputs("batch 3")
    with _lib.Context(c.W, c.H, c.B) as ctx:
        both = {dt: _host(ctx, x, dt) for dt in (np.float32, np.float64)}
        for b in range(c.B):
            one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in x.items()}
            for dt in (np.float32, np.float64):
                assert _host(ctx, one, dt).tobytes() == both[dt][b:b + 1].tobytes(), (b, dt)
        assert both[np.float32][0].tobytes() != both[np.float32][1].tobytes()


def test_depth_scale_is_the_float32_product():
    from mavflow import _lib
    c = {k.name: k for k in T.GT_CASES}["97x71"]
    x = T.gt_inputs("97x71")
    assert x["scale"] == 100.0
    pre = dict(x, depth=x["depth"] * np.float32(100), scale=1.0)
    with _lib.Context(c.W, c.H, 1) as ctx:
        for dt in (np.float32, np.float64):
            assert _host(ctx, pre, dt).tobytes() == _host(ctx, x, dt).tobytes()


def test_refusals_with_a_context():
    from mavflow import _lib, _truth
    x = T.gt_inputs("5x3")
    with _lib.Context(5, 3, 1) as ctx:
        two = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in x.items()}
        with pytest.raises(ValueError, match="mav_gt_flow: batch 2"):
            _host(ctx, two, np.float32)                                     # above the context's max_batch
        with pytest.raises(TypeError):
            ctx.gt_flow(x["depth"].astype(np.float64), None, x["vp1"], x["vp2"], x["disp"])
        assert _host(ctx, x, np.float32).shape == (1, 3, 5, 2)             # and the context is as usable as before

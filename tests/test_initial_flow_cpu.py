"""OPTFLOW_USE_INITIAL_FLOW on the CPU side: the checker (tests/initial_flow_ref.py) against the oracle it is built from, its INTER_AREA
restatement against what an area average must give, and the constants of the boundary."""
import os
import re

import numpy as np
import pytest

import initial_flow_ref as ref
from oracle import fb_oracle as fbo
from oracle import pyramid_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size,params", [((640, 480), fbo.Params(0.4, 1, 12, 10, 8, 1.2, 0)),
                                         ((640, 480), fbo.Params(0.5, 1, 12, 10, 8, 1.2, 0)),
                                         ((333, 227), fbo.Params(0.4, 0, 12, 10, 8, 1.2, 0))])
def test_checker_with_a_zero_initial_flow_is_the_oracle(fb_oracle, size, params):
    """An all-zero flow0 is the flags = 0 computation: bit for bit, for the fast-area ratio, the general one and levels = 0."""
    from mavflow import synth
    W, H = size
    f0, f1, _ = synth.make_pair(W, H, 1)
    got = ref.calc_init(fb_oracle, f0, f1, np.zeros((H, W, 2), np.float32), params)
    assert np.array_equal(got, fb_oracle.calc(f0, f1, params))


def test_ratio_paths_are_the_ones_opencv_takes(fb_oracle):
    """pyr_scale 0.5 at 640x480: layer 1 is 320x240, ratio 2 on both axes (fast-area path); the default 0.4 gives 256x192, ratio 2.5
    (general path)."""
    W, H = 640, 480
    assert fb_oracle.layer_dims(W, H, fbo.Params(0.5, 1, 12, 10, 8, 1.2, 0), 1)[:2] == (320, 240)
    assert ref.area_ratio(W, 320)[1:] == (2, True) and ref.area_ratio(H, 240)[1:] == (2, True)
    assert fb_oracle.layer_dims(W, H, fbo.Params(0.4, 1, 12, 10, 8, 1.2, 0), 1)[:2] == (256, 192)
    assert not ref.area_ratio(W, 256)[2] and ref.area_ratio(W, 256)[0] == 2.5


@pytest.mark.parametrize("src,dst,ulps", [((640, 480), (256, 192), 1), ((1920, 1080), (768, 432), 1), ((640, 480), (320, 240), 1),
                                          # ragged ratios: the float weights of a cell do not sum to 1 exactly, one rounding per tap
                                          ((333, 227), (133, 91), 6), ((3840, 2160), (98, 55), 80)])
def test_area_resize_of_a_constant_field_is_constant(src, dst, ulps):
    W, H = src
    w, h = dst
    for c in (np.array([3.7, -11.25], np.float32), np.array([0.3, 1e-3], np.float32)):
        out = ref.resize_area_flow(np.broadcast_to(c, (H, W, 2)).copy(), w, h)
        for ch in range(2):
            err = np.abs(out[..., ch] - c[ch]).max() / np.spacing(np.abs(c[ch]))
            assert err <= ulps, (ch, err)


def _coverage_centre(S, d):
    """Where an area mean puts a linear ramp: pixel i stands for [i, i + 1) with the value at i; destination index d covers
    [d * S/d', (d + 1) * S/d') of the source.  The coverage-weighted mean of i, in double, computed straight from the overlaps."""
    s = 1.0 / (d / S)
    lo = np.arange(d)[:, None] * s
    hi = np.minimum(lo + s, S)
    i = np.arange(S)[None, :]
    cov = np.clip(np.minimum(hi, i + 1) - np.maximum(lo, i), 0, None)
    return (cov * i).sum(1) / cov.sum(1)


@pytest.mark.parametrize("src,dst", [((640, 480), (256, 192)), ((640, 480), (320, 240)), ((333, 227), (133, 91))])
def test_area_resize_of_a_ramp_samples_it_at_the_cell_centres(src, dst):
    """An area mean of a linear field is its value at the centre of the cell's coverage -- (d + 0.5) * scale - 0.5 for a whole ratio,
    within 0.05 px of it for 2.5 (a cell that starts or ends half way into a pixel weights that pixel's value by its half)."""
    W, H = src
    w, h = dst
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    f = np.stack([0.01 * x - 0.02 * y, -0.015 * x + 0.005 * y], -1).astype(np.float32)
    out = ref.resize_area_flow(f, w, h)
    cx, cy = _coverage_centre(W, w), _coverage_centre(H, h)
    if W % w == 0 and H % h == 0:
        assert np.array_equal(cx, (np.arange(w) + 0.5) * (W // w) - 0.5) and np.array_equal(cy, (np.arange(h) + 0.5) * (H // h) - 0.5)
    X, Y = np.meshgrid(cx, cy)
    exp = np.stack([0.01 * X - 0.02 * Y, -0.015 * X + 0.005 * Y], -1)
    assert np.abs(out - exp).max() <= 1e-5, np.abs(out - exp).max()


def test_area_resize_by_two_is_the_block_mean():
    rng = np.random.default_rng(0)
    f = rng.normal(0, 4, (480, 640, 2)).astype(np.float32)
    out = ref.resize_area_flow(f, 320, 240)
    blocks = f.astype(np.float64).reshape(240, 2, 320, 2, 2).mean(axis=(1, 3))
    assert np.abs(out - blocks).max() <= 4 * np.spacing(np.float32(16))
    # ... and the exact float order: ((a + b) + c) + d, times 0.25f
    a, b, c, d = f[0::2, 0::2], f[0::2, 1::2], f[1::2, 0::2], f[1::2, 1::2]
    assert np.array_equal(out, (((a + b) + c) + d) * np.float32(0.25))


def test_general_path_matches_the_u8_restatement_on_u8_values():
    """The float2 general path is resizeArea_ with T = float: on integer-valued data it accumulates exactly what the u8 form does
    before saturate_cast (pyramid_oracle.resize_area_u8 rounds that sum)."""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (227, 333), np.uint8)
    f = np.stack([img, 255 - img], -1).astype(np.float32)
    out = ref.resize_area_flow(f, 221, 151)
    assert np.array_equal(np.clip(np.rint(out[..., 0]), 0, 255).astype(np.uint8), pyramid_oracle.resize_area_u8(img, 221, 151))


def test_scale_is_one_float_multiply_and_a_copy_at_one():
    f = np.array([[[1.5, -0.0], [3.0, 7.25]]], np.float32)
    assert np.array_equal(ref.times_scale(f, 1.0), f) and np.signbit(ref.times_scale(f, 1.0)[0, 0, 1])
    s = 0.4
    got = ref.times_scale(f, s)
    assert np.array_equal(got, f * np.float32(s))
    assert ref.top_layer_flow(f, 2, 1, 0, 0.4).tobytes() == f.tobytes()


def test_the_flag_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mavflow.h")).read()
    assert re.search(r"#define MAV_OPTFLOW_USE_INITIAL_FLOW 4\b", txt)
    from mavflow import _lib
    assert _lib.OPTFLOW_USE_INITIAL_FLOW == 4
    assert {"mav_farneback_init", "mav_farneback_init_dev"} <= set(_lib.EXPORTS)

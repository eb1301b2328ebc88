"""The 16-bit / float32 checker (tests/depth_ref.py) pinned to the C oracle it restates, before any GPU comparison uses it: on u8
values cast to float32 it must BE the oracle, bit for bit, stage by stage and end to end."""
import numpy as np
import pytest

import depth_ref
from oracle import fb_oracle as fbo


@pytest.mark.parametrize("W,H,levels", [(333, 227, 1), (160, 120, 1), (58, 174, 1), (160, 120, 5), (333, 227, 5)])
def test_blur_resize_f32_is_the_oracle_on_u8_values(fb_oracle, W, H, levels):
    """Every layer of several shapes (ragged widths; 5 levels on a small frame: every layer the size floor leaves).  Long Gaussians
    at fixed sizes: test_blur_resize_f32_at_fixed_kernels."""
    rng = np.random.default_rng(W * 7 + H + levels)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p = fbo.Params(0.4, levels, 12, 10, 8, 1.2, 0)
    for k in range(fb_oracle.num_layers(W, H, p)):
        w, h, sigma, ksize = fb_oracle.layer_dims(W, H, p, k)
        got = depth_ref.blur_resize_f32(img.astype(np.float32), w, h, ksize, sigma, fb_oracle)
        exp = fb_oracle.blur_resize(img, w, h, ksize, sigma)
        assert got.dtype == np.float32 and got.shape == exp.shape
        assert np.array_equal(got, exp), (W, H, k, ksize, float(np.abs(got - exp).max()))


@pytest.mark.parametrize("ksize,sigma", [(3, 0.0), (5, 0.75), (13, 2.3), (37, 6.25)])
def test_blur_resize_f32_at_fixed_kernels(fb_oracle, ksize, sigma):
    """333x227, 160x120 and 58x174 at ksize 3, 5, 13 and 37 (a long Gaussian of the 4K / 5-layer preset), each at a 0.4 resize."""
    for W, H in ((333, 227), (160, 120), (58, 174)):
        img = np.random.default_rng(ksize + W).integers(0, 256, (H, W), dtype=np.uint8)
        w, h = int(round(W * 0.4)), int(round(H * 0.4))
        exp = fb_oracle.blur_resize(img, w, h, ksize, sigma)
        assert np.array_equal(depth_ref.blur_resize_f32(img.astype(np.float32), w, h, ksize, sigma, fb_oracle), exp), (W, H)


def test_u16_and_f64_inputs_convert_as_convert_to(fb_oracle):
    """uint16 -> float32 is exact; float64 is rounded to nearest float32 (numpy's astype = saturate_cast<float>)."""
    img16 = depth_ref.pair16(96, 64)[0]
    assert img16.dtype == np.uint16 and int(img16.max()) - int(img16.min()) > 40000
    a = depth_ref.blur_resize_f32(img16, 38, 26, 5, 0.75, fb_oracle)
    b = depth_ref.blur_resize_f32(img16.astype(np.float32), 38, 26, 5, 0.75, fb_oracle)
    assert np.array_equal(a, b)
    f64 = img16.astype(np.float64) / 65535.0 * 255.0 + 1e-9
    assert np.array_equal(depth_ref.blur_resize_f32(f64, 38, 26, 5, 0.75, fb_oracle),
                          depth_ref.blur_resize_f32(f64.astype(np.float32), 38, 26, 5, 0.75, fb_oracle))


def test_calc_depth_is_the_oracle_on_u8_values(fb_oracle):
    from mavflow import synth
    W, H = 160, 120
    f0, f1, _ = synth.make_pair(W, H, 1)
    p = fbo.default_params()
    assert np.array_equal(depth_ref.calc_depth(fb_oracle, f0.astype(np.float32), f1.astype(np.float32), p), fb_oracle.calc(f0, f1, p))
    # ... and with an initial flow it is initial_flow_ref.calc_init
    import initial_flow_ref
    flow0 = initial_flow_ref.smooth_initial_flow(W, H)
    assert np.array_equal(depth_ref.calc_depth(fb_oracle, f0, f1, p, flow0), initial_flow_ref.calc_init(fb_oracle, f0, f1, flow0, p))


def test_the_16_bit_pair_carries_sub_8_bit_detail():
    from mavflow import synth
    a, b = depth_ref.pair16(200, 150)
    assert a.dtype == np.uint16 and int(a.max()) - int(a.min()) > 60000
    assert len(np.unique(a & 0xff)) > 200                     # the low byte is not constant: detail below one 8-bit step
    assert not np.array_equal(a, b)
    u0, _, _ = synth.make_pair(200, 150, 0)                   # the same scene as synth's u8 pair (a different intensity span)
    assert np.corrcoef(a.ravel().astype(np.float64), u0.ravel().astype(np.float64))[0, 1] > 0.999

"""Every kernel form of the layer images (convertTo -> GaussianBlur -> resize), at the smallest frames that reach it
(tests/stage_cases.py BLUR_CASES; tests/test_stage_cases_cpu.py shows the table is complete), through the stage hook, one frame a call:

  1. every layer, depth and frame against the oracle (u8) or tests/depth_ref.blur_resize_f32 (uint16, float32), within the bounds
     the suite has for the same comparison at the workload's sizes; integer depths are exact on layer 0;
  2. fused == two-pass, bit for bit, wherever the layer is fused;
  3. a u8 frame handed in as uint16 and as float32 gives the u8 frame's bytes, on every layer and in both forms: the u8 forms walk a
     re-aligned dword stream, the wide forms one element per pixel, and this holds the two cursors to each other.

mav_schedule_info's name of every layer ("3x3", "fused", "two-pass") is asserted against stage_cases.blur_form at every case."""
import numpy as np
import pytest

import depth_ref
from stage_cases import (BLUR_ATOL, BLUR_CASES, BLUR_CASE_IDS, COARSE_REL, DEPTH_DTYPES, F32_LAYER0_REL, blur_coarse_name, blur_form,
                         blur_frames, images, pyramid)

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def contexts(mav):
    yield _cache
    for ctx in _cache.values():
        ctx.close()
    _cache.clear()


def _ctx(contexts, case):
    if case.name not in contexts:
        from mavflow import _lib
        ctx = _lib.Context(case.W, case.H, 1, case.fb())
        assert [ctx.layer_dims(k)[:2] + ctx.layer_dims(k)[3:] for k in range(ctx.num_layers())] == pyramid(case.W, case.H, case.pyr_scale, case.levels)
        contexts[case.name] = ctx
    return contexts[case.name]


def _forms(ctx, case, depth):
    """blur_form of every layer, checked against the library's own name for it"""
    names = [l["blur"] for l in ctx.schedule_info(1, DEPTH_DTYPES[depth])["layers"]]
    forms = [blur_form(case.W, case.H, layer, depth) for layer in pyramid(case.W, case.H, case.pyr_scale, case.levels)]
    assert names == [blur_coarse_name(f) if k else "3x3" for k, f in enumerate(forms)], (case.name, depth, names, forms)
    return forms


@pytest.mark.parametrize("case", BLUR_CASES, ids=BLUR_CASE_IDS)
def test_layer_images_against_the_oracle(contexts, fb_oracle, case):
    ctx = _ctx(contexts, case)
    worst = {}
    for depth in case.depths:
        forms = _forms(ctx, case, depth)
        for k, form in enumerate(forms):
            w, h, sigma, ks = ctx.layer_dims(k)
            for img in blur_frames(case, depth):
                if depth == "u8":
                    exp = fb_oracle.blur_resize(img, w, h, ks, sigma)
                else:
                    exp = depth_ref.blur_resize_f32(img, w, h, ks, sigma, fb_oracle)
                for two_pass in ((False, True) if form.startswith("fused") else (False,)):
                    got = ctx.stage_blur_resize(img, k, two_pass=two_pass)
                    tag = (case.name, depth, k, form, two_pass)
                    if k == 0 and depth != "f32":
                        assert np.array_equal(got, exp), (tag, int((got != exp).sum()))          # taps 1/4, 1/2, 1/4: exact
                    elif depth == "u8":
                        e = float(np.abs(got - exp).max())
                        worst[tag] = e
                        assert e <= BLUR_ATOL, (tag, e)
                    else:
                        rel = float(np.abs(got.astype(np.float64) - exp).max() / np.abs(exp).max())
                        worst[tag] = max(worst.get(tag, 0.0), rel)
                        assert rel <= (F32_LAYER0_REL if k == 0 else COARSE_REL), (tag, ks, rel)
    print("\n[blur forms] worst error per (case, depth, layer, form, forced two-pass):", {str(k[1:]): f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("case", BLUR_CASES, ids=BLUR_CASE_IDS)
def test_fused_equals_two_pass(contexts, case):
    ctx = _ctx(contexts, case)
    for depth in case.depths:
        for k, form in enumerate(_forms(ctx, case, depth)):
            if not form.startswith("fused"):
                continue
            for img in blur_frames(case, depth):
                a, b = ctx.stage_blur_resize(img, k), ctx.stage_blur_resize(img, k, two_pass=True)
                assert np.array_equal(a, b), (case.name, depth, k, form, int((a != b).sum()))


@pytest.mark.parametrize("case", BLUR_CASES, ids=BLUR_CASE_IDS)
def test_u8_values_give_the_u8_bytes_at_every_depth(contexts, case):
    ctx = _ctx(contexts, case)
    for img in images(case):
        for k in range(ctx.num_layers()):
            for two_pass in (False, True):
                ref = ctx.stage_blur_resize(img, k, two_pass=two_pass)
                for depth in case.depths:
                    if depth == "u8":
                        continue
                    got = ctx.stage_blur_resize(img.astype(DEPTH_DTYPES[depth]), k, two_pass=two_pass)
                    assert got.tobytes() == ref.tobytes(), (case.name, depth, k, two_pass, int((got != ref).sum()))

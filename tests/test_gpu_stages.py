"""Every kernel form of the Farneback path, stage by stage, against the oracle (oracle/farneback_oracle.c) and the float64
restatement (tests/stage_ref64.py), at the frames and parameters of tests/stage_cases.py -- where tiles, borders and dispatch
predicates go wrong.  One stage at a time on identical inputs: nothing here is amplified by ten sweeps per layer, so a per-pixel slip
that the end-to-end flow gate (oracle/tolerances.py) would absorb fails here.

Bit-exact: the layer-0 blur (every product exact in float32) against the oracle; the initial flow (INTER_AREA, COPY / FAST / GENERAL)
against tests/initial_flow_ref.py; the fused upsample of the initial M (k_update_matrices MODE 1) against the explicit-flow form fed
the oracle's upsampled flow; MODE 0 against MODE 2 with a zero field; a sweep's M' against UpdateMatrices of the flow it stored.
Toleranced, per pixel: every bound below quotes the worst value measured over this matrix on an MI355X and is at most 4x that
(and never looser than tests/test_gpu_flow.py's bound for the same comparison).  Against stage_ref64, for the linear stages, the
GPU's error from float64 may be a small multiple of the oracle's own error from float64 (REF64_RATIO); stage_ref64 is evaluated on
layers of at most REF64_MAX_PIXELS pixels (not on the 4K frame's finest layer)."""
import numpy as np
import pytest

import stage_ref64 as ref
from initial_flow_ref import smooth_initial_flow, top_layer_flow
from stage_cases import (BLUR_ATOL, BLUR_CASES, CASES, CASE_IDS, DEPTH_DTYPES, FORMS, REF64_MAX_PIXELS, UNTESTED, blur0_form,
                         blur_case_forms, blur_coarse_name, crafted_flow, images, initial_flow_form, polyexp_form, smooth_flow,
                         sweep_form)

pytestmark = pytest.mark.gpu
EPS = ref.EPS32
TINY = 2.0 ** -126 * 16

# ---- bounds: at most 4x the worst value measured over every case, layer and input of the matrix on an MI355X --------------------
POLY_ATOL = 1.1e-4          # |GPU - oracle|: measured 2.8e-5 (1000x562, poly_n 5); was 2e-4
POLY_REL = 0.62             # |GPU - oracle| / ((4 n + 4) 2^-24 magnitude), per pixel: measured 0.156 (1000x562)
UPDATE_REL = 2.2            # |GPU - oracle| / (16 x 2^-24 magnitude), per pixel: measured 0.569 (1000x562)
# max |GPU - ref64| / max |oracle - ref64| (the GPU's error from float64 against the oracle's own)
REF64_RATIO = {"blur": 5.0,       # measured 1.26 (3840x2160)
               "polyexp": 31.0,   # measured 7.7 at 8x2 (the oracle's own error is tiny there), <= 2.3 everywhere else
               "update": 7.6}     # measured 1.90 (16x12)
SWEEP_C = 1100              # |GPU flow - oracle flow| / _sweep_unit, per pixel: measured 276 (1000x562, winsize 9, generic kernel)
SWEEP_MAX = 5.4e-4          # px, any pixel of a sweep from the smooth flows: measured 1.37e-4 (58x174, winsize 5; round 6's survey,
                            # winsize 12 only, had 5e-5); was 2e-3
_cache = {}


@pytest.fixture(scope="module")
def contexts(mav):
    yield _cache
    for v in _cache.values():
        v["ctx"].close()
    _cache.clear()


def _case_data(contexts, fb_oracle, case):
    if case.name not in contexts:
        from mavflow import _lib
        ctx = _lib.Context(case.W, case.H, 1, case.fb())
        p = case.oracle_params()
        L = ctx.num_layers()
        assert L == fb_oracle.num_layers(case.W, case.H, p)
        for k in range(L):
            assert ctx.layer_dims(k) == fb_oracle.layer_dims(case.W, case.H, p, k)
        contexts[case.name] = dict(ctx=ctx, L=L, imgs=images(case), layers={})
    return contexts[case.name]


def _layer(contexts, fb_oracle, case, k):
    d = _case_data(contexts, fb_oracle, case)
    if k not in d["layers"]:
        w, h, sigma, ks = d["ctx"].layer_dims(k)
        I = [fb_oracle.blur_resize(img, w, h, ks, sigma) for img in d["imgs"]]
        R = [fb_oracle.polyexp(i, case.poly_n, case.poly_sigma) for i in I]
        d["layers"][k] = dict(w=w, h=h, sigma=sigma, ks=ks, I=I, R=R, small=w * h <= REF64_MAX_PIXELS)
    return d["ctx"], d["layers"][k]


def soa(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def aos(a):
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))


def _report(stage, case, **vals):
    print(f"\n[stages] {stage} {case.name}: " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in vals.items()))


def _ref64_ratio(gpu, orc, exp):
    """max |GPU - ref64| / max |oracle - ref64| (1 when both are exact)"""
    eg, eo = float(np.abs(gpu - exp).max()), float(np.abs(orc - exp).max())
    return eg / eo if eo > 0 else (1.0 if eg == 0 else np.inf)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_blur_resize(contexts, fb_oracle, case):
    """Layer 0 (3x3 u8 kernel or the two-pass form) is the oracle bit for bit; coarser layers (fused or two-pass) within BLUR_ATOL."""
    d = _case_data(contexts, fb_oracle, case)
    worst = ratio = 0.0
    for k in range(d["L"]):
        ctx, l = _layer(contexts, fb_oracle, case, k)
        for img, exp in zip(d["imgs"], l["I"]):
            got = ctx.stage_blur_resize(img, k)
            if k == 0:
                assert np.array_equal(got, exp), (case.name, int((got != exp).sum()))
                continue
            e = float(np.abs(got - exp).max())
            worst = max(worst, e)
            if l["small"]:
                ratio = max(ratio, _ref64_ratio(got, exp, ref.blur_resize(img, l["w"], l["h"], l["ks"], l["sigma"])))
            assert e <= BLUR_ATOL, (case.name, k, e)
            assert ratio <= REF64_RATIO["blur"], (case.name, k, ratio)
    _report("blur", case, max_abs=worst, ref64_ratio=ratio)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_polyexp(contexts, fb_oracle, case):
    d = _case_data(contexts, fb_oracle, case)
    n = case.poly_n
    worst = rel = ratio = 0.0
    for k in range(d["L"]):
        ctx, l = _layer(contexts, fb_oracle, case, k)
        for I, R in zip(l["I"], l["R"]):
            got = aos(ctx.stage_polyexp(I, k))
            diff = np.abs(got.astype(np.float64) - R)
            worst = max(worst, float(diff.max()))
            if l["small"]:
                exp = ref.polyexp(I, n, case.poly_sigma)
                mag = ref.polyexp(I, n, case.poly_sigma, magnitude=True)
                rel = max(rel, float((diff / ((4 * n + 4) * EPS * mag + TINY)).max()))
                ratio = max(ratio, _ref64_ratio(got, R, exp))
            assert worst <= POLY_ATOL and rel <= POLY_REL and ratio <= REF64_RATIO["polyexp"], (case.name, k, worst, rel, ratio)
    _report("polyexp", case, max_abs=worst, rel=rel, ref64_ratio=ratio)


def _flows(w, h):
    return [("smooth", smooth_flow(w, h)), ("crafted", crafted_flow(w, h))]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_update_matrices(contexts, fb_oracle, case):
    """MODE 2 (explicit flow) against the oracle per pixel; MODE 0 == MODE 2 with a zero field; MODE 1 (the coarser flow upsampled
    inside the kernel) == MODE 2 fed fb_oracle.resize_flow of it -- both share update_px (launch_initial_m picks the mode from its FlowSource), so this isolates the fused upsample."""
    d = _case_data(contexts, fb_oracle, case)
    rel = ratio = 0.0
    for k in range(d["L"]):
        ctx, l = _layer(contexts, fb_oracle, case, k)
        w, h = l["w"], l["h"]
        R0, R1 = (soa(r) for r in l["R"])
        for tag, flow in _flows(w, h):
            got = aos(ctx.stage_update_matrices(R0, R1, flow, k)).astype(np.float64)
            exp = fb_oracle.update_matrices(l["R"][0], l["R"][1], flow)
            scale = np.abs(exp).max()
            np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-6 * scale)          # tests/test_gpu_flow.py's bound, kept
            if l["small"]:
                e64, mag = ref.update_matrices(l["R"][0], l["R"][1], flow, magnitude=True)
                rel = max(rel, float((np.abs(got - exp) / (16 * EPS * mag + TINY)).max()))
                ratio = max(ratio, _ref64_ratio(got, exp, e64))
            assert rel <= UPDATE_REL and ratio <= REF64_RATIO["update"], (case.name, k, tag, rel, ratio)
        zero = ctx.stage_update_matrices_from(R0, R1, None, k)
        assert np.array_equal(zero, ctx.stage_update_matrices(R0, R1, np.zeros((h, w, 2), np.float32), k)), (case.name, k)
        if k + 1 < d["L"]:
            pw, ph = ctx.layer_dims(k + 1)[:2]
            for tag, fc in _flows(pw, ph):
                fused = ctx.stage_update_matrices_from(R0, R1, fc, k)
                up = fb_oracle.resize_flow(fc, w, h, 1.0 / case.pyr_scale)
                explicit = ctx.stage_update_matrices(R0, R1, up, k)
                assert np.array_equal(fused, explicit), (case.name, k, tag, int((fused != explicit).sum()))
        else:
            with pytest.raises(ValueError):
                ctx.stage_update_matrices_from(R0, R1, np.zeros((h, w, 2), np.float32), k)
    _report("update_matrices", case, rel=rel, ref64_ratio=ratio)


def _sweep_unit(M, sys, d, winsize):
    """2^-24 ||G^-1|| (||G_abs|| ||d|| + ||h_abs||) per pixel: how far float32 window sums of M move the solution of the system the
    oracle solved (sys = its want_sys record, d = its flow).  G^-1 is the solve's regularised inverse adj(G) / (det + 1e-3) of the
    oracle's G; G_abs and h_abs are the same window sums over |M| -- a float32 sum errs by a fraction of the sum of its terms'
    magnitudes, not of its value, and the h planes cancel heavily where a large flow meets the image border."""
    m = winsize // 2
    Gabs = ref.box_sums(np.abs(M.astype(np.float64)), m) / float(winsize * winsize)
    g11, g12, g22 = sys[..., 0], sys[..., 1], sys[..., 2]
    lmax = np.abs(g11 + g22) / 2 + np.hypot((g11 - g22) / 2, g12)
    inv_norm = lmax / np.abs(g11 * g22 - g12 * g12 + 1e-3)
    labs = (Gabs[..., 0] + Gabs[..., 2]) / 2 + np.hypot((Gabs[..., 0] - Gabs[..., 2]) / 2, Gabs[..., 1])
    return EPS * inv_norm * (labs * np.hypot(d[..., 0], d[..., 1]) + np.hypot(Gabs[..., 3], Gabs[..., 4]))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sweep(contexts, fb_oracle, case):
    """One sweep per layer and flow.  The flow bound scales with the conditioning of the system the oracle solved:
    |GPU - oracle| <= SWEEP_C x _sweep_unit per pixel, and -- for the smooth flows, a flow some way into an iteration -- SWEEP_MAX px
    anywhere (the crafted flows displace whole border columns across the frame, up to w - 1 px, and are held by the relative bound
    alone).  M' is UpdateMatrices of the flow the GPU stored, bit for bit, and the oracle's UpdateMatrices of that flow per pixel."""
    d = _case_data(contexts, fb_oracle, case)
    worst = cmax = cissue = 0.0
    for k in range(d["L"]):
        ctx, l = _layer(contexts, fb_oracle, case, k)
        w, h = l["w"], l["h"]
        R0, R1 = (soa(r) for r in l["R"])
        for tag, flow in _flows(w, h):
            M = fb_oracle.update_matrices(l["R"][0], l["R"][1], flow)
            eflow, eM, sys = fb_oracle.blur_iter(l["R"][0], l["R"][1], flow, M, case.winsize, True, want_sys=True)
            gflow, gM = ctx.stage_blur_iter(R0, R1, soa(M), k, True)
            e = np.hypot(*(gflow.astype(np.float64) - eflow).transpose(2, 0, 1))
            c = float((e / (_sweep_unit(M, sys, eflow, case.winsize) + TINY)).max())
            cissue = max(cissue, float((e / (EPS * ref.system_bound_terms(sys[..., :5], eflow.astype(np.float64)) + TINY)).max()))
            cmax = max(cmax, c)
            if tag == "smooth":
                worst = max(worst, float(e.max()))
                assert e.max() <= SWEEP_MAX, (case.name, k, tag, float(e.max()))
            assert c <= SWEEP_C, (case.name, k, tag, c)
            assert np.array_equal(gM, ctx.stage_update_matrices(R0, R1, gflow, k)), (case.name, k, tag)
            om = fb_oracle.update_matrices(l["R"][0], l["R"][1], gflow)
            np.testing.assert_allclose(aos(gM), om, rtol=1e-4, atol=1e-6 * np.abs(om).max())
            if tag == "smooth":
                gflow_last, none = ctx.stage_blur_iter(R0, R1, soa(M), k, False)
                assert none is None and np.array_equal(gflow_last, gflow), (case.name, k)
    _report("sweep", case, max_px_smooth=worst, C=cmax, C_plain_norms=cissue)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_initial_flow(contexts, fb_oracle, case):
    """resize(flow0, INTER_AREA) * pyr_scale^k to every layer, bit for bit against tests/initial_flow_ref.py."""
    d = _case_data(contexts, fb_oracle, case)
    ctx = d["ctx"]
    flow0 = smooth_initial_flow(case.W, case.H)
    for k in range(d["L"]):
        w, h = ctx.layer_dims(k)[:2]
        got = ctx.stage_initial_flow(flow0, k)
        exp = top_layer_flow(flow0, w, h, k, case.pyr_scale)
        assert np.array_equal(got, exp), (case.name, k, initial_flow_form(case.W, case.H, w, h), int((got != exp).sum()))


def test_every_kernel_form_is_reached(mav):
    """Each case reaches the forms it names, and together they reach every form of stage_cases.FORMS (the forms listed in
    stage_cases.UNTESTED are not reachable from a legal context and are left out on purpose; see the comment there)."""
    from mavflow import _lib
    reached = {s: set() for s in FORMS}
    for case in CASES:
        got = set()
        with _lib.Context(case.W, case.H, 1, case.fb()) as ctx:
            info = ctx.schedule_info(1)["layers"]
            L = ctx.num_layers()
            for k in range(L):
                w, h = ctx.layer_dims(k)[:2]
                got |= {("sweep", sweep_form(w, case.winsize)), ("polyexp", polyexp_form(case.poly_n)),
                        ("initial_flow", initial_flow_form(case.W, case.H, w, h)), ("initial_m", "mode0"), ("initial_m", "mode2")}
                if k + 1 < L:
                    got.add(("initial_m", "mode1"))
                if k == 0:
                    assert info[0]["blur"] == "3x3"
                    got.add(("blur0", blur0_form(case.W, case.H)))
                else:
                    got.add(("blur", info[k]["blur"]))
        for s, f in got:
            reached[s].add(f)
        names = {f for _, f in got}
        assert case.expects <= names, (case.name, sorted(case.expects - names))
    for case in BLUR_CASES:                                       # the layer images' finer forms, at frames of their own
        forms = blur_case_forms(case)
        with _lib.Context(case.W, case.H, 1, case.fb()) as ctx:
            for depth in case.depths:
                info = ctx.schedule_info(1, DEPTH_DTYPES[depth])["layers"]
                for f, k, forced in forms:
                    if k and not forced and f.startswith(depth + ":"):
                        assert info[k]["blur"] == blur_coarse_name(f.split(":")[1]), (case.name, k, f, info[k])
        names = {f for f, _, _ in forms}
        assert case.expects <= names, (case.name, sorted(case.expects - names))
        reached["blur_form"] |= names
    for s, forms in FORMS.items():
        assert forms <= reached[s], (s, sorted(forms - reached[s]))
        assert not (UNTESTED.get(s, set()) & reached[s])

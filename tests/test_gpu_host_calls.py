"""The host-pointer entry points as a family (csrc/mavflow.cpp, HostCall): an output the caller does not ask for changes none of the
others; what a host detection call leaves resident survives the calls that read it, in any order and as often as they come; and such
a call gives its staging blocks back when it is refused half-way.  66x33 (no multiple of any tile), batch 3."""
import ctypes as C
import itertools

import numpy as np
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu
W, H, B = 66, 33, 3
N_PAIRS = dc.DETECT_PAIRS


@pytest.fixture(scope="module")
def x():
    """the inputs every test here reads (none writes them)"""
    from mavflow import _lib, synth
    rng = np.random.default_rng(66033)
    frames = np.stack([synth.make_pair(W, H, i)[0] for i in range(B + 1)])
    flow32 = np.array(dc.noise_fields(W, H))
    fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
    fp.n_pairs, fp.mag_threshold = N_PAIRS, dc.DETECT_GATE
    v = dict(prev=frames[:-1].copy(), next=frames[1:].copy(), flow32=flow32, flow64=flow32.astype(np.float64), foe=dc.foes(W, H),
             sky=dc.sky_masks(W, H).astype(np.uint8), samples=dc.detect_samples(W, H, B, N_PAIRS), omega=dc.OMEGA.copy(), dt=dc.DT.copy(),
             frame0=np.array([1, 0, 0], np.uint8), fp=fp, tp=tp, gt=np.where(rng.random((B, H, W)) < 0.3, 255, 0).astype(np.uint8),
             bgr=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), foe_gt=dc.foes(W, H)[::-1].copy())
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _outs(spec, want):
    """{name: array or None}: the outputs in `want` allocated (filled with a byte no result is made of all over), the others NULL"""
    return {k: (np.full(shape, 0xA5 if np.dtype(dt).kind in "ui" else np.nan, dt) if k in want else None) for k, (shape, dt) in spec.items()}


# name -> (optional outputs {name: (shape, dtype)}, call(ctx, x, outs)); an output that is always passed is checked with the rest
def _phi_mask(ft):
    def call(ctx, x, o):
        from mavflow import _lib
        fn = ctx.lib.mav_phi_mask_f32 if ft == np.float32 else ctx.lib.mav_phi_mask
        flow = x["flow32"] if ft == np.float32 else x["flow64"]
        _lib.check(fn(ctx.h, _p(flow), _p(x["foe"]), _p(x["sky"]), B, C.byref(x["tp"]), _p(o["phi"]), _p(o["mask_fixed"]), _p(o["mask_dyn"]),
                      _p(o["max_phi"])))
    return dict(phi=((B, H, W), ft), mask_fixed=((B, H, W), np.uint8), mask_dyn=((B, H, W), np.uint8), max_phi=((B,), ft)), call


def _stage_phi_mask(ctx, x, o):
    from mavflow import _lib
    _lib.check(ctx.lib.mav_stage_phi_mask(ctx.h, _p(x["flow32"]), _p(x["foe"]), _p(x["omega"]), _p(x["dt"]), _p(x["sky"]), B, C.byref(x["tp"]),
                                          _p(o["phi"]), _p(o["mask_fixed"]), _p(o["mask_dyn"]), _p(o["box"])))


def _process_batch(ctx, x, o):
    from mavflow import _lib
    res = np.empty(B, _lib.RESULT_DTYPE)
    _lib.check(ctx.lib.mav_process_batch(ctx.h, _p(x["prev"]), _p(x["next"]), _p(x["samples"]), _p(x["omega"]), _p(x["dt"]), _p(x["frame0"]),
                                         _p(x["sky"]), B, C.byref(x["fp"]), C.byref(x["tp"]), _p(o["flow"]), _p(o["phi"]), _p(o["mask_fixed"]),
                                         _p(o["mask_dyn"]), _p(res)))
    o["results"] = res


def _detect(ctx, x, o):
    from mavflow import _lib
    res = np.empty(B, _lib.RESULT_DTYPE)
    _lib.check(ctx.lib.mav_detect(ctx.h, _p(x["flow32"]), _p(x["samples"]), _p(x["omega"]), _p(x["dt"]), _p(x["frame0"]), _p(x["sky"]), B,
                                  C.byref(x["fp"]), C.byref(x["tp"]), _p(o["phi"]), _p(o["mask_fixed"]), _p(o["mask_dyn"]), _p(res)))
    o["results"] = res


def _render(ctx, x, o):
    from mavflow import _lib
    _lib.check(ctx.lib.mav_render(ctx.h, _p(x["flow32"]), _p(x["foe"]), _p(x["omega"]), _p(x["dt"]), _p(x["frame0"]), _p(x["sky"]), B,
                                  C.byref(x["tp"]), _p(o["result"]), _p(o["flow"]), _p(o["phi"])))


_MASKS = dict(mask_fixed=((B, H, W), np.uint8), mask_dyn=((B, H, W), np.uint8))
_IMG = ((B, H, W, 3), np.uint8)
ENTRY_POINTS = {
    "mav_phi_mask": _phi_mask(np.float64),
    "mav_phi_mask_f32": _phi_mask(np.float32),
    "mav_stage_phi_mask": (dict(phi=((B, H, W), np.float64), **_MASKS, box=((B, 4), np.int32)), _stage_phi_mask),
    "mav_process_batch": (dict(flow=((B, H, W, 2), np.float32), phi=((B, H, W), np.float64), **_MASKS), _process_batch),
    "mav_detect": (dict(phi=((B, H, W), np.float64), **_MASKS), _detect),
    "mav_render": (dict(result=_IMG, flow=_IMG, phi=_IMG), _render),
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_an_output_not_asked_for_changes_none_of_the_others(mav, x, name):
    """once with every optional output, then once per proper subset of them (the others NULL; the empty one included -- mav_render
    with no image at all returns OK): every buffer that comes back equals the all-outputs call's, byte for byte"""
    from mavflow import _lib
    spec, call = ENTRY_POINTS[name]
    with _lib.Context(W, H, B) as ctx:
        full = _outs(spec, set(spec))
        call(ctx, x, full)
        assert all(v is not None for v in full.values())
        for r in range(len(spec)):
            for want in itertools.combinations(spec, r):
                got = _outs(spec, set(want))
                call(ctx, x, got)
                for k, v in got.items():
                    if v is not None:
                        assert v.tobytes() == full[k].tobytes(), (name, want, k)


def _readers(ctx, x):
    """the calls that read what a host detection call left on the device, each returning what it returned as comparable values"""
    def png(files):
        return tuple(files)
    return {
        "counts": lambda: tuple(a.tobytes() for a in ctx.last_masks_tpr_fpr(x["gt"])),
        "render": lambda: tuple(v.tobytes() for _, v in sorted(ctx.render_last(B).items())),
        "overlay": lambda: tuple(np.asarray(a).tobytes() for a in ctx.overlay_last(x["bgr"], x["foe_gt"])),
        "render_png": lambda: tuple(png(v) for _, v in sorted(ctx.render_last_png(B).items())),
        "overlay_png": lambda: (lambda f, wr: (png(f), wr.tobytes()))(*ctx.overlay_last_png(x["bgr"], x["foe_gt"])),
    }


def _host_detect(ctx, x):
    out = ctx.detect(x["flow32"], x["samples"], omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"], foe_params=x["fp"],
                     thr_params=x["tp"])
    return {k: np.array(v) for k, v in out.items() if v is not None}             # copies: the arrays are pooled


ORDERS = (("counts", "render", "overlay", "render_png", "overlay_png"), ("overlay_png", "render_png", "counts", "overlay", "render"))


def _rounds(ctx, x, first=None):
    """every reader twice in a row, in both orders; -> (the first result of each, mem_info after each round)"""
    first = dict(first or {})
    readers, mem = _readers(ctx, x), []
    for order in ORDERS:
        for name in order:
            for _ in range(2):
                got = readers[name]()
                assert got == first.setdefault(name, got), name
        m = ctx.mem_info()
        mem.append((m["ctx_bytes"], m["workspace_bytes"]))
    return first, mem


def _direct(ctx, x, det):
    """the same results from the calls that take everything from the host"""
    foe = np.ascontiguousarray(det["results"]["foe"])
    mf, md = det["mask_fixed"].view(np.uint8), det["mask_dyn"].view(np.uint8)
    imgs = ctx.render(x["flow32"], foe, omega=x["omega"], dt=x["dt"], sky=x["sky"], thr_params=x["tp"], frame0=x["frame0"])
    over, wr = ctx.overlay(x["bgr"], mf, foe, x["foe_gt"])
    over, wr = np.array(over), np.array(wr)
    return {
        "counts": (ctx.tpr_fpr_counts(x["gt"], mf).tobytes(), ctx.tpr_fpr_counts(x["gt"], md).tobytes()),
        "render": tuple(v.tobytes() for _, v in sorted(imgs.items())),
        "overlay": (over.tobytes(), wr.tobytes()),
        "render_png": tuple(tuple(ctx.png_encode(v)) for _, v in sorted(imgs.items())),
        "overlay_png": (tuple(ctx.png_encode(over)), wr.tobytes()),
    }


def test_the_resident_results_survive_their_readers(mav, x):
    """after one host detect with both masks: the five mav_last_* calls in two orders, each twice in a row -- every result equals its
    first and the direct call's on the same inputs, and the context's memory does not change from the second round on"""
    from mavflow import _lib
    with _lib.Context(W, H, B) as ctx:
        det = _host_detect(ctx, x)
        first, mem = _rounds(ctx, x)
        assert mem[1] == mem[0], mem                      # (the first round has seen every reader: the second grows nothing)
        again, mem2 = _rounds(ctx, x, first)
        assert mem2 == [mem[1]] * 2, (mem, mem2)
        direct = _direct(ctx, x, det)
        for name in ORDERS[0]:
            assert first[name] == direct[name], name


def test_a_refused_reader_gives_its_blocks_back(mav, x):
    """mav_last_render with a wrong batch (MAV_ERR_STATE) and mav_last_overlay with a NaN foe_gt (MAV_ERR_ARG), then the sequence
    above: the results are what they are without the refused calls"""
    from mavflow import _lib
    with _lib.Context(W, H, B) as ctx:
        _host_detect(ctx, x)
        expected, _ = _rounds(ctx, x)
    with _lib.Context(W, H, B) as ctx:
        _host_detect(ctx, x)
        with pytest.raises(_lib.MavflowError):
            ctx.render_last(B - 1)
        nan_gt = x["foe_gt"].copy()
        nan_gt[1, 0] = np.float64("nan")
        with pytest.raises(ValueError, match="NaN"):
            ctx.overlay_last(x["bgr"], [tuple(r) for r in nan_gt])
        got, mem = _rounds(ctx, x)
        assert got == expected and mem[1] == mem[0]
        with pytest.raises(_lib.MavflowError):
            ctx.render_last(B - 1)
        assert _rounds(ctx, x, expected)[1] == [mem[1]] * 2

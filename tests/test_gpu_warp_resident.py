"""The entry points of include/mavflow_warp.h keep every kind of resident state: after each producer of tests/resident_cases.py, every
reader that applies returns the same code and bytes before and after every warp call, host and _dev form (the tables are imported, not
edited: the header of these entry points is not include/mavflow.h, whose list the tables cover).  And the calls hold no memory of the
context's: the _dev forms work on the caller's blocks, the host forms' staging goes back."""
import numpy as np
import pytest

import resident_cases as rc
import warp_cases as T
import warp_ref as R

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B


def _inputs():
    rng = np.random.default_rng(81)
    return dict(u8=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), f32=rng.normal(0, 3, (B, H, W, 2)).astype(np.float32),
                maps=np.stack([T.smooth_map(W, H, k) for k in range(B)]), A=np.stack([np.array(T.affine_matrices(W, H)[4].M, np.float64)] * B),
                P=np.stack([np.array(T.perspective_matrices(W, H)[-2].M, np.float64)] * B))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import warp
    lib = warp.load()
    p_, vp, h = rc.p_, rc.vp, env.h
    mx, my = np.ascontiguousarray(t["maps"][..., 0]), np.ascontiguousarray(t["maps"][..., 1])
    d8, d32 = np.zeros_like(t["u8"]), np.zeros_like(t["f32"])
    mag, rec = np.zeros((B, H, W), np.float32), np.zeros(B, R.RECORD_DTYPE)
    dev = lambda name, src: vp(env.dev("iv_warp_" + name, src))
    runs = {
        "mav_remap": lambda: lib.mav_remap(h, p_(t["u8"]), R.U8C3, p_(t["maps"]), B, p_(d8)),
        "mav_remap_dev": lambda: lib.mav_remap_dev(h, dev("u8", t["u8"]), R.U8C3, dev("maps", t["maps"]), B, dev("d8", d8.nbytes)),
        "mav_remap_planes": lambda: lib.mav_remap_planes(h, p_(t["f32"]), R.F32C2, p_(mx), p_(my), B, p_(d32)),
        "mav_remap_planes_dev": lambda: lib.mav_remap_planes_dev(h, dev("f32", t["f32"]), R.F32C2, dev("mx", mx), dev("my", my), B, dev("d32", d32.nbytes)),
        "mav_warp_flow": lambda: lib.mav_warp_flow(h, p_(t["u8"]), R.U8C3, p_(t["f32"]), B, p_(d8)),
        "mav_warp_flow_dev": lambda: lib.mav_warp_flow_dev(h, dev("u8", t["u8"]), R.U8C3, dev("f32", t["f32"]), B, dev("d8", d8.nbytes)),
        "mav_warp_affine": lambda: lib.mav_warp_affine(h, p_(t["f32"]), R.F32C2, p_(t["A"]), 0, B, p_(d32)),
        "mav_warp_affine_dev": lambda: lib.mav_warp_affine_dev(h, dev("f32", t["f32"]), R.F32C2, dev("A", t["A"]), 0, B, dev("d32", d32.nbytes)),
        "mav_warp_perspective": lambda: lib.mav_warp_perspective(h, p_(t["u8"]), R.U8C3, p_(t["P"]), R.INVERSE_MAP, B, p_(d8)),
        "mav_warp_perspective_dev": lambda: lib.mav_warp_perspective_dev(h, dev("u8", t["u8"]), R.U8C3, dev("P", t["P"]), 0, B, dev("d8", d8.nbytes)),
        "mav_warp_method": lambda: lib.mav_warp_method(h, p_(t["f32"]), p_(t["P"]), R.PERSPECTIVE, B, p_(d32), p_(mag), p_(rec)),
        "mav_warp_method_dev": lambda: lib.mav_warp_method_dev(h, dev("f32", t["f32"]), dev("A", t["A"]), R.AFFINE, B, dev("d32", d32.nbytes),
                                                               dev("mag", mag.nbytes), dev("rec", 16 * B)),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    big = np.zeros((B + 1, H, W, 3), np.uint8)
    out["mav_remap refused(batch above the context's)"] = (lambda: lib.mav_remap(h, p_(big), R.U8C3, p_(np.zeros((B + 1, H, W, 2), np.float32)), B + 1, p_(big.copy())), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_warp_calls(mav, pname):
    from mavflow import _lib, warp
    P, readers, t = rc.PRODUCERS[pname], rc.readers_of(pname), _inputs()
    fails = []
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            P.run(env)
            base = {}
            for name in readers:
                code, _, value = rc.READERS[name][2](env)
                assert code == rc.OK, (pname, name, code)
                base[name] = value
            ivs = _interveners(env, t)
            assert set(warp.EXPORTS) <= set(ivs)
            for iname, (run, want) in ivs.items():
                for rep in ("first", "second"):
                    got = run()
                    assert got == want, (pname, iname, got, _lib.load().mav_last_error())
                    for name in readers:
                        code, _, value = rc.READERS[name][2](env)
                        if code != rc.OK or value != base[name]:
                            fails.append(f"{pname}, {iname} ({rep}), {name}: returned {code}" + ("" if value == base[name] else " with other bytes"))
            ctx.sync()
        finally:
            env.close()
    assert not fails, "\n".join(fails)


def test_the_calls_hold_no_memory_of_the_contexts(mav):
    from mavflow import _lib
    t = _inputs()
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            ivs = _interveners(env, t)
            for run, want in ivs.values():                                  # once: the staging blocks exist from here on
                assert run() == want
            before = ctx.mem_info()
            for run, want in ivs.values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
            out = ctx.warp_method(t["f32"], t["P"])
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["mag"].shape == (B, H, W) and out["flow_max"].shape == (B, 2)
        finally:
            env.close()

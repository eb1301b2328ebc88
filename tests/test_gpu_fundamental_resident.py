"""The entry points of include/mavflow_fundamental.h keep every kind of resident state: after each producer of tests/resident_cases.py,
every reader that applies returns the same code and bytes before and after every new call, host and _dev form (the tables are imported,
not edited: the header of these entry points is not include/mavflow.h, whose list the tables cover).  And the calls hold no memory of the
context's: the _dev forms work in the caller's workspace (the flow form's gathered pairs included), the host forms' staging goes back."""
import ctypes as C

import numpy as np
import pytest

import fundamental_cases as T
import fundamental_ref as R
import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
N, ITERS = 48, 65


def _inputs():
    flow, coords, sub = T.flow_case(W, H, B, n=N, max_iters=ITERS)
    src, dst = R.flow_pairs(flow, coords)
    return dict(flow=flow, coords=coords, sub=sub, src=src, dst=dst, F=np.stack([T.true_F(T.K_CAM, *T.pose(b)) for b in range(B)]))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import fundamental
    lib = fundamental.load()
    p_, vp, h = rc.p_, rc.vp, env.h
    p = fundamental.fundamental_params(max_iters=ITERS)
    pp = C.byref(p)
    need = lib.mav_find_fundamental_workspace_bytes(N, B, pp)
    Fm, inl, rec, pairs = np.zeros((B, 3, 3)), np.zeros((B, N), np.uint8), np.zeros(B, R.RECORD_DTYPE), np.zeros((B, N, 2))
    res, mask, erec = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.uint8), np.zeros(B, R.EPI_DTYPE)
    dev = lambda name, src: vp(env.dev("iv_fundamental_" + name, src))
    outs = lambda: (dev("F", Fm.nbytes), dev("inl", inl.nbytes), dev("rec", rec.nbytes), dev("ws", need), need)
    dflt = fundamental.FundamentalParams()
    runs = {
        "mav_fundamental_defaults": lambda: (lib.mav_fundamental_defaults(C.byref(dflt)), rc.OK)[1],
        "mav_find_fundamental_workspace_bytes": lambda: rc.OK if lib.mav_find_fundamental_workspace_bytes(N, B, pp) == need else rc.ERR_ARG,
        "mav_find_fundamental": lambda: lib.mav_find_fundamental(h, p_(t["src"]), p_(t["dst"]), N, B, pp, p_(t["sub"]), p_(Fm), p_(inl), p_(rec)),
        "mav_find_fundamental_dev": lambda: lib.mav_find_fundamental_dev(h, dev("src", t["src"]), dev("dst", t["dst"]), N, B, pp, dev("sub", t["sub"]), *outs()),
        "mav_flow_fundamental": lambda: lib.mav_flow_fundamental(h, p_(t["flow"]), p_(t["coords"]), N, B, pp, p_(t["sub"]), p_(Fm), p_(inl), p_(rec), p_(pairs)),
        "mav_flow_fundamental_dev": lambda: lib.mav_flow_fundamental_dev(h, dev("flow", t["flow"]), p_(t["coords"]), N, B, pp, dev("sub", t["sub"]), *outs()),
        "mav_epipolar_residual": lambda: lib.mav_epipolar_residual(h, p_(t["flow"]), p_(t["F"]), 1.0, B, p_(res), p_(mask), p_(erec)),
        "mav_epipolar_residual_dev": lambda: lib.mav_epipolar_residual_dev(h, dev("flow", t["flow"]), dev("Fin", t["F"]), 1.0, B, dev("res", res.nbytes),
                                                                           dev("mask", mask.nbytes), dev("erec", erec.nbytes)),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    big = np.zeros((B + 1, N, 2))
    out["mav_find_fundamental refused(batch above the context's)"] = (
        lambda: lib.mav_find_fundamental(h, p_(big), p_(big), N, B + 1, pp, p_(np.tile(t["sub"][:1], (B + 1, 1, 1))), p_(np.zeros((B + 1, 3, 3))),
                                         p_(np.zeros((B + 1, N), np.uint8)), p_(np.zeros(B + 1, R.RECORD_DTYPE))), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_fundamental_calls(mav, pname):
    from mavflow import _lib, fundamental
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
            assert set(fundamental.EXPORTS) <= set(ivs)
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
    want = R.find(t["src"], t["dst"], t["sub"])
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            ivs = _interveners(env, t)
            for run, code in ivs.values():                                  # once: the staging blocks exist from here on
                assert run() == code
            before = ctx.mem_info()
            for iname, (run, code) in ivs.items():
                assert run() == code
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]), iname
            out = ctx.flow_fundamental(t["flow"], t["coords"], subsets=t["sub"])
            epi = ctx.epipolar_residual(t["flow"], out["F"])
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["F"].tobytes() == want["F"].tobytes() and out["records"].tobytes() == want["records"].tobytes()
            assert epi["records"].tobytes() == R.epipolar_residual(t["flow"], want["F"])["records"].tobytes()
        finally:
            env.close()

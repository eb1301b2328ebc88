"""The entry points of include/mavflow_affine.h keep every kind of resident state: after each producer of tests/resident_cases.py, every
reader that applies returns the same code and bytes before and after every affine call, host and _dev form (the tables are imported, not
edited: the header of these entry points is not include/mavflow.h, whose list the tables cover).  And the calls hold no memory of the
context's: the _dev forms work in the caller's workspace (the flow form's gathered pairs included), the host forms' staging goes back."""
import ctypes as C

import numpy as np
import pytest

import affine_cases as T
import affine_ref as R
import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
N, ITERS = 48, 65


def _inputs():
    flow, coords, tri = T.flow_case(W, H, B, n=N, max_iters=ITERS)
    src, dst = R.flow_pairs(flow, coords)
    return dict(flow=flow, coords=coords, tri=tri, src=src, dst=dst)


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import affine
    lib = affine.load()
    p_, vp, h = rc.p_, rc.vp, env.h
    p = affine.affine_params(max_iters=ITERS)
    pp = C.byref(p)
    need = lib.mav_estimate_affine_workspace_bytes(N, B, pp)
    M, inl, rec, pairs = np.zeros((B, 2, 3)), np.zeros((B, N), np.uint8), np.zeros(B, R.RECORD_DTYPE), np.zeros((B, N, 2))
    dev = lambda name, src: vp(env.dev("iv_affine_" + name, src))
    outs = lambda: (dev("M", M.nbytes), dev("inl", inl.nbytes), dev("rec", rec.nbytes), dev("ws", need), need)
    dflt = affine.AffineParams()
    runs = {
        "mav_affine_defaults": lambda: (lib.mav_affine_defaults(C.byref(dflt)), rc.OK)[1],
        "mav_estimate_affine_workspace_bytes": lambda: rc.OK if lib.mav_estimate_affine_workspace_bytes(N, B, pp) == need else rc.ERR_ARG,
        "mav_estimate_affine": lambda: lib.mav_estimate_affine(h, p_(t["src"]), p_(t["dst"]), N, B, pp, p_(t["tri"]), p_(M), p_(inl), p_(rec)),
        "mav_estimate_affine_dev": lambda: lib.mav_estimate_affine_dev(h, dev("src", t["src"]), dev("dst", t["dst"]), N, B, pp, dev("tri", t["tri"]), *outs()),
        "mav_flow_affine": lambda: lib.mav_flow_affine(h, p_(t["flow"]), p_(t["coords"]), N, B, pp, p_(t["tri"]), p_(M), p_(inl), p_(rec), p_(pairs)),
        "mav_flow_affine_dev": lambda: lib.mav_flow_affine_dev(h, dev("flow", t["flow"]), p_(t["coords"]), N, B, pp, dev("tri", t["tri"]), *outs()),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    big = np.zeros((B + 1, N, 2))
    out["mav_estimate_affine refused(batch above the context's)"] = (
        lambda: lib.mav_estimate_affine(h, p_(big), p_(big), N, B + 1, pp, p_(np.tile(t["tri"][:1], (B + 1, 1, 1))), p_(np.zeros((B + 1, 2, 3))),
                                        p_(np.zeros((B + 1, N), np.uint8)), p_(np.zeros(B + 1, R.RECORD_DTYPE))), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_affine_calls(mav, pname):
    from mavflow import _lib, affine
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
            assert set(affine.EXPORTS) <= set(ivs)
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
    want = R.estimate(t["src"], t["dst"], t["tri"])
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
            out = ctx.flow_affine(t["flow"], t["coords"], triples=t["tri"])
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["M"].tobytes() == want["M"].tobytes() and out["records"].tobytes() == want["records"].tobytes()
        finally:
            env.close()

"""The entry points of include/mavflow_essential.h keep every kind of resident state: after each producer of tests/resident_cases.py,
every reader that applies returns the same code and bytes before and after every new call, host and _dev form (the tables are imported,
not edited).  And the calls hold no memory of the context's: the _dev forms work in the caller's workspace (the flow form's gathered
pairs included), the host forms' staging goes back."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as T
import essential_ref as R
import fundamental_ref as FR
import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
N, ITERS = 48, 65


def _inputs():
    flow, coords, sub, cam = T.flow_case(W, H, B, n=N, max_iters=ITERS)
    src, dst = FR.flow_pairs(flow, coords)
    return dict(flow=flow, coords=coords, sub=sub, src=src, dst=dst, cam=cam)


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import essential
    lib = essential.load()
    p_, vp, h = rc.p_, rc.vp, env.h
    p = essential.essential_params(max_iters=ITERS, camera=t["cam"])
    pp = C.byref(p)
    need = lib.mav_find_essential_workspace_bytes(N, B, pp)
    E, Fm, inl, rec, pairs = np.zeros((B, 3, 3)), np.zeros((B, 3, 3)), np.zeros((B, N), np.uint8), np.zeros(B, R.RECORD_DTYPE), np.zeros((B, N, 2))
    dev = lambda name, src: vp(env.dev("iv_essential_" + name, src))
    outs = lambda: (dev("E", E.nbytes), dev("F", Fm.nbytes), dev("inl", inl.nbytes), dev("rec", rec.nbytes), dev("ws", need), need)
    dflt = essential.EssentialParams()
    runs = {
        "mav_essential_defaults": lambda: (lib.mav_essential_defaults(C.byref(dflt)), rc.OK)[1],
        "mav_find_essential_workspace_bytes": lambda: rc.OK if lib.mav_find_essential_workspace_bytes(N, B, pp) == need else rc.ERR_ARG,
        "mav_find_essential": lambda: lib.mav_find_essential(h, p_(t["src"]), p_(t["dst"]), N, B, pp, p_(t["sub"]), p_(E), p_(Fm), p_(inl), p_(rec)),
        "mav_find_essential_dev": lambda: lib.mav_find_essential_dev(h, dev("src", t["src"]), dev("dst", t["dst"]), N, B, pp, dev("sub", t["sub"]), *outs()),
        "mav_flow_essential": lambda: lib.mav_flow_essential(h, p_(t["flow"]), p_(t["coords"]), N, B, pp, p_(t["sub"]), p_(E), p_(Fm), p_(inl), p_(rec),
                                                             p_(pairs)),
        "mav_flow_essential_dev": lambda: lib.mav_flow_essential_dev(h, dev("flow", t["flow"]), p_(t["coords"]), N, B, pp, dev("sub", t["sub"]), *outs()),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    big = np.zeros((B + 1, N, 2))
    out["mav_find_essential refused(batch above the context's)"] = (
        lambda: lib.mav_find_essential(h, p_(big), p_(big), N, B + 1, pp, p_(np.tile(t["sub"][:1], (B + 1, 1, 1))), p_(np.zeros((B + 1, 3, 3))),
                                       p_(np.zeros((B + 1, 3, 3))), p_(np.zeros((B + 1, N), np.uint8)), p_(np.zeros(B + 1, R.RECORD_DTYPE))), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_essential_calls(mav, pname):
    from mavflow import _lib, essential
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
            assert set(essential.EXPORTS) <= set(ivs)
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
    want = R.find(t["src"], t["dst"], t["sub"], camera=t["cam"])
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
            out = ctx.flow_essential(t["flow"], t["coords"], subsets=t["sub"], camera=t["cam"])
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["E"].tobytes() == want["E"].tobytes() and out["F"].tobytes() == want["F"].tobytes()
            assert out["records"].tobytes() == want["records"].tobytes()
        finally:
            env.close()

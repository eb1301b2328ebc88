"""The entry points of include/mavflow_validation.h keep every kind of resident state: after each producer of tests/resident_cases.py,
every reader that applies returns the same code and bytes before and after a mav_gt_stats and a mav_gt_stats_dev (the tables are
imported, not edited: the header of these entry points is not include/mavflow.h, whose list the tables cover).  And the calls leave the
context's memory where it was: the scratch block exists from the first call on (counted by mav_mem_info) and grows with no later call
of the same shape; the host form's staging goes back."""
import numpy as np
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
MAX_PIXELS = 256


def _inputs():
    from mavflow import _validation as V
    rng = np.random.default_rng(67)
    seg = ((rng.random((B, H, W)) < 0.05) * 255).astype(np.uint8)
    depth = rng.uniform(1, 100, (B, H, W)).astype(np.float32)
    gt = rng.normal(0, 3, (B, H, W, 2)).astype(np.float32)
    sky = (depth > 70).astype(np.uint8)
    return dict(seg=seg, depth=depth, gt=gt, sky=sky, params=V.gt_stats_params(rng.normal(0, 0.2, (B, 3)), 1 / 30.0, batch=B))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host form on host arrays, the _dev form on the interveners' own device blocks"""
    from mavflow import _validation as V
    lib = V.load()
    p_, vp = rc.p_, rc.vp

    def host(with_indices):
        rec, idx = np.zeros(B, V.RECORD_DTYPE), np.zeros((B, MAX_PIXELS), np.int32)
        return lambda: lib.mav_gt_stats(env.h, p_(t["seg"]), p_(t["gt"]), p_(t["sky"]), p_(t["depth"]), p_(t["params"]), B, MAX_PIXELS, p_(rec),
                                        p_(idx) if with_indices else None)

    def dev():
        return lib.mav_gt_stats_dev(env.h, vp(env.dev("va_seg", t["seg"])), vp(env.dev("va_gt", t["gt"])), vp(env.dev("va_sky", t["sky"])),
                                    vp(env.dev("va_depth", t["depth"])), vp(env.dev("va_params", t["params"])), B, MAX_PIXELS,
                                    vp(env.dev("va_rec", B * 96)), vp(env.dev("va_idx", B * MAX_PIXELS * 4)))

    def refused():
        rec = np.zeros(B + 1, V.RECORD_DTYPE)
        return lib.mav_gt_stats(env.h, p_(t["seg"]), None, None, None, p_(t["params"]), B + 1, MAX_PIXELS, p_(rec), None)

    return {"mav_gt_stats": (host(True), rc.OK), "mav_gt_stats(no index list)": (host(False), rc.OK), "mav_gt_stats_dev": (dev, rc.OK),
            "mav_gt_stats refused(batch above the context's)": (refused, rc.ERR_ARG)}


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_validation_calls(mav, pname):
    from mavflow import _lib
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
            for iname, (run, want) in _interveners(env, t).items():
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


def test_the_calls_leave_the_memory_where_it_was(mav):
    from mavflow import _lib, _validation as V
    t = _inputs()
    with _lib.Context(W, H, B) as ctx:
        fresh = ctx.mem_info()
        # both shapes once: the staging blocks (one more with an index list) and the scratch (larger with the call's own list) exist from here on
        ctx.gt_stats(t["seg"], t["gt"], t["sky"], t["depth"], max_pixels=MAX_PIXELS, indices=True)
        ctx.gt_stats(t["seg"], t["gt"], t["sky"], t["depth"], max_pixels=MAX_PIXELS, indices=False)
        before = ctx.mem_info()
        assert before["ctx_bytes"] > fresh["ctx_bytes"]                     # the scratch is the context's and is counted while held
        env = rc.Env(ctx)
        try:
            for run, want in _interveners(env, t).values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
            out = ctx.gt_stats(t["seg"], t["gt"], t["sky"], t["depth"], max_pixels=MAX_PIXELS)
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["records"].dtype == V.RECORD_DTYPE
        finally:
            env.close()

"""The four entry points of include/mavflow_truth.h keep every kind of resident state: after each producer of
tests/resident_cases.py, every reader that applies returns the same code and bytes before and after a mav_gt_flow, a
mav_radial_error_hist and their _dev forms (the tables are imported, not edited: the header of these entry points is not
include/mavflow.h, whose list the tables cover).  And a closed accumulator leaves the context's memory where it was."""
import ctypes as C

import numpy as np
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B


def _inputs():
    from mavflow import _truth
    import truth_cases as T
    rng = np.random.default_rng(66)
    depth = rng.uniform(1, 200, (B, H, W)).astype(np.float32)
    seg = ((rng.random((B, H, W)) < 0.2) * 200).astype(np.uint8)
    vp1 = np.stack([T.view_proj(10 + b, W, H) for b in range(B)])
    inv = np.stack([np.linalg.inv(T.view_proj(20 + b, W, H)) for b in range(B)])
    return dict(depth=depth, seg=seg, params=_truth.gt_flow_params(vp1, inv, rng.normal(0, 5, (B, 3)), 100.0, B),
                em=_truth.DEFAULT_MAG_EDGES, ee=_truth.DEFAULT_ERR_EDGES, words=_truth.table_words(159, 159))


def _interveners(env, t):
    """name -> run() -> return code; host forms on host arrays, _dev forms on the interveners' own device blocks"""
    from mavflow import _lib, _truth
    lib, y = _truth.load(), env.y
    p_, vp = rc.p_, rc.vp

    def gt_host(depth_code):
        out = np.empty((B, H, W, 2), np.float32 if depth_code == _lib.DEPTH_32F else np.float64)
        return lambda: lib.mav_gt_flow(env.h, p_(t["depth"]), p_(t["seg"]), p_(t["params"]), B, depth_code, p_(out))

    def gt_dev():
        return lib.mav_gt_flow_dev(env.h, vp(env.dev("tr_depth", t["depth"])), vp(env.dev("tr_seg", t["seg"])), vp(env.dev("tr_params", t["params"])), B,
                                   _lib.DEPTH_64F, vp(env.dev("tr_flow", B * H * W * 16)))

    def hist_host():
        table = np.zeros(t["words"], np.int64)
        return lib.mav_radial_error_hist(env.h, p_(y["flow32"]), p_(env.x["flow32"]), p_(y["sky"]), B, p_(t["em"]), t["em"].size, p_(t["ee"]), t["ee"].size,
                                         p_(table))

    def hist_dev():
        return lib.mav_radial_error_hist_dev(env.h, vp(env.dev("iv_flow", y["flow32"])), vp(env.dev("p_flow", env.x["flow32"])), vp(env.dev("iv_sky", y["sky"])),
                                             B, p_(t["em"]), t["em"].size, p_(t["ee"]), t["ee"].size, vp(env.dev("tr_table", np.zeros(t["words"], np.int64))))

    def hist_refused():
        table = np.zeros(t["words"], np.int64)
        return lib.mav_radial_error_hist(env.h, p_(y["flow32"]), p_(env.x["flow32"]), None, B + 1, p_(t["em"]), t["em"].size, p_(t["ee"]), t["ee"].size, p_(table))

    return {"mav_gt_flow(32F)": (gt_host(_lib.DEPTH_32F), rc.OK), "mav_gt_flow(64F)": (gt_host(_lib.DEPTH_64F), rc.OK), "mav_gt_flow_dev": (gt_dev, rc.OK),
            "mav_radial_error_hist": (hist_host, rc.OK), "mav_radial_error_hist_dev": (hist_dev, rc.OK),
            "mav_radial_error_hist refused(batch above the context's)": (hist_refused, rc.ERR_ARG)}


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_truth_calls(mav, pname):
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


def test_a_closed_accumulator_leaves_the_memory_where_it_was(mav):
    from mavflow import _lib
    x = rc.inputs()
    with _lib.Context(W, H, B) as ctx:
        ctx.radial_error_hist(x["flow32"], x["alt"]["flow32"], x["sky"])          # the context's own blocks (staging, edge lists) exist from here on
        before = ctx.mem_info()
        acc = ctx.radial_error_accumulator()
        acc.add(x["flow32"], x["alt"]["flow32"], x["sky"])
        acc.add(x["flow32"][0], x["alt"]["flow32"][0], None)
        assert acc.counts()["non_sky"] > 0
        during = ctx.mem_info()
        acc.close()
        after = ctx.mem_info()
        assert acc.table is None
        assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) == (during["ctx_bytes"], during["workspace_bytes"])
        assert after["dev_free"] >= before["dev_free"] - (1 << 20)                # the table (202 KB) went back to the device
        acc.close()                                                               # closing twice is harmless

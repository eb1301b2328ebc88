"""The entry points of include/mavflow_cluster.h keep every kind of resident state: after each producer of tests/resident_cases.py, every
reader that applies returns the same code and bytes before and after mav_kmeans, mav_kmeans_dev, mav_kmeans_paint and
mav_kmeans_paint_dev (the tables are imported, not edited: the header of these entry points is not include/mavflow.h, whose list the tables
cover).  And the calls hold no memory of the context's: the _dev form works in the caller's workspace, the host form's staging goes
back."""
import ctypes as C

import numpy as np
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
N, D, K, A = W * H // 3, 3, 8, 10


def _inputs():
    from mavflow import clustering
    rng = np.random.default_rng(71)
    x = np.abs(rng.normal(0, 3, (B, N, D))).astype(np.float32)
    x[:, 100:140] += 40.0
    return dict(x=x, init=clustering.random_centers(x, K, A, rng=72), labels=rng.integers(0, K, (B, N)).astype(np.int32),
                centers=rng.uniform(0, 50, (B, K, D)).astype(np.float32), params=clustering.kmeans_params(K, A, 10, D, np.float32, 1.0))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import clustering
    lib = clustering.load()
    p_, vp = rc.p_, rc.vp
    need = lib.mav_kmeans_workspace_bytes(N, B, C.byref(t["params"]))
    assert need > 0

    def host():
        labels, centers, rec = np.zeros((B, N), np.int32), np.zeros((B, K, D), np.float32), np.zeros(B, clustering.RECORD_DTYPE)
        return lib.mav_kmeans(env.h, p_(t["x"]), N, B, C.byref(t["params"]), p_(t["init"]), p_(labels), p_(centers), p_(rec))

    def dev():
        return lib.mav_kmeans_dev(env.h, vp(env.dev("km_x", t["x"])), N, B, C.byref(t["params"]), vp(env.dev("km_init", t["init"])),
                                  vp(env.dev("km_labels", B * N * 4)), vp(env.dev("km_centers", B * K * D * 4)), vp(env.dev("km_rec", B * 96)),
                                  vp(env.dev("km_ws", need)), need)

    def paint():
        res, mask = np.zeros((B, N, D), np.uint8), np.zeros((B, N), np.uint8)
        return lib.mav_kmeans_paint(env.h, p_(t["labels"]), p_(t["centers"]), N, B, K, D, p_(res), p_(mask))

    def paint_dev():
        return lib.mav_kmeans_paint_dev(env.h, vp(env.dev("km_plabels", t["labels"])), vp(env.dev("km_pcenters", t["centers"])), N, B, K, D,
                                        vp(env.dev("km_res", B * N * D)), vp(env.dev("km_mask", B * N)))

    def refused():
        labels, centers, rec = np.zeros((B + 1, N), np.int32), np.zeros((B + 1, K, D), np.float32), np.zeros(B + 1, clustering.RECORD_DTYPE)
        return lib.mav_kmeans(env.h, p_(t["x"]), N, B + 1, C.byref(t["params"]), p_(t["init"]), p_(labels), p_(centers), p_(rec))

    return {"mav_kmeans": (host, rc.OK), "mav_kmeans_dev": (dev, rc.OK), "mav_kmeans_paint": (paint, rc.OK), "mav_kmeans_paint_dev": (paint_dev, rc.OK),
            "mav_kmeans refused(batch above the context's)": (refused, rc.ERR_ARG)}


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_clustering_calls(mav, pname):
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


def test_the_calls_hold_no_memory_of_the_contexts(mav):
    from mavflow import _lib
    t = _inputs()
    with _lib.Context(W, H, B) as ctx:
        ctx.kmeans(t["x"], K=K, init=t["init"], attempts=A)               # once: the staging blocks exist from here on
        ctx.kmeans_paint(t["labels"], t["centers"])
        before = ctx.mem_info()
        env = rc.Env(ctx)
        try:
            for run, want in _interveners(env, t).values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
            out = ctx.kmeans(t["x"], K=K, init=t["init"], attempts=A)
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out["labels"].shape == (B, N) and out["counts"].shape == (B, K) and (out["counts"].sum(1) == N).all()
        finally:
            env.close()

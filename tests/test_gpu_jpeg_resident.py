"""The entry points of include/mavflow_jpeg.h keep every kind of resident state: after each producer of tests/resident_cases.py, every
reader that applies returns the same code and bytes before and after every JPEG call, host and _dev form; and after a heavy call of
another family a JPEG call returns a fresh context's bytes.  The calls hold no memory of the context's."""
import numpy as np
import pytest

import jpeg_cases as jc
import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B


def _batch():
    """five 70 x 130 and 37 x 53 files: larger than the context's frame, so the staging blocks are larger than any producer's"""
    big = [c for c in jc.valid() if c.name.startswith("pil_70x130_") and "gray" not in c.name]
    small = [c for c in jc.valid() if c.name.startswith("pil_37x53_") and "gray" not in c.name]
    return big, small


def _packed(cases):
    from mavflow import _lib
    W_, H_, comps, packed, index, infos = _lib.Context._jpeg_pack([c.file for c in cases])
    return dict(W=W_, H=H_, n=len(cases), packed=packed, index=index, infos=infos, want=np.stack([c.bgr for c in cases]))


def _interveners(env, groups):
    """name -> (run() -> return code, the code expected)"""
    from mavflow import _lib
    lib, h, p_, vp = env.lib, env.h, rc.p_, rc.vp
    runs = {}
    for tag, g in groups.items():
        n, Wg, Hg = g["n"], g["W"], g["H"]
        out, st = np.zeros((n, Hg, Wg, 3), np.uint8), np.zeros(n, _lib.JPEG_STATUS_DTYPE)
        g["out"], g["st"] = out, st
        scratch = lib.mav_jpeg_decode_scratch_bytes(Wg, Hg, 3, n)
        dev = lambda name, src, tag=tag: vp(env.dev(f"iv_jpeg_{tag}_{name}", src))
        runs[f"mav_jpeg_decode {tag}"] = lambda g=g, out=out, st=st, n=n, Wg=Wg, Hg=Hg: lib.mav_jpeg_decode(
            h, p_(g["packed"]), p_(g["index"]), p_(g["infos"]), n, Wg, Hg, 1, p_(out), p_(st))
        runs[f"mav_jpeg_decode_dev {tag}"] = lambda g=g, dev=dev, n=n, Wg=Wg, Hg=Hg, scratch=scratch: lib.mav_jpeg_decode_dev(
            h, dev("files", g["packed"]), dev("index", g["index"]), dev("infos", g["infos"]), n, Wg, Hg, 2, dev("out", n * Hg * Wg),
            dev("st", 40 * n), dev("scratch", scratch))
    out = {k: (v, rc.OK) for k, v in runs.items()}
    g = next(iter(groups.values()))
    out["mav_jpeg_decode refused(count)"] = (lambda: lib.mav_jpeg_decode(h, p_(g["packed"]), p_(g["index"]), p_(g["infos"]), 0, g["W"], g["H"], 1,
                                                                         p_(g["out"]), p_(g["st"])), rc.ERR_ARG)
    out["mav_jpeg_decode_dev refused(scratch)"] = (lambda: lib.mav_jpeg_decode_dev(h, vp(env.dev("iv_jpeg_x", 64)), vp(env.dev("iv_jpeg_x", 64)),
                                                                                   vp(env.dev("iv_jpeg_x", 64)), 1, 8, 8, 1, vp(env.dev("iv_jpeg_x", 64)),
                                                                                   vp(env.dev("iv_jpeg_x", 64)), None), rc.ERR_ARG)
    return out


def _groups():
    big, small = _batch()
    return {"70x130": _packed(big), "37x53": _packed(small)}


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_jpeg_calls(mav, pname):
    from mavflow import _lib
    P, readers, groups = rc.PRODUCERS[pname], rc.readers_of(pname), _groups()
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
            ivs = _interveners(env, groups)
            for iname, (run, want) in ivs.items():
                for rep in ("first", "second"):
                    got = run()
                    assert got == want, (pname, iname, got, _lib.load().mav_last_error())
                    for name in readers:
                        code, _, value = rc.READERS[name][2](env)
                        if code != rc.OK or value != base[name]:
                            fails.append(f"{pname}, {iname} ({rep}), {name}: returned {code}" + ("" if value == base[name] else " with other bytes"))
            ctx.sync()
            for g in groups.values():                                   # and the JPEG calls themselves gave the fixture's pixels
                assert not g["st"]["code"].any() and np.array_equal(g["out"], g["want"])
        finally:
            env.close()
    assert not fails, "\n".join(fails)


def test_after_a_heavy_call_a_jpeg_call_returns_a_fresh_contexts_bytes(mav):
    from mavflow import _lib
    big, _ = _batch()
    files = [c.file for c in big]
    with _lib.Context(W, H, B) as fresh:
        want = {fmt: fresh.jpeg_decode(files, fmt, return_status=True) for fmt in ("bgr", "gray", "samples")}
    assert np.array_equal(want["bgr"][0], np.stack([c.bgr for c in big]))
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            rc.PRODUCERS["process_batch"].run(env)
            for fmt in ("bgr", "gray", "samples"):
                img, st = ctx.jpeg_decode(files, fmt, return_status=True)
                assert img.tobytes() == want[fmt][0].tobytes() and st.tobytes() == want[fmt][1].tobytes(), fmt
        finally:
            env.close()


def test_the_calls_hold_no_memory_of_the_contexts(mav):
    from mavflow import _lib
    groups = _groups()
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            ivs = _interveners(env, groups)
            for run, want in ivs.values():                                  # once: the staging blocks of every call shape exist from here on
                assert run() == want
            before = ctx.mem_info()
            for run, want in ivs.values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
        finally:
            env.close()

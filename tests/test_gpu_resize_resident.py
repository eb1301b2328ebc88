"""The entry points of include/mavflow_resize.h keep every kind of resident state: after each producer of tests/resident_cases.py, every
reader that applies returns the same code and bytes before and after every resize / sky-mask call, host and _dev form (the tables are
imported, not edited: the header of these entry points is not include/mavflow.h, whose list the tables cover).  The resident LK pyramid
and a flow_history ring persist across them.  And the calls hold no memory of the context's: the _dev forms work on the caller's blocks,
the host forms' staging goes back."""
import numpy as np
import pytest

import resident_cases as rc
import resize_ref as R

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B
SW, SH, DW, DH = 40, 24, 100, 51              # larger than the context's frame, so the staging blocks are larger than any producer's


def _inputs():
    rng = np.random.default_rng(83)
    return dict(u8=rng.integers(0, 256, (B, SH, SW, 3), dtype=np.uint8), f32=rng.normal(0, 3, (B, SH, SW, 2)).astype(np.float32))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import resize
    lib = resize.load()
    p_, vp, h = rc.p_, rc.vp, env.h
    d8, d32, sky = np.zeros((B, DH, DW, 3), np.uint8), np.zeros((B, DH, DW, 2), np.float32), np.zeros((B, DH, DW), np.uint8)
    s8, s32 = np.zeros((B, SH // 2, SW // 2, 3), np.uint8), np.zeros((B, 17, 29, 2), np.float32)
    dev = lambda name, src: vp(env.dev("iv_resize_" + name, src))
    runs = {
        "mav_resize": lambda: lib.mav_resize(h, p_(t["u8"]), R.U8C3, SW, SH, DW, DH, R.LINEAR, B, p_(d8)),
        "mav_resize area": lambda: lib.mav_resize(h, p_(t["f32"]), R.F32C2, SW, SH, 29, 17, R.AREA, B, p_(s32)),
        "mav_resize_dev": lambda: lib.mav_resize_dev(h, dev("f32", t["f32"]), R.F32C2, SW, SH, DW, DH, R.LINEAR, B, dev("d32", d32.nbytes)),
        "mav_resize_dev halving": lambda: lib.mav_resize_dev(h, dev("u8", t["u8"]), R.U8C3, SW, SH, SW // 2, SH // 2, R.LINEAR, B, dev("s8", s8.nbytes)),
        "mav_resize_dev nearest": lambda: lib.mav_resize_dev(h, dev("u8", t["u8"]), R.U8C3, SW, SH, DW, DH, R.NEAREST, B, dev("d8", d8.nbytes)),
        "mav_sky_mask": lambda: lib.mav_sky_mask(h, p_(t["u8"]), SW, SH, DW, DH, 180, 130, B, p_(sky)),
        "mav_sky_mask_dev": lambda: lib.mav_sky_mask_dev(h, dev("u8", t["u8"]), SW, SH, DW, DH, 180, 130, B, dev("sky", sky.nbytes)),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    big = np.zeros((B + 1, SH, SW, 3), np.uint8)
    out["mav_resize refused(batch above the context's)"] = (lambda: lib.mav_resize(h, p_(big), R.U8C3, SW, SH, DW, DH, R.LINEAR, B + 1, p_(np.zeros((B + 1, DH, DW, 3), np.uint8))), rc.ERR_ARG)
    out["mav_sky_mask_dev refused(key)"] = (lambda: lib.mav_sky_mask_dev(h, dev("u8", t["u8"]), SW, SH, DW, DH, 180, 300, B, dev("sky", sky.nbytes)), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_resize_calls(mav, pname):
    from mavflow import _lib, resize
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
            assert set(resize.EXPORTS) <= set(ivs)
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
            py = lambda: (ctx.resize(t["f32"], (DW, DH), batched=True), ctx.sky_mask(t["u8"], (DW, DH)))
            for run, want in ivs.values():                                  # once: the staging blocks of every call shape exist from here on
                assert run() == want
            py()
            before = ctx.mem_info()
            for run, want in ivs.values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
            out, m = py()
            after = ctx.mem_info()
            assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"]) and after["workspace_bytes"] == 0
            assert out.shape == (B, DH, DW, 2) and m.shape == (B, DH, DW)
        finally:
            env.close()


def _run_all(ctx, env, t):
    for run, want in _interveners(env, t).values():
        assert run() == want


def test_the_resident_lk_pyramid_persists(mav):
    """lk_track(None, ...) after the resize calls tracks from the frame given last before them, as on a context that made no such call"""
    from mavflow import _lib
    Wl, Hl = 96, 64
    base = np.random.default_rng(3).integers(0, 256, (Hl + 8, Wl + 8)).astype(np.float32)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4      # smoothed noise, moving by (1, 1) a frame
    seq = [np.ascontiguousarray(base[i:i + Hl, i:i + Wl]).astype(np.uint8) for i in range(3)]
    pts = np.stack(np.meshgrid(np.arange(10, Wl - 10, 12), np.arange(10, Hl - 10, 12)), -1).reshape(-1, 2).astype(np.float32)
    t = _inputs()
    outs = []
    for intervene in (False, True):
        with _lib.Context(Wl, Hl, B) as ctx:
            env = rc.Env(ctx)
            try:
                ctx.lk_track(seq[0], seq[1], pts)
                if intervene:
                    _run_all(ctx, env, t)
                p, s = ctx.lk_track(None, seq[2], pts)                    # from the resident pyramid of seq[1]
                outs.append(p.tobytes() + s.tobytes())
            finally:
                env.close()
    assert outs[0] == outs[1]


def test_a_flow_history_ring_persists(mav):
    from mavflow import _lib
    t = _inputs()
    rng = np.random.default_rng(7)
    fields = rng.normal(0, 1.5, (6, H, W, 2)).astype(np.float32)
    outs = []
    for intervene in (False, True):
        with _lib.Context(W, H, B) as ctx:
            env = rc.Env(ctx)
            hist = ctx.flow_history(4)
            try:
                got = []
                for i, f in enumerate(fields):
                    got.append(hist.push(f).tobytes())
                    if intervene and i in (1, 3, 4):
                        _run_all(ctx, env, t)
                        assert hist.pushes == i + 1
                outs.append(b"".join(got))
            finally:
                hist.close()
                env.close()
    assert outs[0] == outs[1]

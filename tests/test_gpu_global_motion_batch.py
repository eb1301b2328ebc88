"""The fused call of the global-motion branch (mav_global_motion_batch / _dev: frames in, records out) against the two calls it is made
of, ctx.farneback followed by global_motion_step on its output.  Equal bytes everywhere: no tolerance appears in this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(64, 64, 1), (97, 71, 3), (211, 97, 2), (160, 120, 2)]


def _lib():
    from mavflow import _lib
    return _lib


def frames_of(W, H, n, seed):
    """n + 1 frames (n + 1, H, W) u8: a smooth texture drifting and zooming slightly, with a patch moving against it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 6, 6)
    out = []
    for k in range(n + 1):
        z = 1.0 + 0.004 * k
        x, y = (xx - W / 2) / z + 0.6 * k, (yy - H / 2) / z - 0.3 * k
        img = 110 + 40 * np.sin(0.21 * x + ph[0]) * np.cos(0.17 * y + ph[1]) + 30 * np.sin(0.07 * x + 0.11 * y + ph[2]) + 25 * np.cos(0.33 * y + ph[3])
        px, py = W // 3 + 2 * k, H // 3 + k
        img[py:py + 14, px:px + 14] = 230 - 60 * np.sin(0.9 * xx[py:py + 14, px:px + 14] + ph[4])
        out.append(np.clip(np.around(img), 0, 255).astype(np.uint8))
    return np.stack(out)


def coords_of(W, H, n, seed):
    rng = np.random.default_rng(seed)
    return np.c_[rng.integers(3, W - 3, n), rng.integers(3, H - 3, n)]


def two_calls(ctx, prev, nxt, coords, optimize):
    """ctx.farneback, then global_motion_step on its output: dict(flow, H, ok, gray, results)."""
    lib = _lib()
    B = prev.shape[0]
    flow = np.array(ctx.farneback(prev, nxt))
    bufs = dict(flow=ctx.alloc(flow.nbytes).upload(flow), res=ctx.alloc(B * lib.MOTION_DTYPE.itemsize), H=ctx.alloc(72 * B), ok=ctx.alloc(4 * B),
                gray=ctx.alloc(ctx.W * ctx.H * B))
    ctx.global_motion_step(bufs["flow"].ptr, coords, B, bufs["res"].ptr, optimize=optimize, H_ptr=bufs["H"].ptr, ok_ptr=bufs["ok"].ptr,
                           gray_ptr=bufs["gray"].ptr)
    out = dict(flow=flow, H=bufs["H"].download(np.float64, (B, 3, 3)), ok=bufs["ok"].download(np.int32, (B,)),
               gray=bufs["gray"].download(np.uint8, (B, ctx.H, ctx.W)), results=bufs["res"].download(lib.MOTION_DTYPE, (B,)))
    for b in bufs.values():
        b.free()
    return out


def same(got, ref, keys, what):
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (what, k)


@pytest.mark.parametrize("window", ["box", "gaussian"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_fused_call_equals_farneback_then_step(size, window):
    W, H, B = size
    lib = _lib()
    run = frames_of(W, H, B, W + H)                       # B + 1 frames
    prev, nxt = run[:-1].copy(), run[1:].copy()           # two separate batches
    coords = coords_of(W, H, 150, W)
    with lib.Context(W, H, B, window=window) as ctx:
        for optimize in (False, True):
            ref = two_calls(ctx, prev, nxt, coords, optimize)
            assert ref["ok"].all() and ref["results"]["max_mag"].min() > 0
            got = ctx.global_motion_batch(prev, nxt, coords, optimize=optimize, outputs=("flow", "gray"))
            assert set(got) == {"results", "H", "ok", "flow", "gray"}
            same(got, ref, ("flow", "H", "ok", "gray", "results"), (size, window, optimize))
            # the frame-sequence layout: views of one run, next == prev + one frame
            seq = ctx.global_motion_batch(run[:-1], run[1:], coords, optimize=optimize, outputs=("flow", "gray"))
            same(seq, ref, ("flow", "H", "ok", "gray", "results"), (size, window, optimize, "sequence"))
            # every optional output NULL: the records alone, and the flow is where mav_last_flow_dev says
            res = np.empty(B, lib.MOTION_DTYPE)
            c32 = np.ascontiguousarray(coords, np.int32)
            lib.check(ctx.lib.mav_global_motion_batch(ctx.h, lib._ptr(prev), lib._ptr(nxt), lib._ptr(c32), len(c32), B, 1.5, int(optimize), None, None,
                                                      None, None, lib._ptr(res)))
            assert res.tobytes() == ref["results"].tobytes()
            assert all(ctx.last_flow(b).tobytes() == ref["flow"][b].tobytes() for b in range(B))
            bare = ctx.global_motion_batch(prev, nxt, coords, optimize=optimize)
            assert set(bare) == {"results", "H", "ok"}
            same(bare, ref, ("H", "ok", "results"), (size, window, optimize, "bare"))


@pytest.mark.parametrize("size", SIZES[1:3], ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_device_form_equals_farneback_then_step(size):
    W, H, B = size
    lib = _lib()
    run = frames_of(W, H, B, 3 * W)
    prev, nxt = run[:-1].copy(), run[1:].copy()
    coords = coords_of(W, H, 64, H)
    n0 = W * H
    with lib.Context(W, H, B) as ctx:
        d = dict(prev=ctx.alloc(B * n0).upload(prev), nxt=ctx.alloc(B * n0).upload(nxt), run=ctx.alloc((B + 1) * n0).upload(run),
                 flow=ctx.alloc(8 * n0 * B), res=ctx.alloc(B * lib.MOTION_DTYPE.itemsize), H=ctx.alloc(72 * B), ok=ctx.alloc(4 * B), gray=ctx.alloc(n0 * B))
        for optimize in (False, True):
            ref = two_calls(ctx, prev, nxt, coords, optimize)
            for name, (p, q) in dict(batches=(d["prev"].ptr, d["nxt"].ptr), sequence=(d["run"].ptr, d["run"].ptr + n0)).items():
                for buf in ("flow", "res", "H", "ok", "gray"):
                    d[buf].upload(np.full(d[buf].nbytes, 0xA5, np.uint8))
                ctx.global_motion_batch_dev(p, q, coords, B, d["res"].ptr, optimize=optimize, flow_ptr=d["flow"].ptr, H_ptr=d["H"].ptr,
                                            ok_ptr=d["ok"].ptr, gray_ptr=d["gray"].ptr)
                ctx.sync()
                got = dict(flow=d["flow"].download(np.float32, (B, H, W, 2)), H=d["H"].download(np.float64, (B, 3, 3)), ok=d["ok"].download(np.int32, (B,)),
                           gray=d["gray"].download(np.uint8, (B, H, W)), results=d["res"].download(lib.MOTION_DTYPE, (B,)))
                same(got, ref, ("flow", "H", "ok", "gray", "results"), (size, optimize, name))
            # optional outputs NULL
            d["res"].upload(np.full(d["res"].nbytes, 0xA5, np.uint8))
            ctx.global_motion_batch_dev(d["prev"].ptr, d["nxt"].ptr, coords, B, d["res"].ptr, optimize=optimize)
            ctx.sync()
            assert d["res"].download(lib.MOTION_DTYPE, (B,)).tobytes() == ref["results"].tobytes()
            assert ctx.last_flow(B - 1).tobytes() == ref["flow"][B - 1].tobytes()
        for buf in d.values():
            buf.free()


def test_collinear_coords_give_zero_records_and_no_error():
    W, H, B = 97, 71, 3
    lib = _lib()
    run = frames_of(W, H, B, 9)
    t = np.arange(20)
    coords = np.c_[3 * t + 5, 2 * t + 7]                   # on one line: no homography, whatever the flow
    with lib.Context(W, H, B) as ctx:
        got = ctx.global_motion_batch(run[:-1], run[1:], coords, optimize=True, outputs=("flow",))
        assert got["ok"].tolist() == [0] * B and not got["H"].any()
        assert got["results"].tobytes() == bytes(B * lib.MOTION_DTYPE.itemsize)
        assert got["flow"].tobytes() == np.array(ctx.farneback(run[:-1], run[1:])).tobytes()


def test_argument_errors_enqueue_nothing():
    W, H, B = 96, 80, 2                                   # 96x80 at scale 2.0: the 48x40 level has an integer ratio
    lib = _lib()
    run = frames_of(W, H, B, 4)
    prev, nxt = run[:-1].copy(), run[1:].copy()
    coords = np.ascontiguousarray(coords_of(W, H, 40, 1), np.int32)
    A = -1
    with lib.Context(W, H, B) as ctx:
        assert lib.load().mav_global_motion_batch(None, None, None, None, 4, 1, 1.5, 0, None, None, None, None, None) == A
        res = np.zeros(B, lib.MOTION_DTYPE)
        Hm, ok = np.zeros((B, 3, 3)), np.zeros(B, np.int32)
        n0 = W * H
        dev = dict(prev=ctx.alloc(B * n0).upload(prev), nxt=ctx.alloc(B * n0).upload(nxt), res=ctx.alloc(res.nbytes), flow=ctx.alloc(8 * n0 * B))
        sentinel = np.full(8 * n0 * B + res.nbytes, 0x5A, np.uint8)

        def host(prev=prev, nxt=nxt, coords=coords, n=len(coords), batch=B, scale=1.5, results=res):
            p = lib._ptr
            return ctx.lib.mav_global_motion_batch(ctx.h, p(prev), p(nxt), p(coords), n, batch, scale, 0, None, p(Hm), p(ok), None, p(results))

        def device(prev=dev["prev"].ptr, nxt=dev["nxt"].ptr, coords=coords, n=len(coords), batch=B, scale=1.5, results=dev["res"].ptr):
            return ctx.lib.mav_global_motion_batch_dev(ctx.h, prev, nxt, lib._ptr(coords), n, batch, scale, 0, dev["flow"].ptr, None, None, None, results)

        assert host() == 0 and device() == 0               # the good call, first: everything below differs from it in one argument
        ctx.sync()
        assert ok.all() and Hm.any()
        dev["flow"].upload(sentinel[:8 * n0 * B])
        dev["res"].upload(sentinel[:res.nbytes])
        outside = coords.copy()
        outside[7] = (W, 3)
        below = coords.copy()
        below[0] = (2, -1)
        bad = [dict(prev=None), dict(nxt=None), dict(coords=None), dict(results=None), dict(batch=0), dict(batch=B + 1), dict(n=3),
               dict(n=65537), dict(coords=outside), dict(coords=below), dict(scale=1.0), dict(scale=0.5), dict(scale=2.0)]
        for kw in bad:
            assert device(**kw) == A, kw
            assert b"mav_global_motion_batch_dev" in ctx.lib.mav_last_error() or b"pyramid" in ctx.lib.mav_last_error(), kw
        ctx.sync()                                         # nothing was enqueued: the device buffers hold what was put there
        assert dev["flow"].download(np.uint8, (8 * n0 * B,)).tobytes() == sentinel[:8 * n0 * B].tobytes()
        assert dev["res"].download(np.uint8, (res.nbytes,)).tobytes() == sentinel[:res.nbytes].tobytes()
        for kw in bad:
            res[:], Hm[:], ok[:] = 0, 0, 0
            assert host(**kw) == A, kw
            assert res.tobytes() == bytes(res.nbytes) and not Hm.any() and not ok.any(), kw
        with pytest.raises(ValueError):
            ctx.global_motion_batch(prev, nxt, coords, outputs=("warped",))
        with pytest.raises(ValueError):
            ctx.global_motion_batch(prev, nxt[:1], coords)
        with pytest.raises(ValueError):
            ctx.global_motion_batch(prev.astype(np.float32), nxt.astype(np.float32), coords)
        with pytest.raises(ValueError):
            ctx.global_motion_batch(prev, nxt, coords[:3])
        for b in dev.values():
            b.free()


def test_render_after_the_fused_call_equals_render_after_the_step():
    W, H, B = 97, 71, 3
    lib = _lib()
    run = frames_of(W, H, B, 21)
    coords = coords_of(W, H, 120, 2)
    with lib.Context(W, H, B) as ctx:
        flow = np.array(ctx.farneback(run[:-1], run[1:]))
        bufs = dict(flow=ctx.alloc(flow.nbytes).upload(flow), res=ctx.alloc(B * lib.MOTION_DTYPE.itemsize))
        ctx.global_motion_step(bufs["flow"].ptr, coords, B, bufs["res"].ptr)
        ref = ctx.render_last_global_motion(B)
        assert ref["warped"].any() and ref["global"].any()
        ctx.global_motion_batch(run[:-1], run[1:], coords, outputs=("gray",))
        got = ctx.render_last_global_motion(B)
        assert got["warped"].tobytes() == ref["warped"].tobytes() and got["global"].tobytes() == ref["global"].tobytes()
        assert set(ctx.render_last_global_motion(B, images=("warped",))) == {"warped"}
        ctx.global_motion_batch(run[:-1], run[1:], coords)            # no optional output: the context's own flow and matrix are resident
        got = ctx.render_last_global_motion(B)
        assert got["warped"].tobytes() == ref["warped"].tobytes() and got["global"].tobytes() == ref["global"].tobytes()
        bufs["run"] = ctx.alloc((B + 1) * W * H).upload(run)
        ctx.global_motion_batch_dev(bufs["run"].ptr, bufs["run"].ptr + W * H, coords, B, bufs["res"].ptr)
        got = ctx.render_last_global_motion(B)
        assert got["warped"].tobytes() == ref["warped"].tobytes() and got["global"].tobytes() == ref["global"].tobytes()
        with pytest.raises(lib.MavflowError):
            ctx.render_last_global_motion(B - 1)
        for b in bufs.values():
            b.free()

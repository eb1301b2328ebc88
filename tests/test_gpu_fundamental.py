"""The robust fundamental-matrix fit and the dense epipolar residual on the GPU (csrc/kernels_fundamental.hip and the calls around it)
against the numpy restatement tests/fundamental_ref.py at every case of tests/fundamental_cases.py: F, the mask, ok and every record field,
byte for byte, in the host and the _dev forms, the _dev forms also on pointers offset by one element into canary-filled blocks whose heads
and tails stay untouched, every item of a batch also alone, and every run once more on a second context.  The dense pass at
tests/warp_cases.py's frames, batch 1 and 3, with each output pointer NULL in turn.  No tolerance appears in this file."""
import ctypes as C

import numpy as np
import pytest

import fundamental_cases as T
import fundamental_ref as R
import warp_cases

pytestmark = pytest.mark.gpu
CANARY, TAIL = 0xA5, 64
W, H, B = 66, 33, 3
DENSE_FRAMES = ((1, 1), (2, 3), (5, 3), (37, 23), (131, 67))
assert set(DENSE_FRAMES) <= set(tuple(f) for f in warp_cases.FRAMES)


class _Dev:
    """caller-owned blocks of one context: an array uploaded `shift` bytes into a canary-filled block with a tail behind it"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a, shift):
        a = np.ascontiguousarray(a)
        raw = np.full(shift + a.nbytes + TAIL, CANARY, np.uint8)
        raw[shift:shift + a.nbytes] = a.view(np.uint8).ravel()
        b = self.ctx.alloc(raw.nbytes).upload(raw)
        self.bufs.append(b)
        return b, b.ptr + shift

    def blank(self, nbytes, shift):
        return self.put(np.full(nbytes, CANARY, np.uint8), shift)

    def get(self, b, shift, dtype, shape):
        raw = b.download(np.uint8, (b.nbytes,))
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert (raw[:shift] == CANARY).all() and (raw[shift + n:] == CANARY).all(), "the block's head or tail was written"
        return raw[shift:shift + n].view(dtype).reshape(shape).copy()

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _same(got, want, what):
    """got = (F, inliers, records) against the reference dict (or a slice of it), by bytes"""
    Fm, inl, rec = got
    assert Fm.shape == want["F"].shape and inl.shape == want["inliers"].shape and rec.shape == want["records"].shape, what
    bad = np.argwhere(Fm.view(np.uint64) != np.ascontiguousarray(want["F"]).view(np.uint64))
    assert len(bad) == 0, (what, "F", bad[:4].tolist(), Fm[tuple(bad[0])], want["F"][tuple(bad[0])])
    bad = np.argwhere(inl != want["inliers"])
    assert len(bad) == 0, (what, "inliers", len(bad), bad[:4].tolist())
    for f in R.RECORD_DTYPE.names:
        assert np.array_equal(rec[f].view(np.uint64 if f == "sq_error" else np.int32),
                              want["records"][f].view(np.uint64 if f == "sq_error" else np.int32)), (what, f, rec[f], want["records"][f])
    assert rec.tobytes() == np.ascontiguousarray(want["records"]).tobytes(), (what, "record bytes")


def _params(c, K):
    return K.fundamental_params(c.threshold, c.confidence, c.subsets.shape[1])


def _host(ctx, K, c, sl):
    from mavflow._lib import _ptr, check
    src, dst, sub = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.subsets))
    nb, n = src.shape[:2]
    Fm, inl, rec = np.full((nb, 3, 3), np.nan), np.full((nb, n), 7, np.uint8), np.zeros(nb, R.RECORD_DTYPE)
    p = _params(c, K)
    check(K.load().mav_find_fundamental(ctx.h, _ptr(src), _ptr(dst), n, nb, C.byref(p), _ptr(sub), _ptr(Fm), _ptr(inl), _ptr(rec)))
    return Fm, inl, rec


def _dev(ctx, K, c, sl, shifted):
    from mavflow._lib import check
    vp = lambda q: C.c_void_p(int(q))
    src, dst, sub = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.subsets))
    nb, n = src.shape[:2]
    p = _params(c, K)
    need = ctx.find_fundamental_workspace_bytes(n, nb, sub.shape[1])
    d = _Dev(ctx)
    try:
        s8, s4, s1, s16 = (8, 4, 1, 16) if shifted else (0, 0, 0, 0)
        _, ds = d.put(src, s8)
        _, dd = d.put(dst, s8)
        _, dt = d.put(sub, s4)
        bF, dF = d.blank(72 * nb, s8)
        bi, di = d.blank(nb * n, s1)
        br, dr = d.blank(32 * nb, s16)
        bw, dw = d.blank(need, s16)
        check(K.load().mav_find_fundamental_dev(ctx.h, vp(ds), vp(dd), n, nb, C.byref(p), vp(dt), vp(dF), vp(di), vp(dr), vp(dw), need))
        ctx.sync()
        d.get(bw, s16, np.uint8, (need,))                    # (the workspace's head and tail)
        return d.get(bF, s8, np.float64, (nb, 3, 3)), d.get(bi, s1, np.uint8, (nb, n)), d.get(br, s16, R.RECORD_DTYPE, (nb,))
    finally:
        d.close()


def _slice(want, sl):
    return {k: v[sl] for k, v in want.items()}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_device_equals_the_restatement(mav, name):
    from mavflow import _lib, fundamental as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    every = slice(0, nb)
    with _lib.Context(W, H, B) as ctx, _lib.Context(W + 3, H + 2, B) as other:
        if not c.dev_only:
            _same(_host(ctx, K, c, every), want, (name, "host"))
            _same(_host(other, K, c, every), want, (name, "host, second context"))
        else:
            from mavflow._lib import _ptr
            if name == "bad_subsets":                          # the host form refuses what the _dev form counts as invalid
                src, dst, sub = (np.ascontiguousarray(a) for a in (c.src, c.dst, c.subsets))
                out = np.zeros(128 * nb, np.uint8)
                p = _params(c, K)
                rc = K.load().mav_find_fundamental(ctx.h, _ptr(src), _ptr(dst), src.shape[1], nb, C.byref(p), _ptr(sub), _ptr(out), _ptr(out), _ptr(out))
                assert rc == _lib.MAV_ERR_ARG and not out.any()
        _same(_dev(ctx, K, c, every, False), want, (name, "_dev"))
        _same(_dev(ctx, K, c, every, True), want, (name, "_dev, offset pointers"))
        _same(_dev(other, K, c, every, True), want, (name, "_dev, second context"))
        if nb > 1:
            for b in range(nb):                                 # every item alone: the bytes do not depend on the batch position
                _same(_dev(other, K, c, slice(b, b + 1), False), _slice(want, slice(b, b + 1)), (name, "alone", b))


def test_python_members_return_the_restatements_fields(mav):
    from mavflow import _lib
    c, want = T.BY_NAME["n65_it65_b3"], T.reference("n65_it65_b3")
    with _lib.Context(W, H, B) as ctx:
        out = ctx.find_fundamental(c.src, c.dst, subsets=c.subsets)
        _same((out["F"], out["inliers"], out["records"]), want, "Context.find_fundamental")
        assert np.array_equal(out["ok"], want["records"]["ok"]) and np.array_equal(out["inliers_count"], want["records"]["inliers"])
        one = ctx.find_fundamental(c.src[1], c.dst[1], subsets=c.subsets[1])
        assert one["F"].shape == (3, 3) and one["inliers"].shape == (c.src.shape[1],) and isinstance(one["ok"], int)
        assert one["F"].tobytes() == want["F"][1].tobytes() and one["best_iter"] == want["records"]["best_iter"][1]
        assert one["best_slot"] == want["records"]["best_slot"][1]
        drawn = ctx.find_fundamental(c.src[0], c.dst[0], max_iters=100, rng=9)
        again = ctx.find_fundamental(c.src[0], c.dst[0], subsets=T.subsets_for(9, c.src.shape[1], 100, 1)[0])
        assert drawn["F"].tobytes() == again["F"].tobytes() and drawn["ok"] == 1


@pytest.mark.parametrize("frame", T.FLOW_FRAMES)
@pytest.mark.parametrize("nb", (1, 3))
def test_flow_form(mav, frame, nb):
    from mavflow import _lib, fundamental as K
    from mavflow._lib import _ptr, check
    w, h = frame
    flow, coords, sub = T.flow_case(w, h, nb)
    src, dst = R.flow_pairs(flow, coords)
    want = R.find(src, dst, sub, threshold=0.5)
    assert np.all(want["records"]["ok"] == 1) and np.all(want["records"]["inliers"] >= 60)
    n = coords.shape[0]
    vp = lambda q: C.c_void_p(int(q))
    for ctx_no in (0, 1):
        with _lib.Context(w, h, B) as ctx:
            out = ctx.flow_fundamental(flow, coords, threshold=0.5, subsets=sub, want_pairs=True)
            _same((out["F"], out["inliers"], out["records"]), want, (frame, nb, "host", ctx_no))
            assert out["pairs_dst"].tobytes() == dst.tobytes()
            p = K.fundamental_params(threshold=0.5, max_iters=sub.shape[1])
            need = ctx.find_fundamental_workspace_bytes(n, nb, sub.shape[1])
            d = _Dev(ctx)
            try:
                _, df = d.put(flow, 8)
                _, dt = d.put(sub, 4)
                bF, dF = d.blank(72 * nb, 8)
                bi, di = d.blank(nb * n, 1)
                br, dr = d.blank(32 * nb, 16)
                bw, dw = d.blank(need, 16)
                check(K.load().mav_flow_fundamental_dev(ctx.h, vp(df), _ptr(coords), n, nb, C.byref(p), vp(dt), vp(dF), vp(di), vp(dr), vp(dw), need))
                ctx.sync()
                d.get(bw, 16, np.uint8, (need,))
                got = d.get(bF, 8, np.float64, (nb, 3, 3)), d.get(bi, 1, np.uint8, (nb, n)), d.get(br, 16, R.RECORD_DTYPE, (nb,))
                _same(got, want, (frame, nb, "_dev", ctx_no))
                # the fit feeds the dense pass without the host: F is read where the fit wrote it
                want_epi = R.epipolar_residual(flow, want["F"], 1.0)
                bres, dres = d.blank(4 * nb * w * h, 4)
                bm, dm = d.blank(nb * w * h, 1)
                be, de = d.blank(32 * nb, 16)
                ctx.epipolar_residual_enqueue(df, dF, nb, dres, dm, de, threshold=1.0)
                ctx.sync()
                _same_epi((d.get(bres, 4, np.float32, (nb, h, w)), d.get(bm, 1, np.uint8, (nb, h, w)), d.get(be, 16, R.EPI_DTYPE, (nb,))), want_epi,
                          (frame, nb, "fit -> residual", ctx_no))
                outside = coords.copy()
                outside[3] = (w, 0)
                rc = K.load().mav_flow_fundamental_dev(ctx.h, vp(df), _ptr(outside), n, nb, C.byref(p), vp(dt), vp(dF), vp(di), vp(dr), vp(dw), need)
                assert rc == _lib.MAV_ERR_ARG and b"mav_flow_fundamental_dev:" in K.load().mav_last_error()
            finally:
                d.close()


# ---- the dense pass ------------------------------------------------------------------------------------------------------------------------
def _same_epi(got, want, what):
    """got = (residual | None, mask | None, records) against the restatement's dict, by bytes"""
    res, mask, rec = got
    if res is not None:
        bad = np.argwhere(res.view(np.uint32) != want["residual"].view(np.uint32))
        assert len(bad) == 0, (what, "residual", len(bad), bad[:4].tolist(), res[tuple(bad[0])], want["residual"][tuple(bad[0])])
    if mask is not None:
        bad = np.argwhere(mask != want["mask"])
        assert len(bad) == 0, (what, "mask", len(bad), bad[:4].tolist())
    for f in ("max_residual", "max_row", "max_col", "movers", "not_finite"):
        assert rec[f].tobytes() == want["records"][f].tobytes(), (what, f, rec[f], want["records"][f])
    assert rec.tobytes() == want["records"].tobytes(), (what, "record bytes")


def _dense_inputs(w, h, nb, kind):
    flow, _ = T.dense_scene(w, h, nb)
    Fm = np.stack([T.true_F(np.array([[100.0, 0, (w - 1) / 2], [0, 100.0, (h - 1) / 2], [0, 0, 1]]), *T.pose(b)) for b in range(nb)])
    if kind == "zero_F":
        Fm = np.zeros_like(Fm)
    elif kind == "non_finite":
        flow = flow.copy()
        flat = flow.reshape(nb, -1)
        flat[:, 0] = np.nan
        flat[:, -1] = np.inf
        if flat.shape[1] > 8:
            flat[:, 5], flat[:, 8] = -np.inf, 3e38
    elif kind == "tie":                                        # a constant field under a pure sideways translation: F = [t]x, every residual
        flow = np.zeros_like(flow)                             # is |v| exactly; two equal maxima, the first in raster order wins
        flow[..., 1] = 0.25
        flat = flow.reshape(nb, -1, 2)
        flat[:, -1, 1] = 4.0
        flat[:, (w * h) // 2, 1] = 4.0
        Fm = np.tile(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.5], [0.0, 0.5, 0.0]]), (nb, 1, 1))
    return flow, Fm


@pytest.mark.parametrize("frame", DENSE_FRAMES)
@pytest.mark.parametrize("kind", ("scene", "zero_F", "non_finite", "tie"))
def test_dense_pass_equals_the_restatement(mav, frame, kind):
    from mavflow import _lib
    w, h = frame
    with _lib.Context(w, h, B) as ctx:
        for nb in (1, 3):
            flow, Fm = _dense_inputs(w, h, nb, kind)
            want = R.epipolar_residual(flow, Fm, 1.0)
            if kind == "zero_F":
                assert not want["residual"].any() and not want["mask"].any() and np.all(want["records"]["not_finite"] == w * h)
            if kind == "tie" and w * h > 2:
                assert np.all(want["records"]["max_residual"] == 4.0) and np.all(want["records"]["max_row"] * w + want["records"]["max_col"] == (w * h) // 2)
            out = ctx.epipolar_residual(flow, Fm, 1.0)
            _same_epi((out["residual"], out["mask"], out["records"]), want, (frame, kind, nb, "host"))
            for outputs in (("residual",), ("mask",), ()):     # each output pointer NULL in turn; the record does not depend on them
                out = ctx.epipolar_residual(flow, Fm, 1.0, outputs=outputs)
                assert set(out) & {"residual", "mask"} == set(outputs)
                _same_epi((out.get("residual"), out.get("mask"), out["records"]), want, (frame, kind, nb, outputs))
            d = _Dev(ctx)
            try:
                _, df = d.put(flow, 4)
                _, dF = d.put(Fm, 8)
                for res_on, mask_on in ((True, True), (False, True), (True, False)):
                    bres, dres = d.blank(4 * nb * w * h, 4)
                    bm, dm = d.blank(nb * w * h, 1)
                    be, de = d.blank(32 * nb, 16)
                    ctx.epipolar_residual_enqueue(df, dF, nb, dres if res_on else None, dm if mask_on else None, de, threshold=1.0)
                    ctx.sync()
                    res, mask = d.get(bres, 4, np.float32, (nb, h, w)), d.get(bm, 1, np.uint8, (nb, h, w))
                    if not res_on:
                        assert (res.view(np.uint8) == CANARY).all()
                    if not mask_on:
                        assert (mask == CANARY).all()
                    _same_epi((res if res_on else None, mask if mask_on else None, d.get(be, 16, R.EPI_DTYPE, (nb,))), want,
                              (frame, kind, nb, "_dev", res_on, mask_on))
            finally:
                d.close()


# ---- past the caps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.CAP_CASES])
def test_device_equals_the_restatement_under_a_capped_score_grid(mav, name):
    """batch 16 on a context of max_batch 16: k_fm_score's grid is FM_GRID_CAP / 16 workgroups per item, its slots' counts written (and,
    at n = FM_CHUNK + 1, added to) under the longer stride; the _late cases' winners are among the last slots"""
    from mavflow import _lib, fundamental as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    assert nb == T.CAP_BATCH and T.score_grid(c.subsets.shape[1], nb) == "capped"
    every = slice(0, nb)
    with _lib.Context(W, H, T.CAP_BATCH) as ctx:
        _same(_host(ctx, K, c, every), want, (name, "host"))
        _same(_dev(ctx, K, c, every, False), want, (name, "_dev"))
        _same(_dev(ctx, K, c, every, True), want, (name, "_dev, offset pointers"))


@pytest.mark.parametrize("kind", ("noise", "zero_F"))
def test_dense_pass_equals_the_restatement_past_the_cap(mav, kind):
    """397 x 331 at batch 2: the second trip of k_epipolar_residual's loop -- the last 335 pixels written, the key and both counts carried
    across trips into the wave reduction and the atomics"""
    from mavflow import _lib
    (w, h), nb = T.EPI_FRAME, T.EPI_BATCH
    flow, Fm, t, want = T.epi_cap_reference(kind)
    with _lib.Context(w, h, nb) as ctx:
        out = ctx.epipolar_residual(flow, Fm, t)
        _same_epi((out["residual"], out["mask"], out["records"]), want, (kind, "host"))
        for outputs in (("residual",), ("mask",), ()):
            out = ctx.epipolar_residual(flow, Fm, t, outputs=outputs)
            assert set(out) & {"residual", "mask"} == set(outputs)
            _same_epi((out.get("residual"), out.get("mask"), out["records"]), want, (kind, outputs))
        d = _Dev(ctx)
        try:
            _, df = d.put(flow, 4)
            _, dF = d.put(Fm, 8)
            for res_on, mask_on in ((True, True), (False, True), (True, False), (False, False)):
                bres, dres = d.blank(4 * nb * w * h, 4)
                bm, dm = d.blank(nb * w * h, 1)
                be, de = d.blank(32 * nb, 16)
                ctx.epipolar_residual_enqueue(df, dF, nb, dres if res_on else None, dm if mask_on else None, de, threshold=t)
                ctx.sync()
                res, mask = d.get(bres, 4, np.float32, (nb, h, w)), d.get(bm, 1, np.uint8, (nb, h, w))
                if not res_on:
                    assert (res.view(np.uint8) == CANARY).all()
                if not mask_on:
                    assert (mask == CANARY).all()
                _same_epi((res if res_on else None, mask if mask_on else None, d.get(be, 16, R.EPI_DTYPE, (nb,))), want, (kind, "_dev", res_on, mask_on))
        finally:
            d.close()

"""The robust essential-matrix fit on the GPU (csrc/kernels_essential.hip and the calls around it) against the numpy restatement
tests/essential_ref.py at every case of tests/essential_cases.py: E, F, the mask, ok and every record field, byte for byte, in the host
and the _dev forms, the _dev forms also on pointers offset by one element into canary-filled blocks whose heads and tails stay untouched,
every item of a batch also alone, and every run once more on a second context.  The flow forms at two frames, batch 1 and 3, and the
fit's F read by the dense epipolar pass where the fit wrote it.  Refused arguments leave canaries intact.  No tolerance appears in this
file."""
import ctypes as C

import numpy as np
import pytest

import essential_cases as T
import essential_ref as R
import fundamental_ref as FR

pytestmark = pytest.mark.gpu
CANARY, TAIL = 0xA5, 64
W, H, B = 66, 33, 3


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
    """got = (E, F, inliers, records) against the reference dict (or a slice of it), by bytes"""
    E, Fm, inl, rec = got
    assert E.shape == want["E"].shape and inl.shape == want["inliers"].shape and rec.shape == want["records"].shape, what
    for name, m in (("E", E), ("F", Fm)):
        bad = np.argwhere(m.view(np.uint64) != np.ascontiguousarray(want[name]).view(np.uint64))
        assert len(bad) == 0, (what, name, bad[:4].tolist(), m[tuple(bad[0])], want[name][tuple(bad[0])])
    bad = np.argwhere(inl != want["inliers"])
    assert len(bad) == 0, (what, "inliers", len(bad), bad[:4].tolist())
    for f in R.RECORD_DTYPE.names:
        assert np.array_equal(rec[f].view(np.uint64 if f == "sq_error" else np.int32),
                              want["records"][f].view(np.uint64 if f == "sq_error" else np.int32)), (what, f, rec[f], want["records"][f])
    assert rec.tobytes() == np.ascontiguousarray(want["records"]).tobytes(), (what, "record bytes")


def _params(c, K):
    return K.essential_params(c.threshold, c.confidence, c.subsets.shape[1], c.camera)


def _host(ctx, K, c, sl):
    from mavflow._lib import _ptr, check
    src, dst, sub = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.subsets))
    nb, n = src.shape[:2]
    E, Fm, inl, rec = np.full((nb, 3, 3), np.nan), np.full((nb, 3, 3), np.nan), np.full((nb, n), 7, np.uint8), np.zeros(nb, R.RECORD_DTYPE)
    p = _params(c, K)
    check(K.load().mav_find_essential(ctx.h, _ptr(src), _ptr(dst), n, nb, C.byref(p), _ptr(sub), _ptr(E), _ptr(Fm), _ptr(inl), _ptr(rec)))
    return E, Fm, inl, rec


def _dev(ctx, K, c, sl, shifted):
    from mavflow._lib import check
    vp = lambda q: C.c_void_p(int(q))
    src, dst, sub = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.subsets))
    nb, n = src.shape[:2]
    p = _params(c, K)
    need = ctx.find_essential_workspace_bytes(n, nb, sub.shape[1])
    d = _Dev(ctx)
    try:
        s8, s4, s1, s16 = (8, 4, 1, 16) if shifted else (0, 0, 0, 0)
        _, ds = d.put(src, s8)
        _, dd = d.put(dst, s8)
        _, dt = d.put(sub, s4)
        bE, dE = d.blank(72 * nb, s8)
        bF, dF = d.blank(72 * nb, s8)
        bi, di = d.blank(nb * n, s1)
        br, dr = d.blank(32 * nb, s16)
        bw, dw = d.blank(need, s16)
        check(K.load().mav_find_essential_dev(ctx.h, vp(ds), vp(dd), n, nb, C.byref(p), vp(dt), vp(dE), vp(dF), vp(di), vp(dr), vp(dw), need))
        ctx.sync()
        d.get(bw, s16, np.uint8, (need,))                    # (the workspace's head and tail)
        return (d.get(bE, s8, np.float64, (nb, 3, 3)), d.get(bF, s8, np.float64, (nb, 3, 3)), d.get(bi, s1, np.uint8, (nb, n)),
                d.get(br, s16, R.RECORD_DTYPE, (nb,)))
    finally:
        d.close()


def _slice(want, sl):
    return {k: v[sl] for k, v in want.items()}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_device_equals_the_restatement(mav, name):
    from mavflow import _lib, essential as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    every = slice(0, nb)
    with _lib.Context(W, H, B) as ctx, _lib.Context(W + 3, H + 2, B) as other:
        if not c.dev_only:
            _same(_host(ctx, K, c, every), want, (name, "host"))
            _same(_host(other, K, c, every), want, (name, "host, second context"))
        elif name == "bad_subsets":                            # the host form refuses what the _dev form counts as invalid
            from mavflow._lib import _ptr
            src, dst, sub = (np.ascontiguousarray(a) for a in (c.src, c.dst, c.subsets))
            out = np.zeros(128 * nb, np.uint8)
            p = _params(c, K)
            rc = K.load().mav_find_essential(ctx.h, _ptr(src), _ptr(dst), src.shape[1], nb, C.byref(p), _ptr(sub), _ptr(out), _ptr(out), _ptr(out),
                                             _ptr(out))
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
        out = ctx.find_essential(c.src, c.dst, subsets=c.subsets, camera=c.camera)
        _same((out["E"], out["F"], out["inliers"], out["records"]), want, "Context.find_essential")
        assert np.array_equal(out["ok"], want["records"]["ok"]) and np.array_equal(out["inliers_count"], want["records"]["inliers"])
        one = ctx.find_essential(c.src[1], c.dst[1], subsets=c.subsets[1], camera=c.camera)
        assert one["E"].shape == (3, 3) and one["F"].shape == (3, 3) and one["inliers"].shape == (c.src.shape[1],) and isinstance(one["ok"], int)
        assert one["E"].tobytes() == want["E"][1].tobytes() and one["best_iter"] == want["records"]["best_iter"][1]
        assert one["best_slot"] == want["records"]["best_slot"][1] and 0 <= one["best_slot"] <= 9
        drawn = ctx.find_essential(c.src[0], c.dst[0], max_iters=100, rng=9, camera=c.camera)
        again = ctx.find_essential(c.src[0], c.dst[0], subsets=T.subsets_for(9, c.src.shape[1], 100, 1)[0], camera=c.camera)
        assert drawn["E"].tobytes() == again["E"].tobytes() and drawn["ok"] == 1


@pytest.mark.parametrize("frame", T.FLOW_FRAMES)
@pytest.mark.parametrize("nb", (1, 3))
def test_flow_form(mav, frame, nb):
    from mavflow import _lib, essential as K
    from mavflow._lib import _ptr, check
    w, h = frame
    flow, coords, sub, cam = T.flow_case(w, h, nb)
    src, dst = FR.flow_pairs(flow, coords)
    want = R.find(src, dst, sub, threshold=0.5, camera=cam)
    assert np.all(want["records"]["ok"] == 1) and np.all(want["records"]["inliers"] >= 60)
    n = coords.shape[0]
    vp = lambda q: C.c_void_p(int(q))
    for ctx_no in (0, 1):
        with _lib.Context(w, h, B) as ctx:
            out = ctx.flow_essential(flow, coords, threshold=0.5, subsets=sub, camera=cam, want_pairs=True)
            _same((out["E"], out["F"], out["inliers"], out["records"]), want, (frame, nb, "host", ctx_no))
            assert out["pairs_dst"].tobytes() == dst.tobytes()
            p = K.essential_params(threshold=0.5, max_iters=sub.shape[1], camera=cam)
            need = ctx.find_essential_workspace_bytes(n, nb, sub.shape[1])
            d = _Dev(ctx)
            try:
                _, df = d.put(flow, 8)
                _, dt = d.put(sub, 4)
                bE, dE = d.blank(72 * nb, 8)
                bF, dF = d.blank(72 * nb, 8)
                bi, di = d.blank(nb * n, 1)
                br, dr = d.blank(32 * nb, 16)
                bw, dw = d.blank(need, 16)
                check(K.load().mav_flow_essential_dev(ctx.h, vp(df), _ptr(coords), n, nb, C.byref(p), vp(dt), vp(dE), vp(dF), vp(di), vp(dr), vp(dw), need))
                ctx.sync()
                d.get(bw, 16, np.uint8, (need,))
                got = (d.get(bE, 8, np.float64, (nb, 3, 3)), d.get(bF, 8, np.float64, (nb, 3, 3)), d.get(bi, 1, np.uint8, (nb, n)),
                       d.get(br, 16, R.RECORD_DTYPE, (nb,)))
                _same(got, want, (frame, nb, "_dev", ctx_no))
                # the fit feeds the dense pass without the host: F is read where the fit wrote it
                want_epi = FR.epipolar_residual(flow, want["F"], 1.0)
                bres, dres = d.blank(4 * nb * w * h, 4)
                bm, dm = d.blank(nb * w * h, 1)
                be, de = d.blank(32 * nb, 16)
                ctx.epipolar_residual_enqueue(df, dF, nb, dres, dm, de, threshold=1.0)
                ctx.sync()
                res, mask, rec = d.get(bres, 4, np.float32, (nb, h, w)), d.get(bm, 1, np.uint8, (nb, h, w)), d.get(be, 16, FR.EPI_DTYPE, (nb,))
                assert res.tobytes() == want_epi["residual"].tobytes() and mask.tobytes() == want_epi["mask"].tobytes(), (frame, nb, "fit -> residual")
                assert rec.tobytes() == want_epi["records"].tobytes(), (frame, nb, "fit -> residual, records")
                outside = coords.copy()
                outside[3] = (w, 0)
                rc = K.load().mav_flow_essential_dev(ctx.h, vp(df), _ptr(outside), n, nb, C.byref(p), vp(dt), vp(dE), vp(dF), vp(di), vp(dr), vp(dw), need)
                assert rc == _lib.MAV_ERR_ARG and b"mav_flow_essential_dev:" in K.load().mav_last_error()
            finally:
                d.close()


def _refusals(K, n, mi):
    """(what, params, n, workspace shortfall, pointer to misalign) of calls the _dev form must refuse"""
    P = K.essential_params
    return [("n below 5", P(max_iters=mi), 4, 0, None), ("max_iters 0", P(max_iters=0), n, 0, None),
            ("max_iters above the maximum", P(max_iters=K.ESSENTIAL_MAX_ITERS + 1), n, 0, None),
            ("negative threshold", P(threshold=-1.0, max_iters=mi), n, 0, None), ("NaN threshold", P(threshold=np.nan, max_iters=mi), n, 0, None),
            ("confidence 1", P(confidence=1.0, max_iters=mi), n, 0, None), ("confidence 0", P(confidence=0.0, max_iters=mi), n, 0, None),
            ("fx 0", P(max_iters=mi, camera=(0.0, 1.0, 0.0, 0.0)), n, 0, None), ("fy negative", P(max_iters=mi, camera=(1.0, -2.0, 0.0, 0.0)), n, 0, None),
            ("fx infinite", P(max_iters=mi, camera=(np.inf, 1.0, 0.0, 0.0)), n, 0, None), ("fy NaN", P(max_iters=mi, camera=(1.0, np.nan, 0.0, 0.0)), n, 0, None),
            ("cx NaN", P(max_iters=mi, camera=(1.0, 1.0, np.nan, 0.0)), n, 0, None), ("cy infinite", P(max_iters=mi, camera=(1.0, 1.0, 0.0, np.inf)), n, 0, None),
            ("short workspace", P(max_iters=mi), n, 1, None), ("src off by 4", P(max_iters=mi), n, 0, "src"), ("E off by 4", P(max_iters=mi), n, 0, "E"),
            ("F off by 4", P(max_iters=mi), n, 0, "F"), ("records off by 8", P(max_iters=mi), n, 0, "records"), ("subsets off by 2", P(max_iters=mi), n, 0, "subsets")]


def test_refused_arguments_leave_canaries_intact(mav):
    from mavflow import _lib, essential as K
    c = T.BY_NAME["n65_it65_b3"]
    src, dst, sub = c.src[:1], c.dst[:1], c.subsets[:1]
    n, mi = src.shape[1], sub.shape[1]
    vp = lambda q: C.c_void_p(int(q))
    with _lib.Context(W, H, B) as ctx:
        need = ctx.find_essential_workspace_bytes(n, 1, mi)
        d = _Dev(ctx)
        try:
            _, ds = d.put(src, 0)
            _, dd = d.put(dst, 0)
            _, dt = d.put(sub, 0)
            outs = dict(E=d.blank(72, 0), F=d.blank(72, 0), inliers=d.blank(n, 0), records=d.blank(32, 0), ws=d.blank(need, 0))
            ptr = dict(src=ds, dst=dd, subsets=dt, **{k: v[1] for k, v in outs.items()})
            for what, p, nn, short, off in _refusals(K, n, mi):
                q = dict(ptr)
                if off:
                    q[off] += {"src": 4, "E": 4, "F": 4, "records": 8, "subsets": 2}[off]
                rc = K.load().mav_find_essential_dev(ctx.h, vp(q["src"]), vp(q["dst"]), nn, 1, C.byref(p), vp(q["subsets"]), vp(q["E"]), vp(q["F"]),
                                                     vp(q["inliers"]), vp(q["records"]), vp(q["ws"]), need - short)
                assert rc == _lib.MAV_ERR_ARG, what
                assert b"mav_find_essential_dev:" in K.load().mav_last_error(), what
            for k in ("E", "F", "inliers", "records", "ws"):
                rc = K.load().mav_find_essential_dev(ctx.h, vp(ds), vp(dd), n, 1, C.byref(K.essential_params(max_iters=mi)), vp(dt),
                                                     *[None if j == k else vp(ptr[j]) for j in ("E", "F", "inliers", "records", "ws")], need)
                assert rc == _lib.MAV_ERR_ARG, ("NULL", k)
            assert ctx.find_essential_workspace_bytes(n, 1, mi) == need
            with pytest.raises(_lib.MavflowError):
                ctx.find_essential_workspace_bytes(4, 1, mi)
            ctx.sync()
            for k, (b, _) in outs.items():                      # nothing was enqueued, nothing written
                assert (b.download(np.uint8, (b.nbytes,)) == CANARY).all(), k
        finally:
            d.close()


# ---- past the score kernel's grid cap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.CAP_CASES])
def test_device_equals_the_restatement_under_a_capped_score_grid(mav, name):
    """batch 16 on a context of max_batch 16: k_em_score's grid is EM_GRID_CAP / 16 workgroups per item, its counts written (and, at n = CHUNK + 1,
    added to) under the longer stride; the _late cases' winners are among the last hypotheses"""
    from mavflow import _lib, essential as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    assert nb == T.CAP_BATCH and T.score_grid(c[3].shape[1], nb) == "capped"
    every = slice(0, nb)
    with _lib.Context(W, H, T.CAP_BATCH) as ctx:
        _same(_host(ctx, K, c, every), want, (name, "host"))
        _same(_dev(ctx, K, c, every, False), want, (name, "_dev"))
        _same(_dev(ctx, K, c, every, True), want, (name, "_dev, offset pointers"))

"""The robust affine fit on the GPU (csrc/kernels_affine.hip and the calls around it) against the numpy restatement tests/affine_ref.py at
every case of tests/affine_cases.py: M, the mask, ok and every record field, byte for byte, in the host and the _dev forms, the _dev
forms also on pointers offset by one element into canary-filled blocks whose heads and tails stay untouched, every item of a batch also
alone, and every run once more on a second context.  No tolerance appears in this file."""
import ctypes as C

import numpy as np
import pytest

import affine_cases as T
import affine_ref as R

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
    """got = (M, inliers, records) against the reference dict (or a slice of it), by bytes"""
    M, inl, rec = got
    assert M.shape == want["M"].shape and inl.shape == want["inliers"].shape and rec.shape == want["records"].shape, what
    bad = np.argwhere(M.view(np.uint64) != np.ascontiguousarray(want["M"]).view(np.uint64))
    assert len(bad) == 0, (what, "M", bad[:4].tolist(), M[tuple(bad[0])], want["M"][tuple(bad[0])])
    bad = np.argwhere(inl != want["inliers"])
    assert len(bad) == 0, (what, "inliers", len(bad), bad[:4].tolist())
    for f in R.RECORD_DTYPE.names:
        assert np.array_equal(rec[f].view(np.uint64 if f == "sq_error" else np.int32),
                              want["records"][f].view(np.uint64 if f == "sq_error" else np.int32)), (what, f, rec[f], want["records"][f])
    assert rec.tobytes() == np.ascontiguousarray(want["records"]).tobytes(), (what, "record bytes")


def _params(c, K):
    return K.affine_params(c.threshold, c.triples.shape[1], c.confidence, bool(c.refine))


def _host(ctx, K, c, sl):
    from mavflow._lib import _ptr, check
    src, dst, tri = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.triples))
    nb, n = src.shape[:2]
    M, inl, rec = np.full((nb, 2, 3), np.nan), np.full((nb, n), 7, np.uint8), np.zeros(nb, R.RECORD_DTYPE)
    p = _params(c, K)
    check(K.load().mav_estimate_affine(ctx.h, _ptr(src), _ptr(dst), n, nb, C.byref(p), _ptr(tri), _ptr(M), _ptr(inl), _ptr(rec)))
    return M, inl, rec


def _dev(ctx, K, c, sl, shifted):
    from mavflow._lib import check
    vp = lambda q: C.c_void_p(int(q))
    src, dst, tri = (np.ascontiguousarray(a[sl]) for a in (c.src, c.dst, c.triples))
    nb, n = src.shape[:2]
    p = _params(c, K)
    need = ctx.estimate_affine_workspace_bytes(n, nb, tri.shape[1])
    d = _Dev(ctx)
    try:
        s8, s4, s1, s16 = (8, 4, 1, 16) if shifted else (0, 0, 0, 0)
        _, ds = d.put(src, s8)
        _, dd = d.put(dst, s8)
        _, dt = d.put(tri, s4)
        bM, dM = d.blank(48 * nb, s8)
        bi, di = d.blank(nb * n, s1)
        br, dr = d.blank(32 * nb, s16)
        bw, dw = d.blank(need, s16)
        check(K.load().mav_estimate_affine_dev(ctx.h, vp(ds), vp(dd), n, nb, C.byref(p), vp(dt), vp(dM), vp(di), vp(dr), vp(dw), need))
        ctx.sync()
        d.get(bw, s16, np.uint8, (need,))                    # (the workspace's head and tail)
        return d.get(bM, s8, np.float64, (nb, 2, 3)), d.get(bi, s1, np.uint8, (nb, n)), d.get(br, s16, R.RECORD_DTYPE, (nb,))
    finally:
        d.close()


def _slice(want, sl):
    return {k: v[sl] for k, v in want.items()}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_device_equals_the_restatement(mav, name):
    from mavflow import _lib, affine as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    every = slice(0, nb)
    with _lib.Context(W, H, B) as ctx, _lib.Context(W + 3, H + 2, B) as other:
        if not c.dev_only:
            _same(_host(ctx, K, c, every), want, (name, "host"))
            _same(_host(other, K, c, every), want, (name, "host, second context"))
        else:
            from mavflow._lib import _ptr
            if name == "bad_triples":                          # the host form refuses what the _dev form counts as invalid
                src, dst, tri = (np.ascontiguousarray(a) for a in (c.src, c.dst, c.triples))
                out = np.zeros(64 * nb, np.uint8)
                p = _params(c, K)
                rc = K.load().mav_estimate_affine(ctx.h, _ptr(src), _ptr(dst), src.shape[1], nb, C.byref(p), _ptr(tri), _ptr(out), _ptr(out), _ptr(out))
                assert rc == _lib.MAV_ERR_ARG and not out.any()
        _same(_dev(ctx, K, c, every, False), want, (name, "_dev"))
        _same(_dev(ctx, K, c, every, True), want, (name, "_dev, offset pointers"))
        _same(_dev(other, K, c, every, True), want, (name, "_dev, second context"))
        if nb > 1:
            for b in range(nb):                                 # every item alone: the bytes do not depend on the batch position
                _same(_dev(other, K, c, slice(b, b + 1), False), _slice(want, slice(b, b + 1)), (name, "alone", b))


def test_python_members_return_the_restatements_fields(mav):
    from mavflow import _lib
    c, want = T.BY_NAME["noisy_refine1"], T.reference("noisy_refine1")
    with _lib.Context(W, H, B) as ctx:
        out = ctx.estimate_affine(c.src, c.dst, triples=c.triples)
        _same((out["M"], out["inliers"], out["records"]), want, "Context.estimate_affine")
        assert np.array_equal(out["ok"], want["records"]["ok"]) and np.array_equal(out["inliers_count"], want["records"]["inliers"])
        one = ctx.estimate_affine(c.src[1], c.dst[1], triples=c.triples[1], refine=True)
        assert one["M"].shape == (2, 3) and one["inliers"].shape == (c.src.shape[1],) and isinstance(one["ok"], int)
        assert one["M"].tobytes() == want["M"][1].tobytes() and one["best_iter"] == want["records"]["best_iter"][1]
        drawn = ctx.estimate_affine(c.src[0], c.dst[0], max_iters=100, rng=9)
        again = ctx.estimate_affine(c.src[0], c.dst[0], triples=T.triples_for(9, c.src.shape[1], 100, 1)[0])
        assert drawn["M"].tobytes() == again["M"].tobytes() and drawn["ok"] == 1


@pytest.mark.parametrize("frame", T.FLOW_FRAMES)
@pytest.mark.parametrize("nb", (1, 3))
def test_flow_form(mav, frame, nb):
    from mavflow import _lib, affine as K
    from mavflow._lib import _ptr, check
    w, h = frame
    flow, coords, tri = T.flow_case(w, h, nb)
    src, dst = R.flow_pairs(flow, coords)
    want = R.estimate(src, dst, tri)
    assert np.all(want["records"]["ok"] == 1) and np.all(want["records"]["inliers"] >= 30)
    n = coords.shape[0]
    vp = lambda q: C.c_void_p(int(q))
    for ctx_no in (0, 1):
        with _lib.Context(w, h, B) as ctx:
            out = ctx.flow_affine(flow, coords, triples=tri, want_pairs=True)
            _same((out["M"], out["inliers"], out["records"]), want, (frame, nb, "host", ctx_no))
            assert out["pairs_dst"].tobytes() == dst.tobytes()
            p = K.affine_params(max_iters=tri.shape[1])
            need = ctx.estimate_affine_workspace_bytes(n, nb, tri.shape[1])
            d = _Dev(ctx)
            try:
                _, df = d.put(flow, 8)
                _, dt = d.put(tri, 4)
                bM, dM = d.blank(48 * nb, 8)
                bi, di = d.blank(nb * n, 1)
                br, dr = d.blank(32 * nb, 16)
                bw, dw = d.blank(need, 16)
                check(K.load().mav_flow_affine_dev(ctx.h, vp(df), _ptr(coords), n, nb, C.byref(p), vp(dt), vp(dM), vp(di), vp(dr), vp(dw), need))
                ctx.sync()
                d.get(bw, 16, np.uint8, (need,))
                got = d.get(bM, 8, np.float64, (nb, 2, 3)), d.get(bi, 1, np.uint8, (nb, n)), d.get(br, 16, R.RECORD_DTYPE, (nb,))
                _same(got, want, (frame, nb, "_dev", ctx_no))
                outside = coords.copy()
                outside[3] = (w, 0)
                rc = K.load().mav_flow_affine_dev(ctx.h, vp(df), _ptr(outside), n, nb, C.byref(p), vp(dt), vp(dM), vp(di), vp(dr), vp(dw), need)
                assert rc == _lib.MAV_ERR_ARG and b"mav_flow_affine_dev:" in K.load().mav_last_error()
            finally:
                d.close()


# ---- past the score kernel's grid cap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.CAP_CASES])
def test_device_equals_the_restatement_under_a_capped_score_grid(mav, name):
    """batch 16 on a context of max_batch 16: k_affine_score's grid is AFF_GRID_CAP / 16 workgroups per item, its counts written (and, at n = CHUNK + 1,
    added to) under the longer stride; the _late cases' winners are among the last hypotheses"""
    from mavflow import _lib, affine as K
    c, want = T.BY_NAME[name], T.reference(name)
    nb = c.src.shape[0]
    assert nb == T.CAP_BATCH and T.score_grid(c[3].shape[1], nb) == "capped"
    every = slice(0, nb)
    with _lib.Context(W, H, T.CAP_BATCH) as ctx:
        _same(_host(ctx, K, c, every), want, (name, "host"))
        _same(_dev(ctx, K, c, every, False), want, (name, "_dev"))
        _same(_dev(ctx, K, c, every, True), want, (name, "_dev, offset pointers"))

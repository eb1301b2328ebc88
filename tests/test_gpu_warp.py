"""The image warps on the GPU (csrc/kernels_warp.hip and the calls around it) against the numpy restatement tests/warp_ref.py at every case
of tests/warp_cases.py: every (coordinate policy x pixel format) instance at every frame, in the host and the _dev forms, at batch 1 and
3 with different operands per item, the _dev forms on pointers offset by one element into canary-filled blocks whose tails stay
untouched.  Equal bytes everywhere (a NaN is compared by position after canonicalisation, which both sides do): no tolerance appears in
this file.  The same bytes come out across two runs, every batch position and two contexts; every refusal of the header returns
MAV_ERR_ARG and leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import warp_cases as T
import warp_ref as R

pytestmark = pytest.mark.gpu
CANARY, TAIL = 0xA5, 64
_refs = {}


def _ref(policy, fmt, W, H):
    """[(names, src (B, ...), operands (B, ...), flags, want (B, ...))] per call of batch B, computed once and shared"""
    key = (policy, fmt, W, H)
    if key not in _refs:
        imgs = T.images(fmt, W, H)
        out = []
        by_flags = {}
        for name, op, fl in T.operands(policy, W, H):
            by_flags.setdefault(fl, []).append((name, op))
        for fl, items in by_flags.items():
            for g in T.groups(items):
                ops = np.stack([op for _, op in g])
                want = np.stack([T.reference(policy, imgs[b], g[b][1], fl) for b in range(T.B)])
                for a in (imgs, ops, want):
                    a.setflags(write=False)
                out.append((tuple(n for n, _ in g), imgs, ops, fl, want))
        _refs[key] = out
    return _refs[key]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        bad = np.argwhere(R.bits(got) != R.bits(want))
    else:
        bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _host_call(lib, ctx, policy, fmt, src, ops, fl, n, dst):
    from mavflow._lib import _ptr
    src, ops = np.ascontiguousarray(src[:n]), np.ascontiguousarray(ops[:n])
    if policy == "map":
        return lib.mav_remap(ctx.h, _ptr(src), fmt, _ptr(ops), n, _ptr(dst))
    if policy == "planes":
        mx, my = np.ascontiguousarray(ops[..., 0]), np.ascontiguousarray(ops[..., 1])
        return lib.mav_remap_planes(ctx.h, _ptr(src), fmt, _ptr(mx), _ptr(my), n, _ptr(dst))
    if policy == "flow":
        return lib.mav_warp_flow(ctx.h, _ptr(src), fmt, _ptr(ops), n, _ptr(dst))
    fn = lib.mav_warp_affine if policy == "affine" else lib.mav_warp_perspective
    return fn(ctx.h, _ptr(src), fmt, _ptr(ops), fl, n, _ptr(dst))


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


def _dev_call(lib, ctx, dev, policy, fmt, src, ops, fl, n, shifted):
    """the _dev form on device blocks; shifted: every pointer one element into its block.  -> (rc, dst block, its shift)"""
    vp = lambda p: C.c_void_p(int(p))
    src, ops = np.ascontiguousarray(src[:n]), np.ascontiguousarray(ops[:n])
    e = src.dtype.itemsize if shifted else 0
    _, ds = dev.put(src, e)
    db, dd = dev.blank(src.nbytes, e)
    if policy == "planes":
        _, dx = dev.put(ops[..., 0], 4 if shifted else 0)
        _, dy = dev.put(ops[..., 1], 4 if shifted else 0)
        rc = lib.mav_remap_planes_dev(ctx.h, vp(ds), fmt, vp(dx), vp(dy), n, vp(dd))
    elif policy in ("map", "flow"):
        _, do = dev.put(ops, 4 if shifted else 0)
        rc = (lib.mav_remap_dev if policy == "map" else lib.mav_warp_flow_dev)(ctx.h, vp(ds), fmt, vp(do), n, vp(dd))
    else:
        _, do = dev.put(ops, 8 if shifted else 0)
        rc = (lib.mav_warp_affine_dev if policy == "affine" else lib.mav_warp_perspective_dev)(ctx.h, vp(ds), fmt, vp(do), fl, n, vp(dd))
    return rc, db, e


@pytest.fixture(scope="module")
def contexts(mav):
    from mavflow import _lib
    made = {}

    def get(W, H, which=0):
        if (W, H, which) not in made:
            made[(W, H, which)] = _lib.Context(W, H, T.B)
        return made[(W, H, which)]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("frame", T.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("fmt", list(T.FORMATS), ids=str)
@pytest.mark.parametrize("policy", list(T.POLICIES), ids=str)
def test_device_bytes_equal_the_restatement(contexts, policy, fmt, frame):
    from mavflow import _lib, warp
    lib = warp.load()
    (W, H), f = frame, T.FORMATS[fmt]
    ctx = contexts(W, H)
    dev = _Dev(ctx)
    try:
        for names, src, ops, fl, want in _ref(policy, f, W, H):
            refused = policy in ("affine", "perspective") and [T.host_refuses(ops[b], fl) for b in range(T.B)]
            for n in (1, T.B):
                what = (policy, fmt, frame, names[:n], fl, n)
                # host form (matrices it refuses are refused, the output untouched)
                dst = np.full_like(want[:n], CANARY) if want.dtype == np.uint8 else np.full(want[:n].shape, np.float32(-777.25))
                keep = dst.copy()
                rc = _host_call(lib, ctx, policy, f, src, ops, fl, n, dst)
                if refused and any(refused[:n]):
                    assert rc == _lib.MAV_ERR_ARG and dst.tobytes() == keep.tobytes(), what
                else:
                    assert rc == 0, (what, lib.mav_last_error())
                    _same(dst, want[:n], ("host",) + what)
                # _dev form, plain and on pointers offset by one element
                for shifted in (False, True):
                    rc, db, e = _dev_call(lib, ctx, dev, policy, f, src, ops, fl, n, shifted)
                    assert rc == 0, (what, shifted, lib.mav_last_error())
                    ctx.sync()
                    _same(dev.get(db, e, want.dtype, want[:n].shape), want[:n], ("dev", shifted) + what)
                    dev.close()
    finally:
        dev.close()


@pytest.mark.parametrize("frame", T.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("kind", [R.AFFINE, R.PERSPECTIVE], ids=["affine", "perspective"])
def test_warp_method_equals_the_restatement(contexts, kind, frame):
    from mavflow import _lib, warp
    from mavflow._lib import _ptr
    lib = warp.load()
    W, H = frame
    ctx = contexts(W, H)
    flow = T.method_flow(W, H)
    ms = T.method_matrices(kind, W, H)
    vp = lambda p: C.c_void_p(int(p))
    dev = _Dev(ctx)
    try:
        for g in T.groups(ms):
            M = np.stack([np.array(m.M, np.float64) for m in g])
            ref = [R.warp_method(flow[b], M[b], kind) for b in range(T.B)]
            wd, wm, wr = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), np.stack([r[2] for r in ref])
            for n in (1, T.B):
                what = (kind, frame, [m.name for m in g][:n], n)
                diff, mag, rec = np.full((n, H, W, 2), np.float32(-7)), np.full((n, H, W), np.float32(-7)), np.full(n, -1, np.int32).repeat(4).view(R.RECORD_DTYPE)
                assert lib.mav_warp_method(ctx.h, _ptr(flow[:n]), _ptr(M[:n]), kind, n, _ptr(diff), _ptr(mag), _ptr(rec)) == 0, lib.mav_last_error()
                _same(diff, wd[:n], ("diff",) + what)
                _same(mag, wm[:n], ("mag",) + what)
                assert rec.tobytes() == wr[:n].tobytes(), (what, rec, wr[:n])
                # the record alone (diff and mag NULL)
                rec2 = np.full(n, -1, np.int32).repeat(4).view(R.RECORD_DTYPE)
                assert lib.mav_warp_method(ctx.h, _ptr(flow[:n]), _ptr(M[:n]), kind, n, None, None, _ptr(rec2)) == 0
                assert rec2.tobytes() == wr[:n].tobytes()
                for shifted in (False, True):
                    _, df = dev.put(flow[:n], 4 if shifted else 0)
                    _, dm = dev.put(M[:n], 8 if shifted else 0)
                    bd, dd = dev.blank(diff.nbytes, 4 if shifted else 0)
                    bg, dg = dev.blank(mag.nbytes, 4 if shifted else 0)
                    br, dr = dev.blank(16 * n, 16 if shifted else 0)
                    assert lib.mav_warp_method_dev(ctx.h, vp(df), vp(dm), kind, n, vp(dd), vp(dg), vp(dr)) == 0, lib.mav_last_error()
                    ctx.sync()
                    _same(dev.get(bd, 4 if shifted else 0, np.float32, diff.shape), wd[:n], ("dev diff", shifted) + what)
                    _same(dev.get(bg, 4 if shifted else 0, np.float32, mag.shape), wm[:n], ("dev mag", shifted) + what)
                    assert dev.get(br, 16 if shifted else 0, R.RECORD_DTYPE, (n,)).tobytes() == wr[:n].tobytes(), what
                    dev.close()
    finally:
        dev.close()


def test_same_bytes_across_runs_batch_positions_and_contexts(contexts):
    from mavflow import warp
    lib = warp.load()
    W, H = T.FRAMES[-1]
    a, b = contexts(W, H), contexts(W, H, 1)
    img = T.images(R.F32C2, W, H, nan=False)[1]
    u8 = T.images(R.U8C3, W, H)[1]
    M = np.array(T.perspective_matrices(W, H)[-2].M, np.float64)           # the mild tilt
    A = np.array(T.affine_matrices(W, H)[4].M, np.float64)
    flow = T.method_flow(W, H)[2]
    rep = lambda x: np.stack([x] * T.B)
    outs = []
    for ctx in (a, a, b):
        p = ctx.warp_perspective(rep(img), rep(M))
        q = ctx.warp_affine(rep(u8), rep(A), inverse_map=True)
        r = ctx.remap(rep(u8), rep(T.smooth_map(W, H)))
        m = ctx.warp_method(rep(flow), rep(M))
        for x in (p, q, r, m["diff"], m["mag"], m["records"]):
            for i in range(1, T.B):
                assert x[i].tobytes() == x[0].tobytes()                     # every batch position
        assert (m["records"]["row"][0], m["records"]["col"][0]) == tuple(np.argwhere(m["mag"][0] == m["mag"][0].max())[0])
        outs.append(b"".join(x.tobytes() for x in (p, q, r, m["diff"], m["mag"], m["records"])))
        one = ctx.warp_perspective(img, M)
        assert one.tobytes() == p[0].tobytes()                              # batch 1 and batch 3
    assert outs[0] == outs[1] == outs[2]


def test_refusals_that_need_the_context(contexts):
    """what the arguments alone decide is tests/test_abi_warp.py's; here: a batch above the context's, in every entry point, outputs untouched"""
    from mavflow import _lib, warp
    from mavflow._lib import _ptr
    lib = warp.load()
    W, H = T.FRAMES[2]
    ctx = contexts(W, H)
    n = T.B + 1
    src, m, M = np.zeros((n, H, W, 2), np.float32), np.zeros((n, H, W, 2), np.float32), np.stack([np.eye(3)] * n)
    dst = np.full((n, H, W, 2), np.float32(-3.5))
    rec = np.full(4 * n, -1, np.int32)
    A = np.ascontiguousarray(M[:, :2, :])
    s, mp, Mp, Ap, d = _ptr(src), _ptr(m), _ptr(M), _ptr(A), _ptr(dst)
    calls = {"mav_remap": (s, 3, mp, n, d), "mav_remap_planes": (s, 3, mp, mp, n, d), "mav_warp_flow": (s, 3, mp, n, d),
             "mav_warp_affine": (s, 3, Ap, 0, n, d), "mav_warp_perspective": (s, 3, Mp, 0, n, d),
             "mav_warp_method": (s, Mp, 1, n, d, d, _ptr(rec))}
    blk = ctx.alloc(dst.nbytes + 256).upload(np.full(dst.nbytes + 256, CANARY, np.uint8))
    try:
        for name, args in calls.items():
            assert getattr(lib, name)(ctx.h, *args) == _lib.MAV_ERR_ARG, name
            assert b"batch" in lib.mav_last_error() and name.encode() in lib.mav_last_error()
            dargs = tuple(C.c_void_p(blk.ptr) if isinstance(x, C.c_void_p) else x for x in args)
            assert getattr(lib, name + "_dev")(ctx.h, *dargs) == _lib.MAV_ERR_ARG, name
        # and on a live context what the arguments alone decide (tests/test_abi_warp.py has the full list on a handle never looked at)
        ok = T.B
        for name, args in {"mav_remap": (s, 4, mp, ok, d), "mav_warp_flow": (s, -1, mp, ok, d), "mav_remap_planes": (s, 3, mp, None, ok, d),
                           "mav_warp_affine": (s, 3, Ap, 1, ok, d), "mav_warp_perspective": (s, 3, Mp, 48, ok, d), "mav_warp_method": (s, Mp, 2, ok, d, d, _ptr(rec)),
                           "mav_warp_method_dev": (C.c_void_p(blk.ptr), C.c_void_p(blk.ptr + 256), 1, ok, C.c_void_p(blk.ptr), C.c_void_p(blk.ptr), C.c_void_p(blk.ptr + 8)),
                           "mav_remap_dev": (C.c_void_p(blk.ptr + 2), 3, C.c_void_p(blk.ptr), ok, C.c_void_p(blk.ptr)),
                           "mav_warp_affine_dev": (C.c_void_p(blk.ptr), 3, C.c_void_p(blk.ptr + 4), 0, ok, C.c_void_p(blk.ptr))}.items():
            assert getattr(lib, name)(ctx.h, *args) == _lib.MAV_ERR_ARG, name
            assert name.encode() + b":" in lib.mav_last_error()
        ctx.sync()
        assert (dst == np.float32(-3.5)).all() and (rec == -1).all()
        assert (blk.download(np.uint8, (blk.nbytes,)) == CANARY).all()
        # a singular matrix in the last item of a batch refuses the whole host call
        Ms = np.stack([np.eye(3)] * T.B)
        Ms[-1] = 0
        assert lib.mav_warp_perspective(ctx.h, s, 3, _ptr(Ms), 0, T.B, d) == _lib.MAV_ERR_ARG and (dst == np.float32(-3.5)).all()
        assert lib.mav_warp_perspective(ctx.h, s, 3, _ptr(Ms), warp.WARP_INVERSE_MAP_FLAG, T.B, d) == 0      # nothing to invert: taken
    finally:
        blk.free()


# ---- past the caps: the second trip of the grid-stride loops (tests/warp_cases.py CAP_FRAME, METHOD_CAP_FRAME) ---------------------------------
@pytest.mark.parametrize("fmt", list(T.FORMATS), ids=str)
@pytest.mark.parametrize("policy", list(T.POLICIES), ids=str)
def test_device_bytes_equal_the_restatement_past_the_cap(contexts, policy, fmt):
    """one _dev call at batch 2 per instance, plain and on pointers one element into their blocks (F32C2, CoordMap and CoordFlow on
    their scalar access), into canary-filled blocks; one host-form call per policy"""
    from mavflow import warp
    lib = warp.load()
    (W, H), f = T.CAP_FRAME, T.FORMATS[fmt]
    ctx = contexts(W, H)
    names, src, ops, fl, want, _ = T.cap_reference(policy, fmt)
    n = T.CAP_B
    what = (policy, fmt, T.CAP_FRAME, names, fl)
    dev = _Dev(ctx)
    try:
        if fmt == "F32C2":
            dst = np.full(want.shape, np.float32(-777.25))
            assert _host_call(lib, ctx, policy, f, src, ops, fl, n, dst) == 0, (what, lib.mav_last_error())
            _same(dst, want, ("host",) + what)
        for shifted in (False, True):
            rc, db, e = _dev_call(lib, ctx, dev, policy, f, src, ops, fl, n, shifted)
            assert rc == 0, (what, shifted, lib.mav_last_error())
            ctx.sync()
            _same(dev.get(db, e, want.dtype, want.shape), want, ("dev", shifted) + what)
            dev.close()
    finally:
        dev.close()


@pytest.mark.parametrize("kind", [R.AFFINE, R.PERSPECTIVE], ids=["affine", "perspective"])
def test_warp_method_equals_the_restatement_past_the_cap(contexts, kind):
    """batch 3, host and _dev forms, diff and mag present and both NULL: keys and the first pixel among equals carried across trips and
    workgroups into the one atomic per workgroup"""
    from mavflow import warp
    from mavflow._lib import _ptr
    lib = warp.load()
    W, H = T.METHOD_CAP_FRAME
    ctx = contexts(W, H)
    vp = lambda p: C.c_void_p(int(p))
    n = T.B
    dev = _Dev(ctx)
    try:
        for names, flow, M, wd, wm, wr in T.method_cap_reference(kind):
            what = (kind, T.METHOD_CAP_FRAME, names)
            diff, mag, rec = np.full((n, H, W, 2), np.float32(-7)), np.full((n, H, W), np.float32(-7)), np.full(n, -1, np.int32).repeat(4).view(R.RECORD_DTYPE)
            assert lib.mav_warp_method(ctx.h, _ptr(flow), _ptr(M), kind, n, _ptr(diff), _ptr(mag), _ptr(rec)) == 0, lib.mav_last_error()
            _same(diff, wd, ("diff",) + what)
            _same(mag, wm, ("mag",) + what)
            assert rec.tobytes() == wr.tobytes(), (what, rec, wr)
            rec2 = np.full(n, -1, np.int32).repeat(4).view(R.RECORD_DTYPE)
            assert lib.mav_warp_method(ctx.h, _ptr(flow), _ptr(M), kind, n, None, None, _ptr(rec2)) == 0
            assert rec2.tobytes() == wr.tobytes(), (what, rec2, wr)
            for shifted, outputs in ((False, True), (True, True), (False, False)):
                s4 = 4 if shifted else 0
                _, df = dev.put(flow, s4)
                _, dm = dev.put(M, 8 if shifted else 0)
                bd, dd = dev.blank(diff.nbytes, s4)
                bg, dg = dev.blank(mag.nbytes, s4)
                br, dr = dev.blank(16 * n, 16 if shifted else 0)
                assert lib.mav_warp_method_dev(ctx.h, vp(df), vp(dm), kind, n, vp(dd) if outputs else None, vp(dg) if outputs else None, vp(dr)) == 0, lib.mav_last_error()
                ctx.sync()
                if outputs:
                    _same(dev.get(bd, s4, np.float32, diff.shape), wd, ("dev diff", shifted) + what)
                    _same(dev.get(bg, s4, np.float32, mag.shape), wm, ("dev mag", shifted) + what)
                else:
                    assert (dev.get(bd, s4, np.uint8, (diff.nbytes,)) == CANARY).all() and (dev.get(bg, s4, np.uint8, (mag.nbytes,)) == CANARY).all()
                got = dev.get(br, 16 if shifted else 0, R.RECORD_DTYPE, (n,))
                assert got.tobytes() == wr.tobytes(), (what, shifted, outputs, got, wr)
                dev.close()
    finally:
        dev.close()

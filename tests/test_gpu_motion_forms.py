"""Every form of the global-motion branch (csrc/kernels_motion.hip and its launches) at the cases of tests/motion_cases.py, against the
numpy restatement tests/global_motion_ref.py and, for the windows, oracle/pyramid_oracle.py.  Equal bytes everywhere: no tolerance
appears in this file.  tests/test_motion_cases_cpu.py proves from the predicates that the cases reach every form; what is new here
over tests/test_gpu_global_motion.py: frames past the cap of the two grid-stride loops (ties across iterations and workgroups
included), frames of a few pixels, every output set on a batch item with an 8-byte base, a caller's own unaligned pointers, and the
fit at the ends of its range of n."""
import functools
import time

import numpy as np
import pytest

import global_motion_ref as R
import motion_cases as mc
from test_gpu_global_motion import check_record, expected_record

pytestmark = pytest.mark.gpu


def _ctx(W, H, B=1):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def _make_fields(W, H, B, kind):
    flows, Ms = mc.fields_of(mc.Case("fields", "host", W, H, B), kind)
    flows.setflags(write=False)
    return flows, Ms


def _make_restated(W, H, B, kind, b):
    flows, Ms = _fields(W, H, B, kind)
    sub = R.subtract(flows[b], Ms[b])
    for a in sub.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    sub["records"] = {}
    return sub


_shared_fields, _shared_restated = functools.lru_cache(maxsize=None)(_make_fields), functools.lru_cache(maxsize=None)(_make_restated)


def _fields(W, H, B, kind):
    """The random field of a size serves several tests: made once, shared, read-only.  The other kinds are used once each."""
    return (_shared_fields if kind == "random" else _make_fields)(W, H, B, kind)


def _restated(W, H, B, kind, b):
    """R.subtract of item b of a field kind, with room for its records (plain / optimised, filled by _check_item)."""
    return (_shared_restated if kind == "random" else _make_restated)(W, H, B, kind, b)


def _check_item(out, sub, b, optimize, what):
    for key in ("warped", "mag"):
        if key in out:
            assert out[key][b].tobytes() == sub[key].tobytes(), (what, key, b)
    if "gray" in out:
        assert np.array_equal(out["gray"][b], sub["gray"]), (what, b, np.flatnonzero(out["gray"][b].ravel() != sub["gray"].ravel())[:4])
    if optimize not in sub["records"]:
        sub["records"][optimize] = expected_record(sub["gray"], sub, optimize)
    check_record(out["results"][b], sub["records"][optimize], (what, b, optimize))


@pytest.mark.parametrize("case", mc.frame_cases("host"), ids=lambda c: c.name)
def test_fields_image_and_records_equal_the_restatement(case):
    """Every field kind of the case through mav_global_motion with every output: warped, mag, gray and the record of every item.  Small
    frames take `optimize` both ways on every field, frames past the cap once (on the random field)."""
    c = case
    large = c.n0 > mc.second_iteration_pixel(mc.PX_A)
    with _ctx(c.W, c.H, c.B) as ctx:
        for kind in c.fields:
            flows, Ms = _fields(c.W, c.H, c.B, kind)
            subs = [_restated(c.W, c.H, c.B, kind, b) for b in range(c.B)]
            for optimize in ((False, True) if (not large or kind == "random") else (False,)):
                out = ctx.global_motion(flows, Ms, optimize=optimize, outputs=("warped", "mag", "gray"))
                for b in range(c.B):
                    _check_item(out, subs[b], b, optimize, (c.name, kind))
                first = [(int(r["max_row"]), int(r["max_col"])) for r in out["results"]]
                if kind == "constant":                    # every pixel ties, in every workgroup and iteration: pixel (0, 0) wins
                    assert first == [(0, 0)] * c.B and (out["gray"] == 255).all()
                if kind == "zero":
                    assert first == [(0, 0)] * c.B and not out["gray"].any() and all(float(r["max_mag"]) == 0.0 for r in out["results"])
                if kind.startswith("ties"):
                    assert first == [divmod(mc.tie_pixels(c)[kind][0], c.W)] * c.B, (kind, first)
                    assert all(float(r["max_mag"]) == mc.TIE_MAG for r in out["results"])


@pytest.mark.parametrize("case", [c for c in mc.CASES if c.name.startswith("outputs")], ids=lambda c: c.name)
def test_every_output_set_gives_the_same_record_and_fields(case):
    """The sets of optional outputs the entry points can request of pass A -- none, warped, mag, both through mav_global_motion; gm alone
    and warped alone, without the key, through mav_last_global_motion_render -- on a batch with an item whose base is 8 bytes past a
    16-byte boundary (the two-float store path)."""
    c = case
    flows, Ms = _fields(c.W, c.H, c.B, "random")
    subs = [_restated(c.W, c.H, c.B, "random", b) for b in range(c.B)]
    with _ctx(c.W, c.H, c.B) as ctx:
        # flow_to_color is a host call of its own, after which nothing of a global-motion call is resident: the references first
        ref_w = ctx.flow_to_color(np.stack([s["warped"] for s in subs]))
        ref_g = ctx.flow_to_color(np.stack([s["global_motion"] for s in subs]))
        full = ctx.global_motion(flows, Ms, optimize=True, outputs=("warped", "mag", "gray"))
        for b in range(c.B):
            _check_item(full, subs[b], b, True, c.name)
        for name, outs in mc.OUTPUT_SETS.items():
            got = ctx.global_motion(flows, Ms, optimize=True, outputs=outs)
            assert set(got) == set(outs) | {"results"}, name
            assert got["results"].tobytes() == full["results"].tobytes(), name
            for b in range(c.B):
                _check_item(got, subs[b], b, True, (c.name, name))
        for name, images in mc.RENDER_SETS.items():
            imgs = ctx.render_last_global_motion(c.B, images=images)
            assert set(imgs) == set(images), name
            ref = ref_g if images == ("global",) else ref_w
            assert np.array_equal(imgs[images[0]], ref), (name, int((imgs[images[0]] != ref).sum()))


# ---- a caller's own device pointers --------------------------------------------------------------------------------------------------
GUARD = 16


class _Dev:
    """Device buffers of one test.  Each has GUARD spare bytes and starts out filled with 0xA5, so that a pointer moved by a few bytes
    still has its whole extent inside the allocation, and guards_intact() can tell whether anything was written before or behind it."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def alloc(self, nbytes, off=0):
        assert 0 <= off <= GUARD
        buf = self.ctx.alloc(nbytes + GUARD)
        buf.upload(np.full(nbytes + GUARD, 0xA5, np.uint8))
        self.bufs.append((buf, off, nbytes))
        return buf.ptr + off

    def put(self, a, off=0):
        from mavflow import _lib
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes, off)
        _lib.check(self.ctx.lib.mav_memcpy_h2d(self.ctx.h, p, a.ctypes.data, a.nbytes))
        return p

    def get(self, p, dtype, shape):
        from mavflow import _lib
        out = np.empty(shape, dtype)
        _lib.check(self.ctx.lib.mav_memcpy_d2h(self.ctx.h, out.ctypes.data, p, out.nbytes))
        return out

    def guards_intact(self):
        for buf, off, nbytes in self.bufs:
            whole = buf.download(np.uint8, (nbytes + GUARD,))
            if not ((whole[:off] == 0xA5).all() and (whole[off + nbytes:] == 0xA5).all()):
                return False
        return True

    def free(self):
        for buf, _, _ in self.bufs:
            buf.free()
        self.bufs = []


def _dev_call(ctx, c, flows, Ms, optimize):
    """mav_global_motion_dev with the case's offsets on the caller's buffers -> dict of what it wrote; nothing outside them is touched."""
    from mavflow import _lib
    B, n0 = c.B, c.n0
    d = _Dev(ctx)
    try:
        pf = d.put(flows, c.flow_off)
        pM = d.put(np.ascontiguousarray(Ms[:, :2, :]))
        pw, pm = d.alloc(n0 * B * 8, c.warped_off), d.alloc(n0 * B * 4, c.mag_off)
        pg, pr = d.alloc(n0 * B, c.gray_off), d.alloc(B * _lib.MOTION_DTYPE.itemsize)
        _lib.check(ctx.lib.mav_global_motion_dev(ctx.h, pf, pM, B, 1.5, int(optimize), pw, pm, pg, pr))
        got = dict(warped=d.get(pw, np.float32, (B, c.H, c.W, 2)), mag=d.get(pm, np.float32, (B, c.H, c.W)),
                   gray=d.get(pg, np.uint8, (B, c.H, c.W)), results=d.get(pr, _lib.MOTION_DTYPE, (B,)))
        assert d.guards_intact(), (c.name, "bytes outside a caller's buffer were written")
        return got
    finally:
        d.free()


DEV_GROUPS = sorted({(c.W, c.H, c.B) for c in mc.frame_cases("dev")})


@pytest.mark.parametrize("size", DEV_GROUPS, ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_callers_pointers_give_the_aligned_calls_bytes_and_stay_inside(size):
    """mav_global_motion_dev on the caller's own buffers.  64 x 64: every item base is 16-byte aligned, and the flow 8 bytes, warped 8
    bytes, mag 4 bytes or gray 1 byte past such a boundary (ordinary pointers for their types; include/mavflow.h asks for no more)
    selects the two-float / byte forms -- every output keeps the bytes of the aligned call and of the restatement.  97 x 71: an odd pixel
    count, whose last pair has one pixel.  Every buffer is followed by guard bytes, which must survive."""
    cases = [c for c in mc.frame_cases("dev") if (c.W, c.H, c.B) == size]
    aligned = cases[0]
    assert aligned.name.endswith("aligned") and not (aligned.flow_off or aligned.gray_off or aligned.warped_off or aligned.mag_off)
    flows, Ms = _fields(aligned.W, aligned.H, aligned.B, "random")
    with _ctx(aligned.W, aligned.H, aligned.B) as ctx:
        for optimize in (False, True):
            base = _dev_call(ctx, aligned, flows, Ms, optimize)
            for b in range(aligned.B):
                _check_item(base, _restated(aligned.W, aligned.H, aligned.B, "random", b), b, optimize, aligned.name)
            for c in cases[1:]:
                got = _dev_call(ctx, c, flows, Ms, optimize)
                for key in ("warped", "mag", "gray", "results"):
                    assert got[key].tobytes() == base[key].tobytes(), (c.name, key, optimize)


def test_step_on_callers_pointers_and_with_a_failed_item():
    """mav_global_motion_step_dev (gather, fit, both passes with the matrix behind the fit at stride 9 and the fit's flags): H, ok, gray and
    the records against the restated chain; with the flow 8 bytes or gray 1 byte off, the bytes of the same call on aligned buffers."""
    from mavflow import _lib
    for c in mc.frame_cases("step"):
        flows, coords = mc.step_inputs(c)
        exp = []
        for b in range(c.B):
            He, oke = R.find_homography(coords.astype(np.float64), R.coords_new(coords, flows[b]))
            assert oke == (0 if b == c.failed else 1)
            exp.append((He, oke, R.subtract(flows[b], He) if oke else None))
        with _ctx(c.W, c.H, c.B) as ctx:
            d = _Dev(ctx)
            try:
                runs = {}
                for tag, fo, go in (("aligned", 0, 0), ("offset", c.flow_off, c.gray_off)):
                    pf, pg = d.put(flows, fo), d.alloc(c.n0 * c.B, go)
                    pH, pok, pr = d.alloc(72 * c.B), d.alloc(4 * c.B), d.alloc(c.B * _lib.MOTION_DTYPE.itemsize)
                    for optimize in (False, True):
                        ctx.global_motion_step(pf, coords, c.B, pr, optimize=optimize, H_ptr=pH, ok_ptr=pok, gray_ptr=pg)
                        runs[tag, optimize] = dict(H=d.get(pH, np.float64, (c.B, 3, 3)), ok=d.get(pok, np.int32, (c.B,)),
                                                   gray=d.get(pg, np.uint8, (c.B, c.H, c.W)), results=d.get(pr, _lib.MOTION_DTYPE, (c.B,)))
                for optimize in (False, True):
                    got = runs["aligned", optimize]
                    for b, (He, oke, sub) in enumerate(exp):
                        assert int(got["ok"][b]) == oke and got["H"][b].tobytes() == He.tobytes(), (c.name, b)
                        if oke:
                            assert np.array_equal(got["gray"][b], sub["gray"]), (c.name, b)
                            check_record(got["results"][b], expected_record(sub["gray"], sub, optimize), (c.name, b, optimize))
                        else:
                            assert got["results"][b].tobytes() == bytes(_lib.MOTION_DTYPE.itemsize) and not got["H"][b].any()
                    for key, a in runs["offset", optimize].items():
                        assert a.tobytes() == got[key].tobytes(), (c.name, key, optimize)
                assert d.guards_intact(), c.name
            finally:
                d.free()


# ---- the fit at the ends of its range ------------------------------------------------------------------------------------------------
def test_fit_at_the_sums_chunk_and_at_the_bound():
    """n = 4, 15, 16, 256, 1000 and MAV_HOMOGRAPHY_MAX_PAIRS against R.find_homography, byte for byte; one pair more is refused, and the
    context works afterwards.  Prints the call's time at the bound (upload and synchronisation included)."""
    cases = [c for c in mc.CASES if c.entry == "fit"]
    with _ctx(64, 64, 1) as ctx:
        for c in cases:
            src, dst = mc.fit_pairs(c)
            He, oke = R.find_homography(src, dst)
            t0 = time.perf_counter()
            H, ok = ctx.find_homography(src, dst)
            t1 = time.perf_counter()
            assert int(ok[0]) == oke == 1 and H[0].tobytes() == He.tobytes(), (c.name, np.abs(H[0] - He).max())
            if c.n == mc.MAX_PAIRS:
                t2 = time.perf_counter()
                H2, _ = ctx.find_homography(src, dst)
                t3 = time.perf_counter()
                assert H2.tobytes() == H.tobytes()
                print(f"mav_find_homography at n = {c.n}: {1e3 * (t1 - t0):.1f} ms first call (buffers grow), {1e3 * (t3 - t2):.1f} ms second")
        src, dst = mc.fit_pairs(mc.Case("over", "fit", n=mc.MAX_PAIRS + 1))
        with pytest.raises(ValueError, match="pairs outside"):
            ctx.find_homography(src, dst)
        small = mc.BY_NAME["fit16"]
        H, ok = ctx.find_homography(*mc.fit_pairs(small))
        assert int(ok[0]) == 1 and H[0].tobytes() == R.find_homography(*mc.fit_pairs(small))[0].tobytes()


def test_frame_like_fit_then_its_fields_and_gray_conversion_past_the_cap():
    """The frame-like pairs (1000 samples of a 1920 x 1024 field, perspective motion, noise, a moving patch): H byte for byte, then the
    fields of a 1025 x 1025 frame under that H.  On the same context, k_bgr2gray past its cap of 4096 workgroups (1 048 576 px)."""
    from oracle import gray_oracle
    c = mc.BY_NAME["1025x1025b1"]
    src, dst = mc.frame_like_pairs()
    He, oke = R.find_homography(src, dst)
    flows, _ = _fields(c.W, c.H, c.B, "random")
    sub = R.subtract(flows[0], He)
    with _ctx(c.W, c.H, 1) as ctx:
        H, ok = ctx.find_homography(src, dst)
        assert int(ok[0]) == oke == 1 and H[0].tobytes() == He.tobytes()
        out = ctx.global_motion(flows, H, optimize=True, outputs=("warped", "mag", "gray"))
        assert out["warped"][0].tobytes() == sub["warped"].tobytes() and out["mag"][0].tobytes() == sub["mag"].tobytes()
        assert np.array_equal(out["gray"][0], sub["gray"])
        check_record(out["results"][0], expected_record(sub["gray"], sub, True), "frame-like")
        assert c.n0 > 4096 * 256
        bgr = np.random.default_rng(9).integers(0, 256, (1, c.H, c.W, 3), dtype=np.uint8)
        assert np.array_equal(ctx.bgr2gray(bgr)[0], gray_oracle.bgr_to_gray(bgr[0]))

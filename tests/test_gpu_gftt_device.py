"""The corner sort and pick on the device, the enqueue-only corner call, cv2's mask and the tracker that reads its point count from the
device, against the CPU restatements (tests/lk_ref.py, tests/gftt_pick_model.py): EQUAL BYTES throughout."""
import numpy as np
import pytest

import gftt_pick_model as gm
import lk_ref
from test_gpu_lk import border_maximum_image, same
from test_lk_ref_cpu import blurred_noise

pytestmark = pytest.mark.gpu
F = np.float32
PATTERN = 0xA5                                                   # pre-fill of every output buffer: what must stay untouched
SPARSE_WORKSPACE_640x480 = 6_898_868                            # the figure of include/mavflow.h


class Outputs:
    """Device buffers of the enqueue-only calls: corners (max_corners, 2) f32, count i32, tracked points, status."""

    def __init__(self, ctx, mc):
        self.ctx, self.mc = ctx, mc
        self.corners, self.count = ctx.alloc(mc * 8), ctx.alloc(4)
        self.out, self.status = ctx.alloc(mc * 8), ctx.alloc(mc)
        self.fill()

    def fill(self):
        for b in (self.corners, self.count, self.out, self.status):
            b.upload(np.full(b.nbytes, PATTERN, np.uint8))

    def read(self):
        self.ctx.sync()
        return (self.corners.download(F, (self.mc, 2)), int(self.count.download(np.int32, (1,))[0]), self.out.download(F, (self.mc, 2)),
                self.status.download(np.uint8, (self.mc,)))


def untouched(a, start):
    return bool(np.all(np.ascontiguousarray(a[start:]).view(np.uint8) == PATTERN))


def corners_enqueue(ctx, o, gray_ptr, mask_ptr=None, **kw):
    o.fill()
    ctx.good_features_enqueue(gray_ptr, o.corners.ptr, o.count.ptr, mask_ptr, max_corners=o.mc, **kw)
    corners, n, _, _ = o.read()
    assert n < 0 or untouched(corners, n), "entries beyond the count were written"
    return corners[:max(n, 0)].copy(), n


def images_of(W, H):
    from mavflow import synth
    return {"synth0": synth.make_pair(W, H, 0)[0], "synth1": synth.make_pair(W, H, 1)[1], "blurred": blurred_noise(W, H, 3),
            "border": border_maximum_image(W, H)}


# ---- 1. the enqueue-only corner call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(320, 240), (1920, 1080)])
def test_good_features_enqueue_is_exact(mav, W, H):
    from mavflow import _lib
    with _lib.Context(W, H, 1) as ctx:
        outs = {mc: Outputs(ctx, mc) for mc in (1, 50, 2000)}
        for name, img in images_of(W, H).items():
            dev = ctx.alloc(W * H).upload(img)
            # lk_ref's candidates once per image; good_features's loop (gm.sequential IS that loop) per parameter pair
            v, idx = lk_ref.corner_candidates(lk_ref.min_eigen(img), 0.2)
            keys = gm.keys_of(v, idx)
            if name in ("synth0", "border"):
                assert same(gm.sequential(keys, W, 2000, 7), lk_ref.good_features(img)), name
                assert same(gm.sequential(keys, W, 50, 7.5), lk_ref.good_features(img, max_corners=50, min_distance=7.5)), name
                assert same(gm.sequential(keys, W, 2000, 40), lk_ref.good_features(img, min_distance=40)), name
            for mc in (1, 50, 2000):
                for md in (1, 7, 7.5, 40):
                    ref = gm.sequential(keys, W, mc, md)
                    got = [corners_enqueue(ctx, outs[mc], dev.ptr if r == 0 else None, min_distance=md) for r in range(3)]
                    for r, (c, n) in enumerate(got):                # three times: the append order of the candidates is arbitrary
                        assert n == len(ref) and same(c, ref), (name, mc, md, r, n, len(ref))
            assert same(ctx.good_features(None), gm.sequential(keys, W, 2000, 7)), name       # the host form, the resident frame
            dev.free()


# ---- 2. hostile candidate sets through the stage hook ---------------------------------------------------------------------------------
def check_pick(ctx, W, keys, mc, md, label):
    keys = np.random.default_rng(9).permutation(keys)
    got = ctx.stage_corner_pick(keys, max_corners=mc, min_distance=md)
    ref = gm.sequential(keys, W, mc, md)
    chunks, rounds = ctx.gftt_last_pick()
    print(f"pick {label}: n={len(keys)} mc={mc} md={md:g} -> {len(got)} corners, {chunks} chunks, {rounds} rounds")
    assert same(got, ref), (label, mc, md, len(got), len(ref))
    return chunks, rounds


def test_stage_corner_pick_on_hostile_families(mav):
    from mavflow import _lib
    from test_gftt_pick_model_cpu import MIN_DISTANCES, families
    W, H = 96, 64
    with _lib.Context(W, H, 1) as ctx:
        for name, keys in families():
            full = len(gm.sequential(keys, W, 65536, 7))
            for md in MIN_DISTANCES:
                for mc in (1, max(full // 2, 1), 65536):
                    check_pick(ctx, W, keys, mc, md, name)
        assert ctx.stage_corner_pick(np.zeros(0, np.uint64)).shape == (0, 2)
        with pytest.raises(ValueError, match="outside the frame"):
            ctx.stage_corner_pick(np.array([W * H], np.uint64))
        for w, h in ((3, 3), (5, 3)):
            with _lib.Context(w, h, 1) as tiny:
                for md in (1, 2, 3):
                    check_pick(tiny, w, gm.all_equal(w, h), 65536, md, "tiny")


def test_stage_corner_pick_on_a_long_ramp(mav):
    """6000 candidates decided strictly one after the other: a legitimate input that must simply finish, and be right."""
    from mavflow import _lib
    W, H = 400, 300
    with _lib.Context(W, H, 1) as ctx:
        model_rounds = gm.good_features_from_keys(gm.ramp(6000, W, H), W, H, 65536, 2.5, want_stats=True)[1]["rounds"]
        chunks, rounds = check_pick(ctx, W, gm.ramp(6000, W, H), 65536, 2.5, "ramp6000")
        assert chunks == 6 and 3000 <= rounds <= model_rounds          # the model's schedule is the slowest one
        check_pick(ctx, W, gm.ramp(6000, W, H), 2000, 7, "ramp6000")
        check_pick(ctx, W, gm.ramp(300, W, H), 65536, 2.5, "ramp300")


def test_stage_corner_pick_on_a_full_buffer(mav):
    from mavflow import _lib
    W, H = 1026, 514
    keys = gm.all_equal(W, H, every=2)
    assert len(keys) == _lib.GFTT_MAX_CANDIDATES
    with _lib.Context(W, H, 1) as ctx:
        for mc, md in ((65536, 7), (1, float(np.hypot(W, H)) + 1), (65536, 0), (3000, 40), (65536, 1)):
            check_pick(ctx, W, keys, mc, md, "capacity")
        check_pick(ctx, W, gm.random_set(W, H, _lib.GFTT_MAX_CANDIDATES, 3, levels=4), 65536, 7.5, "capacity, ties")
        with pytest.raises(ValueError):
            ctx.stage_corner_pick(np.arange(_lib.GFTT_MAX_CANDIDATES + 1, dtype=np.uint64))


# ---- 3. masks --------------------------------------------------------------------------------------------------------------------------
def test_masks_host_and_device_forms(mav):
    from mavflow import _lib
    W, H = 320, 240
    img = blurred_noise(W, H, 3)
    eig = lk_ref.min_eigen(img)
    ym, xm = np.unravel_index(np.argmax(eig), eig.shape)
    ones = np.ones((H, W), np.uint8)
    left, top = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    left[:, :W // 2] = 255
    top[:H // 2] = 1
    hidden = ones.copy()
    hidden[max(ym - 12, 0):ym + 13, max(xm - 12, 0):xm + 13] = 0
    pixel = ones.copy()
    pixel[ym, xm] = 0
    with _lib.Context(W, H, 1) as ctx:
        o = Outputs(ctx, 2000)
        dev = ctx.alloc(W * H).upload(img)
        dmask = ctx.alloc(W * H)
        plain = ctx.good_features(img)
        assert same(plain, lk_ref.good_features(img))
        for name, mask in (("ones", ones), ("left", left), ("top", top), ("hidden", hidden), ("pixel", pixel), ("zero", np.zeros((H, W), np.uint8))):
            for kw in ({}, {"min_distance": 1, "quality_level": 0.05}):
                ref = gm.good_features_masked(img, mask, **kw)
                assert same(ctx.good_features(img, mask=mask, **kw), ref), (name, kw)
                assert same(ctx.good_features(None, mask=mask, **kw), ref), (name, kw)
                dmask.upload(mask)
                got, n = corners_enqueue(ctx, o, dev.ptr, dmask.ptr, **kw)
                assert n == len(ref) and same(got, ref), (name, kw)
            if name == "ones":
                assert same(ctx.good_features(img, mask=mask), plain) and same(ctx.good_features(img, mask=None), plain)
            if name == "zero":
                assert ctx.good_features(img, mask=mask).shape == (0, 2)
        # the threshold moves with the masked maximum: corners below the old threshold come in
        got = ctx.good_features(img, mask=hidden, max_corners=65536, min_distance=0)
        old_thr = F(np.float64(eig.max()) * 0.2)
        assert (eig[got[:, 1].astype(int), got[:, 0].astype(int)] <= old_thr).any()
        # a mask after a track call (the mask is staged in the frame slot that no call reads again)
        nxt = np.roll(img, (1, 2), axis=(0, 1))
        pts, st = ctx.lk_track(img, nxt, plain)
        assert same(ctx.good_features(None, mask=left), gm.good_features_masked(nxt, left))
        p2, s2 = ctx.lk_track(None, img, pts)
        r2, rs2 = lk_ref.lk_track(nxt, img, pts)
        assert same(p2, r2) and same(s2, rs2)
        for bad in (np.ones((H, W + 1), np.uint8), np.ones((H, W), np.float32), np.ones((H, W), bool), np.ones(W * H, np.uint8)):
            with pytest.raises(ValueError, match="mask"):
                ctx.good_features(img, mask=bad)


# ---- 4. overflow -----------------------------------------------------------------------------------------------------------------------
def test_overflow_is_a_negative_count_on_the_device(mav):
    from mavflow import _lib
    W, H = 1600, 1400
    yy, xx = np.mgrid[0:H, 0:W]
    img = ((((yy // 2) + (xx // 2)) & 1) * 255).astype(np.uint8)
    _, idx = lk_ref.corner_candidates(lk_ref.min_eigen(img), 0.2)
    assert len(idx) > _lib.GFTT_MAX_CANDIDATES
    with _lib.Context(W, H, 1) as ctx:
        o = Outputs(ctx, 2000)
        dev = ctx.alloc(W * H).upload(img)
        o.fill()
        ctx.good_features_enqueue(dev.ptr, o.corners.ptr, o.count.ptr)
        corners, n, _, _ = o.read()
        assert n == -len(idx) and untouched(corners, 0)
        # a tracker behind it tracks nothing
        ctx.lk_track_enqueue(None, dev.ptr, o.corners.ptr, o.mc, o.count.ptr, o.out.ptr, o.status.ptr)
        _, _, out, status = o.read()
        assert untouched(out, 0) and untouched(status, 0) and ctx.lk_last_iterations().sum() == 0
        with pytest.raises(ValueError, match=str(len(idx))):
            ctx.good_features(img)
        with pytest.raises(ValueError, match=str(len(idx))):
            ctx.good_features(img, mask=np.ones((H, W), np.uint8))


# ---- 5. corners -> track as one chain --------------------------------------------------------------------------------------------------
def test_corners_to_track_chain(mav):
    from mavflow import _lib, synth
    W, H, MC = 320, 240, 2000
    seq = synth.make_sequence(W, H, 4, seed=3)
    with _lib.Context(W, H, 1) as a, _lib.Context(W, H, 1) as b:
        dev = [a.alloc(W * H).upload(f) for f in seq]
        o = Outputs(a, MC)
        for i in range(3):
            o.fill()
            a.good_features_enqueue(dev[0].ptr if i == 0 else None, o.corners.ptr, o.count.ptr)      # the resident frame is carried
            a.lk_track_enqueue(None, dev[i + 1].ptr, o.corners.ptr, MC, o.count.ptr, o.out.ptr, o.status.ptr)
            corners, n, out, status = o.read()                                                      # the one sync() of the frame
            pts = b.good_features(seq[i])
            r_out, r_status = b.lk_track(None, seq[i + 1], pts)
            assert n == len(pts) and 0 < n < MC and same(corners[:n], pts), i
            assert same(out[:n], r_out) and same(status[:n], r_status), i
            assert untouched(corners, n) and untouched(out, n) and untouched(status, n), i
            assert same(a.lk_last_iterations(), b.lk_last_iterations()), i
        # the count equal to n_max: the bytes of mav_lk_track_dev(n_max)
        o.count.upload(np.array([n], np.int32))
        a.lk_track_enqueue(dev[2].ptr, dev[3].ptr, o.corners.ptr, n, o.count.ptr, o.out.ptr, o.status.ptr)
        _, _, out1, status1 = o.read()
        hist1 = a.lk_last_iterations()
        o.out.upload(np.full(MC * 8, PATTERN, np.uint8)); o.status.upload(np.full(MC, PATTERN, np.uint8))
        a.lk_track_dev(dev[2].ptr, dev[3].ptr, o.corners.ptr, n, o.out.ptr, o.status.ptr)
        _, _, out2, status2 = o.read()
        assert same(out1, out2) and same(status1, status2) and same(hist1, a.lk_last_iterations())
        # a count above n_max runs n_max points; a negative count tracks nothing
        o.count.upload(np.array([n + 1000], np.int32))
        a.lk_track_enqueue(dev[2].ptr, dev[3].ptr, o.corners.ptr, 100, o.count.ptr, o.out.ptr, o.status.ptr)
        _, _, out3, status3 = o.read()
        assert same(out3[:100], out2[:100]) and same(status3[:100], status2[:100])
        o.fill()
        o.count.upload(np.array([-7], np.int32))
        a.lk_track_enqueue(dev[2].ptr, dev[3].ptr, o.corners.ptr, MC, o.count.ptr, o.out.ptr, o.status.ptr)
        _, _, out4, status4 = o.read()
        assert untouched(out4, 0) and untouched(status4, 0) and a.lk_last_iterations().sum() == 0
        with pytest.raises(ValueError):
            a.lk_track_enqueue(None, dev[0].ptr, o.corners.ptr, MC, None, o.out.ptr, o.status.ptr)


# ---- 6. memory -------------------------------------------------------------------------------------------------------------------------
def test_the_device_pick_brings_no_memory_of_its_own(mav):
    from mavflow import _lib, synth
    W, H = 640, 480
    f0, f1, _ = synth.make_pair(W, H, 0)
    with _lib.Context(W, H, 1) as ctx:
        dev = ctx.alloc(W * H).upload(f0)
        o = Outputs(ctx, 2000)
        before = ctx.mem_info()["ctx_bytes"]
        ctx.good_features(f0)
        grown = ctx.mem_info()["ctx_bytes"] - before
        print(f"sparse workspace at {W}x{H}: {grown} bytes")
        assert abs(grown - SPARSE_WORKSPACE_640x480) <= 9 * 4096, grown                 # nine allocations, each rounded at most a page
        held = ctx.mem_info()["ctx_bytes"]
        ctx.good_features_enqueue(dev.ptr, o.corners.ptr, o.count.ptr, min_distance=1)
        ctx.good_features_enqueue(None, o.corners.ptr, o.count.ptr, dev.ptr, min_distance=40)
        ctx.lk_track_enqueue(None, dev.ptr, o.corners.ptr, o.mc, o.count.ptr, o.out.ptr, o.status.ptr)
        ctx.good_features(f1, mask=np.ones((H, W), np.uint8), min_distance=2)
        ctx.stage_corner_pick(gm.random_set(W, H, 5000, 1), min_distance=3)
        ctx.sync()
        assert ctx.mem_info()["ctx_bytes"] == held

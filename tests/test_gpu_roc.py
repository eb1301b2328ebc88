"""The threshold sweep on the device (mav_roc_sweep: k_roc_sweep / k_roc_suffix of csrc/kernels_detect.hip), held by equality to the
existing device path -- Ka x Km runs of the phi / mask stage plus tpr_fpr_counts -- and to the numpy reference (tests/roc_ref.py) at
the ragged shapes of tests/detect_cases.py, on the planted fields and on a batch of more than 64 pairs.  Nothing is excused: the band
condition that makes equality with the oracle fair is kept by tests/test_roc_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
import roc_cases as rc
import roc_ref as R

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A5A5A5A5A


def _ctx(W, H, B):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def _thr(a, m):
    from mavflow import _lib
    p = _lib.thr_defaults()
    p.fixed_deg, p.fixed_min_mag = float(a), float(m)
    return p


def _route(c, call, fl, fe, sky, gt, angles, mags, want_phi):
    """The parent's only route to the same answer: one phi / mask stage and one counts pass per threshold pair."""
    B = fl.shape[0]
    kw = rc.sweep_kwargs(call, B)
    src = fl.astype(np.float64) if call.flow == "f64" else fl
    out = np.empty((B, len(angles), len(mags), 4), np.int64)
    for i, a in enumerate(angles):
        for j, m in enumerate(mags):
            if call.entry == "stage":
                _, mf, _, _ = c.stage_phi_mask(fl, fe, omega=kw.get("omega"), dt=kw.get("dt"), sky=sky, params=_thr(a, m), want_phi=want_phi)
            else:                                             # mav_phi_mask on the promoted field | mav_phi_mask_f32: the frame-0 route
                _, mf, _, _ = c.phi_mask(src, fe, sky=sky, params=_thr(a, m), want_phi=want_phi)
            out[:, i, j] = c.tpr_fpr_counts(gt, mf, 255)
    return out


def _noise(case):
    return dc.noise_fields(case.W, case.H), dc.foes(case.W, case.H), dc.sky_masks(case.W, case.H), rc.gt_images(case.W, case.H)


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_equals_the_existing_device_path(mav, case):
    fl, fe, sky, gt = _noise(case)
    with _ctx(case.W, case.H, dc.PHI_B) as c:
        for call in rc.CALLS:
            kw = rc.sweep_kwargs(call, dc.PHI_B)
            for g in ("full", "one") + rc.DEVICE_ONLY_GRIDS:
                a, m = rc.GRIDS[g]
                got = c.roc_sweep(fl, fe, gt, a, m, sky=sky, **kw)
                assert got["counts"].shape == (dc.PHI_B, len(a), len(m), 4) and got["counts"].dtype == np.int64
                assert np.array_equal(got["counts"], _route(c, call, fl, fe, sky, gt, a, m, True)), (case.name, call.name, g, "exact")
                if g == "full":                               # ... and once with the single-precision screen in front of the stage
                    assert np.array_equal(got["counts"], _route(c, call, fl, fe, sky, gt, a, m, False)), (case.name, call.name, g, "screen")
            a, m = rc.GRIDS["one"]                            # no sky mask
            assert np.array_equal(c.roc_sweep(fl, fe, gt, a, m, **kw)["counts"], _route(c, call, fl, fe, None, gt, a, m, True)), (case.name, call.name)


@pytest.mark.parametrize("call", rc.CALLS, ids=[c.name for c in rc.CALLS])
def test_the_maximum_grid_equals_the_existing_device_path(mav, call):
    case = dc.PHI_CASES[dc.PHI_IDS.index(rc.MAX_GRID_CASE)]
    fl, fe, sky, gt = _noise(case)
    a, m = rc.GRIDS["max"]
    with _ctx(case.W, case.H, dc.PHI_B) as c:
        got = c.roc_sweep(fl, fe, gt, a, m, sky=sky, **rc.sweep_kwargs(call, dc.PHI_B))["counts"]
        assert got.shape == (dc.PHI_B, rc.MAX_ANGLES, rc.MAX_MAGS, 4)
        assert np.array_equal(got, _route(c, call, fl, fe, sky, gt, a, m, True))
        assert got[..., 2:].any()


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_equals_the_reference_on_the_noise_cases(mav, case):
    fl, fe, sky, gt = _noise(case)
    with _ctx(case.W, case.H, dc.PHI_B) as c:
        for call in rc.CALLS:
            for g in rc.REF_GRIDS:
                a, m = rc.GRIDS[g]
                got = c.roc_sweep(fl, fe, gt, a, m, sky=sky, **rc.sweep_kwargs(call, dc.PHI_B))["counts"]
                for b in range(dc.PHI_B):
                    phi, mag = rc.oracle_fields(fl[b], call.mode(b), fe[b], dc.OMEGA[b], dc.DT[b])
                    assert np.array_equal(got[b], R.ref_counts(phi, mag, sky[b], gt[b], a, m)), (case.name, call.name, g, b)


@pytest.mark.parametrize("shape", rc.PLANTED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planted_fields(mav, shape):
    W, H = shape
    pl, P = rc.planted(W, H), len(rc.PLANTED)
    gt = rc.gt_images(W, H, P)
    plain, frame0 = dc.PhiCall("plain", "stage", "f32"), dc.PhiCall("frame0", "host", "f32", frame0=(1,))
    with _ctx(W, H, P) as c:
        for call in (plain, frame0):
            kw = rc.sweep_kwargs(call, P)
            got = c.roc_sweep(pl["flow"], pl["foe"], gt, rc.ANG, rc.MAG_PLANTED, sky=pl["sky"], **kw)["counts"]
            for k, name in enumerate(rc.PLANTED):
                phi, mag = rc.oracle_fields(pl["flow"][k], call.mode(k), pl["foe"][k])
                assert np.array_equal(got[k], R.ref_counts(phi, mag, pl["sky"][k], gt[k], rc.ANG, rc.MAG_PLANTED)), (shape, call.name, name)
            top = got[rc.PLANTED.index("antiradial")]
            assert top[-1, -1, 2] == np.sum(gt[rc.PLANTED.index("antiradial")] >= 1) and np.all(top[..., 2] == top[-1, -1, 2])
            for g in rc.DEVICE_ONLY_GRIDS:                    # thresholds at 0, 90 and 180: where these fields' phi lies
                a, m = rc.GRIDS[g]
                dev = c.roc_sweep(pl["flow"], pl["foe"], gt, a, m, sky=pl["sky"], **kw)["counts"]
                assert np.array_equal(dev, _route(c, call, pl["flow"], pl["foe"], pl["sky"], gt, a, m, True)), (shape, call.name, g)


def test_more_than_64_pairs(mav):
    W, H, B = rc.LARGE
    lb = rc.large_batch()
    derot = dc.PhiCall("derot", "stage", "f32", rates=True)
    with _ctx(W, H, B) as c:
        got = c.roc_sweep(lb["flow"], lb["foe"], lb["gt"], rc.ANG, rc.MAG, sky=lb["sky"])["counts"]
        for b in range(B):
            phi, mag = rc.oracle_fields(lb["flow"][b], "plain", lb["foe"][b])
            assert np.array_equal(got[b], R.ref_counts(phi, mag, lb["sky"][b], lb["gt"][b], rc.ANG, rc.MAG)), b
        for g in ("one", "right"):
            a, m = rc.GRIDS[g]
            dev = c.roc_sweep(lb["flow"], lb["foe"], lb["gt"], a, m, sky=lb["sky"], **rc.sweep_kwargs(derot, B))["counts"]
            assert np.array_equal(dev, _route(c, derot, lb["flow"], lb["foe"], lb["sky"], lb["gt"], a, m, True)), g


def test_host_form_dev_form_and_last_form_agree(mav):
    from mavflow import _lib
    case = dc.PHI_CASES[dc.PHI_IDS.index("257x19")]
    W, H, B = case.W, case.H, dc.PHI_B
    fl, fe, sky, gt = _noise(case)
    sky8 = sky.astype(np.uint8)
    f0 = np.array([1, 0, 0], np.uint8)
    words = _lib.roc_table_words(len(rc.ANG), len(rc.MAG))
    with _ctx(W, H, B) as c:
        host = c.roc_sweep(fl, fe, gt, rc.ANG, rc.MAG, omega=dc.OMEGA, dt=dc.DT, sky=sky, frame0=f0)["counts"]
        # device pointers; the sky and ground-truth images start one byte into their buffers (the kernel reads them byte by byte)
        bufs = dict(flow=c.alloc(fl.nbytes).upload(fl), foe=c.alloc(fe.nbytes).upload(fe), omega=c.alloc(dc.OMEGA.nbytes).upload(dc.OMEGA),
                    dt=c.alloc(dc.DT.nbytes).upload(dc.DT), f0=c.alloc(8).upload(f0), sky=c.alloc(sky8.nbytes + 1), gt=c.alloc(gt.nbytes + 1),
                    table=c.alloc(8 * words * B))
        _lib.check(c.lib.mav_memcpy_h2d(c.h, bufs["sky"].ptr + 1, _lib._ptr(np.ascontiguousarray(sky8)), sky8.nbytes))
        _lib.check(c.lib.mav_memcpy_h2d(c.h, bufs["gt"].ptr + 1, _lib._ptr(np.ascontiguousarray(gt)), gt.nbytes))
        c.roc_sweep_dev(bufs["flow"], bufs["foe"], bufs["gt"].ptr + 1, B, B, rc.ANG, rc.MAG, bufs["table"], omega_ptr=bufs["omega"],
                        dt_ptr=bufs["dt"], frame0_ptr=bufs["f0"], sky_ptr=bufs["sky"].ptr + 1)
        c.sync()
        dev = _lib.roc_expand(bufs["table"].download(np.int64, (B, words)), len(rc.ANG), len(rc.MAG))
        assert np.array_equal(dev, host)
        for b in bufs.values():
            b.free()
        # what a detection call leaves resident
        fp = _lib.foe_defaults()
        fp.n_pairs, fp.mag_threshold = dc.DETECT_PAIRS, dc.DETECT_GATE
        smp = dc.detect_samples(W, H, B, dc.DETECT_PAIRS)
        det = c.detect(fl, smp, omega=dc.OMEGA, dt=dc.DT, sky=sky, foe_params=fp, frame0=f0)
        last = c.roc_sweep_last(B, gt, rc.ANG, rc.MAG)["counts"]
        again = c.roc_sweep_last(B, gt[1], rc.ANG, rc.MAG)["counts"]          # still resident; one shared image
        with pytest.raises(_lib.MavflowError):                 # MAV_ERR_STATE: another batch ...
            c.roc_sweep_last(B - 1, gt[:B - 1], rc.ANG, rc.MAG)
        want = c.roc_sweep(fl, det["results"]["foe"], gt, rc.ANG, rc.MAG, omega=dc.OMEGA, dt=dc.DT, sky=sky, frame0=f0)["counts"]
        assert np.array_equal(last, want)
        assert np.array_equal(again, c.roc_sweep(fl, det["results"]["foe"], np.stack([gt[1]] * B), rc.ANG, rc.MAG, omega=dc.OMEGA, dt=dc.DT,
                                                 sky=sky, frame0=f0)["counts"])
        with pytest.raises(_lib.MavflowError):                 # ... and another host call in between, exactly as render_last
            c.roc_sweep_last(B, gt, rc.ANG, rc.MAG)
        with pytest.raises(_lib.MavflowError):
            c.render_last(B)
        # the staged loop's route: the float64 field (and a float32 frame-0 field) a phi_mask call left behind
        c.phi_mask(fl.astype(np.float64), fe, sky=sky, want_phi=False)
        assert np.array_equal(c.roc_sweep_last(B, gt, rc.ANG, rc.MAG)["counts"], c.roc_sweep(fl, fe, gt, rc.ANG, rc.MAG, sky=sky)["counts"])
        c.phi_mask(fl, fe, sky=sky, want_phi=False)
        assert np.array_equal(c.roc_sweep_last(B, gt, rc.ANG, rc.MAG)["counts"],
                              c.roc_sweep(fl, fe, gt, rc.ANG, rc.MAG, sky=sky, frame0=[1] * B)["counts"])


def test_shared_ground_truth_repeatable_bytes_and_canary(mav):
    from mavflow import _lib
    case = dc.PHI_CASES[dc.PHI_IDS.index("66x33")]
    W, H, B = case.W, case.H, dc.PHI_B
    fl, fe, sky, gt = _noise(case)
    ptr = _lib._ptr
    with _ctx(W, H, B) as c:
        shared = c.roc_sweep(fl, fe, gt[0], rc.ANG, rc.MAG, sky=sky, omega=dc.OMEGA, dt=dc.DT)["counts"]
        assert np.array_equal(shared, c.roc_sweep(fl, fe, np.stack([gt[0]] * B), rc.ANG, rc.MAG, sky=sky, omega=dc.OMEGA, dt=dc.DT)["counts"])
        # the raw table of two calls: the same bytes, and nothing outside batch x words of an over-allocated one
        p, a, m = _lib.roc_params(rc.ANG, rc.MAG)
        words = _lib.roc_table_words(a.size, m.size)
        sky8, flc, foe = np.ascontiguousarray(sky.astype(np.uint8)), np.ascontiguousarray(fl), np.ascontiguousarray(fe)
        tables = []
        for _ in range(2):
            t = np.full(B * words + 64, CANARY, np.uint64)
            _lib.check(c.lib.mav_roc_sweep(c.h, ptr(flc), ptr(foe), None, None, None, ptr(sky8), ptr(np.ascontiguousarray(gt)), B, B, None,
                                           C.byref(p), ptr(t)))
            assert np.all(t[B * words:] == CANARY)
            tables.append(t)
        assert tables[0].tobytes() == tables[1].tobytes()
        assert np.array_equal(_lib.roc_expand(tables[0][:B * words].view(np.int64), a.size, m.size), c.roc_sweep(fl, fe, gt, rc.ANG, rc.MAG, sky=sky)["counts"])
        # what the ABI refuses, with a live context: ValueError (MAV_ERR_ARG), nothing written
        t = np.full(B * words, CANARY, np.uint64)
        for bad, (ba, bm) in rc.BAD_LISTS.items():
            q, _, _ = _lib.roc_params(ba, bm)
            assert c.lib.mav_roc_sweep(c.h, ptr(flc), ptr(foe), None, None, None, ptr(sky8), ptr(np.ascontiguousarray(gt)), B, B, None,
                                       C.byref(q), ptr(t)) == _lib.MAV_ERR_ARG, bad
            with pytest.raises(ValueError):
                c.roc_arm(ba, bm, 0)
        assert np.all(t == CANARY)
        with pytest.raises(ValueError):                        # gt_images is the batch or 1
            _lib.check(c.lib.mav_roc_sweep(c.h, ptr(flc), ptr(foe), None, None, None, None, ptr(np.ascontiguousarray(gt)), 2, B, None, C.byref(p), ptr(t)))
        with pytest.raises(ValueError):
            c.roc_arm(rc.ANG, rc.MAG, 12)                      # off_table: a multiple of 8
        c.roc_arm(rc.ANG, rc.MAG, 96)
        c.roc_arm(None)

"""mav_gt_stats / mav_gt_stats_dev (csrc/kernels_validation.hip) against tests/validation_ref.py, byte for byte: the records (every
byte, padding included) and the index lists of every case of tests/validation_cases.py; each image of a batch equal to its batch-1
result; two runs equal; the Python layer's convenience fields."""
import ctypes as C

import numpy as np
import pytest

import validation_cases as T
import validation_ref as R

pytestmark = pytest.mark.gpu
CANARY = 0x5A


def _blocks(c, x):
    """the case's arrays as the call takes them (None for what it passes as NULL) and its parameter blocks"""
    from mavflow import _validation as V
    a = {k: (None if k in c.null else np.ascontiguousarray(x[k])) for k in ("gt_flow", "sky", "depth")}
    p = V.gt_stats_params(x["omega"], x["dt"], frame0=c.frame0, legacy_threshold=c.legacy, batch=c.B)
    assert list(p["flags"]) == list(x["flags"])
    return np.ascontiguousarray(x["seg"]), a, p


def run_case(ctx, c, x, images=None):
    """(records (B,), indices (B, max_pixels) or None) of the device for case c (images: a slice of the batch)"""
    from mavflow import _lib, _validation as V
    lib, ptr = V.load(), _lib._ptr
    seg, a, p = _blocks(c, x)
    if images is not None:
        seg, p = np.ascontiguousarray(seg[images]), np.ascontiguousarray(p[images])
        a = {k: (None if v is None else np.ascontiguousarray(v[images])) for k, v in a.items()}
    B = seg.shape[0]
    rec = np.full(B, CANARY, np.uint8).repeat(96).view(V.RECORD_DTYPE)
    idx = None if "indices" in c.null else np.full((B, c.max_pixels), 0x5A5A5A5A, np.int32)
    if c.form == "host":
        _lib.check(lib.mav_gt_stats(ctx.h, ptr(seg), ptr(a["gt_flow"]), ptr(a["sky"]), ptr(a["depth"]), ptr(p), B, c.max_pixels, ptr(rec), ptr(idx)))
        return rec, idx
    bufs = []
    try:
        def up(arr, align, pad_value=None):
            """a device copy whose address is a multiple of `align` and, with min_align, of nothing larger"""
            if arr is None:
                return None
            shift = align if c.min_align else 0
            b = ctx.alloc(arr.nbytes + shift + 64)
            bufs.append(b)
            raw = np.full(arr.nbytes + shift + 64, CANARY, np.uint8)
            raw[shift:shift + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            b.upload(raw)
            assert (b.ptr + shift) % align == 0 and (not c.min_align or (b.ptr + shift) % (2 * align) != 0)
            return b.ptr + shift
        ds, dg, dk, dd, dp = up(seg, 1), up(a["gt_flow"], 8), up(a["sky"], 1), up(a["depth"], 4), up(p, 8)
        dr, di = up(rec, 16), up(idx, 4)
        ctx.gt_stats_enqueue(ds, dg, dk, dd, dp, B, c.max_pixels, dr, di)
        ctx.sync()
        out = []
        for b, host, shift in ((bufs[-2 if idx is not None else -1], rec, 16), (bufs[-1] if idx is not None else None, idx, 4)):
            if b is None:
                out.append(None)
                continue
            shift = shift if c.min_align else 0
            raw = b.download(np.uint8, (host.nbytes + shift + 64,))
            assert (raw[:shift] == CANARY).all() and (raw[shift + host.nbytes:] == CANARY).all(), "bytes around the output were written"
            out.append(raw[shift:shift + host.nbytes].copy().view(host.dtype).reshape(host.shape))
        return out[0], out[1]
    finally:
        for b in bufs:
            b.free()


def _check(c, got, want, what=""):
    rec, idx = got
    wrec, widx = want
    if rec.tobytes() != wrec.tobytes():
        diff = [n for n in rec.dtype.names if rec[n].tobytes() != wrec[n].tobytes()]
        raise AssertionError(f"{c.name}{what}: records differ in {diff}: device {rec[diff]} restatement {wrec[diff]}")
    if idx is not None:
        assert idx.dtype == np.int32 and np.array_equal(idx, widx), f"{c.name}{what}: index lists differ"


@pytest.mark.parametrize("name", list(T.CASES))
def test_device_equals_the_restatement_byte_for_byte(mav, name):
    from mavflow import _lib
    c, x = T.CASES[name], T.inputs(name)
    with _lib.Context(c.W, c.H, c.B) as ctx:
        first = run_case(ctx, c, x)
        _check(c, first, x["ref"])
        second = run_case(ctx, c, x)                                       # the same bytes on every run
        assert second[0].tobytes() == first[0].tobytes() and (first[1] is None or np.array_equal(first[1], second[1]))
        if c.B > 1:                                                        # ... and at every batch position
            for b in range(c.B):
                one = run_case(ctx, c, x, images=slice(b, b + 1))
                _check(c, one, (x["ref"][0][b:b + 1], x["ref"][1][b:b + 1]), f" image {b} alone")


def test_python_layer_fields(mav):
    from mavflow import _lib, im_helpers
    c, x = T.CASES["batch 3"], T.inputs("batch 3")
    wrec, widx = x["ref"]
    with _lib.Context(c.W, c.H, c.B) as ctx:
        out = ctx.gt_stats(x["seg"], x["gt_flow"], x["sky"], x["depth"], omega=x["omega"], dt=x["dt"], max_pixels=c.max_pixels)
        assert out["records"].tobytes() == wrec.tobytes()
        for b in range(c.B):
            n = int(wrec["listed"][b])
            assert out["indices"][b].dtype == np.int32 and np.array_equal(out["indices"][b], widx[b, :n])
            assert out["drone_size_pixels"][b] == wrec["drone_pixels"][b] and isinstance(out["drone_size_pixels"][b], np.int64)
            assert out["box"][b].get_topleft() == (wrec["box"][b][0], wrec["box"][b][1])
            assert out["box"][b].get_bottomright() == (wrec["box"][b][2], wrec["box"][b][3])
            assert out["sky_tpr_fpr"][b] == im_helpers._rates(wrec["sky"][b])
            assert out["drone_flow_avg"][b].tobytes() == R.drone_flow_avg(wrec[b]).tobytes() and not out["truncated"][b]
        # one frame, device handles for seg and gt_flow: the same record, fields unwrapped
        seg_d, gt_d = ctx.alloc(x["seg"][1].nbytes).upload(x["seg"][1]), ctx.alloc(x["gt_flow"][1].nbytes).upload(x["gt_flow"][1])
        try:
            from mavflow import pipeline
            one = ctx.gt_stats(pipeline.DeviceArray(ctx, seg_d.ptr, (c.H, c.W), np.uint8), pipeline.DeviceArray(ctx, gt_d.ptr, (c.H, c.W, 2), np.float32),
                               x["sky"][1], x["depth"][1], omega=x["omega"][1], dt=x["dt"][1], max_pixels=c.max_pixels)
        finally:
            seg_d.free()
            gt_d.free()
        assert one["records"].tobytes() == wrec[1:2].tobytes() and np.array_equal(one["indices"][0], widx[1, :int(wrec["listed"][1])])
        assert one["drone_flow_avg"].tobytes() == R.drone_flow_avg(wrec[1]).tobytes() and one["box"].get_center() == out["box"][1].get_center()
        # an empty drone: NaN as numpy gives; a truncated list: no average
        e = T.inputs("no mav")
        empty = ctx.gt_stats(e["seg"][0], e["gt_flow"][0], e["sky"][0], e["depth"][0], omega=e["omega"][0], dt=e["dt"][0])
        assert empty["drone_size_pixels"] == 0 and np.isnan(empty["drone_flow_avg"]).all() and empty["indices"][0].size == 0
        cut = ctx.gt_stats(x["seg"][0], x["gt_flow"][0], max_pixels=4)
        assert cut["truncated"] and cut["drone_flow_avg"] is None and cut["sky_tpr_fpr"] is None and cut["indices"][0].size == 4
        with pytest.raises(ValueError):
            ctx.gt_stats(x["seg"][0], max_pixels=0)


def test_profile_classes_split_the_phases(mav):
    from mavflow import _lib
    c, x = T.CASES["97x71"], T.inputs("97x71")
    with _lib.Context(c.W, c.H, 1) as ctx:
        ctx.profile_enable(True)
        run_case(ctx, c, x)
        prof = ctx.profile_get()
        ctx.profile_enable(False)
    for k in ("gt_stats_max", "gt_stats_count", "gt_stats_list", "gt_stats_sum"):
        assert prof[k][1] == 1, (k, prof[k])

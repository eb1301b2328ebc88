"""mav_components / mav_components_dev against tests/components_ref.py on every case of tests/components_cases.py: labels, counts and
whole tables equal bit for bit (all results are integers; nothing is excused), the same call twice gives the same bytes, and the
outputs without a label image equal those with one."""
import ctypes as C

import numpy as np
import pytest

import components_cases as CC

pytestmark = pytest.mark.gpu


def _host_call(ctx, case, want_labels=True):
    from mavflow import _lib
    B = len(case.names)
    p = _lib.cc_defaults(connectivity=case.connectivity, min_area=case.min_area, max_blobs=case.max_blobs)
    labels = np.full((B, case.H, case.W), -7, np.int32) if want_labels else None
    counts = np.full(B, -7, np.int32).repeat(2).view(_lib.CC_COUNTS_DTYPE)
    tables = np.frombuffer(bytearray(b"\xa5" * (B * case.max_blobs * 40)), _lib.BLOB_DTYPE).reshape(B, case.max_blobs)
    _lib.check(ctx.lib.mav_components(ctx.h, _lib._ptr(case.masks), B, C.byref(p), _lib._ptr(labels), _lib._ptr(counts), _lib._ptr(tables)))
    return labels, counts, tables


def _dev_call(ctx, case, want_labels):
    """The caller's own device buffers, pre-filled with a pattern: mav_components_dev must write every byte it promises."""
    from mavflow import _lib
    B, n = len(case.names), case.W * case.H
    mask = ctx.alloc(B * n).upload(case.masks)
    labels = ctx.alloc(B * n * 4).upload(np.full(B * n, -7, np.int32)) if want_labels else None
    counts = ctx.alloc(B * 8).upload(np.full(2 * B, -7, np.int32))
    tables = ctx.alloc(B * case.max_blobs * 40).upload(np.full(B * case.max_blobs * 40, 0xA5, np.uint8))
    ctx.components_dev(mask, B, counts, tables, labels_ptr=labels, connectivity=case.connectivity, min_area=case.min_area,
                       max_blobs=case.max_blobs)
    ctx.sync()
    out = (labels.download(np.int32, (B, case.H, case.W)) if want_labels else None, counts.download(_lib.CC_COUNTS_DTYPE, (B,)),
           tables.download(_lib.BLOB_DTYPE, (B, case.max_blobs)))
    for buf in (mask, labels, counts, tables):
        if buf is not None:
            buf.free()
    return out


def _same(got, want, what, case):
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (case.id, what)
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        bad = np.argwhere(got != want)
        pytest.fail(f"{case.id}: {what} differs at {len(bad)} entries, first {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


@pytest.mark.parametrize("cid", [c.id for c in CC.CASES])
def test_components_equal_the_restatement(cid):
    from mavflow import _lib
    case = CC.BY_ID[cid]
    labels, counts, tables = case.expected
    B = len(case.names)
    with _lib.Context(case.W, case.H, B) as ctx:
        if case.cap_mb is not None:
            ctx.set_option("cc_workspace_mb", case.cap_mb)
        first = _host_call(ctx, case)
        for got, want, what in zip(first, (labels, counts, tables), ("labels", "counts", "tables")):
            _same(got, want, what, case)
        again = _host_call(ctx, case)
        for a, b, what in zip(first, again, ("labels", "counts", "tables")):
            assert a.tobytes() == b.tobytes(), (cid, what, "second call")
        bare = _host_call(ctx, case, want_labels=False)
        assert bare[1].tobytes() == counts.tobytes() and bare[2].tobytes() == tables.tobytes(), (cid, "labels NULL")
        for want_labels in (True, False):
            dl, dc, dt = _dev_call(ctx, case, want_labels)
            if want_labels:
                _same(dl, labels, "labels (dev)", case)
            _same(dc, counts, "counts (dev)", case)
            _same(dt, tables, "tables (dev)", case)
        # the scratch is the context's, counted by its ledger and bounded by the cap (or one image)
        per = CC.workspace_per_image(case.W, case.H)
        held = ctx.mem_info()["ctx_bytes"]
        assert held >= per * min(B, max(1, ((256 if case.cap_mb is None else case.cap_mb) << 20) // per))
        if case.cap_mb == 0:
            assert case.sub_batches(per) == B > 1


def test_python_method_trims_the_tables():
    from mavflow import _lib
    case = CC.BY_ID["131x67-trunc-c4"]
    labels, counts, tables = case.expected
    with _lib.Context(case.W, case.H, len(case.names)) as ctx:
        out = ctx.components(case.masks.astype(bool), connectivity=4, min_area=case.min_area, max_blobs=case.max_blobs, labels=True)
        assert np.array_equal(out["labels"], labels)
        assert np.array_equal(out["n_components"], counts["n_components"]) and np.array_equal(out["n_blobs"], counts["n_blobs"])
        for b, blobs in enumerate(out["blobs"]):
            k = min(int(counts["n_blobs"][b]), case.max_blobs)
            assert len(blobs) == k and blobs.tobytes() == tables[b, :k].tobytes()
        assert (counts["n_blobs"] > case.max_blobs).any()                   # the caller sees the truncation
        assert "labels" not in ctx.components(case.masks)


def test_bad_arguments():
    from mavflow import _lib
    W, H = 40, 30
    lib = _lib.load()
    mask = np.ones((1, H, W), np.uint8)
    counts, table = np.zeros(1, _lib.CC_COUNTS_DTYPE), np.zeros((1, 256), _lib.BLOB_DTYPE)
    p = _lib._ptr
    A = _lib.MAV_ERR_ARG
    with _lib.Context(W, H, 1) as ctx:
        h = ctx.h
        before = ctx.mem_info()["ctx_bytes"]
        for fn in (lib.mav_components, lib.mav_components_dev):
            assert fn(h, None, 1, None, None, p(counts), p(table)) == A
            assert fn(h, p(mask), 1, None, None, None, p(table)) == A
            assert fn(h, p(mask), 1, None, None, p(counts), None) == A
            for bad in (dict(connectivity=6), dict(connectivity=0), dict(min_area=0), dict(max_blobs=0), dict(max_blobs=65536), dict(max_blobs=-1)):
                assert fn(h, p(mask), 1, C.byref(_lib.cc_defaults(**bad)), None, p(counts), p(table)) == A, bad
        assert lib.mav_components(h, p(mask), 2, None, None, p(counts), p(table)) == A                  # batch > max_batch
        assert lib.mav_components(h, p(mask), 0, None, None, p(counts), p(table)) == A
        assert ctx.mem_info()["ctx_bytes"] == before                                                    # nothing was allocated or enqueued
        assert lib.mav_last_masks_components(h, 2, 1, None, None, p(counts), p(table)) == A
        assert lib.mav_last_masks_components(h, 0, 1, None, None, p(counts), p(table)) == _lib.MAV_ERR_STATE
        assert lib.mav_components(h, p(mask), 1, None, None, p(counts), p(table)) == _lib.MAV_OK
        assert (int(counts["n_components"][0]), int(counts["n_blobs"][0])) == (1, 1)
        assert tuple(table[0, 0]) == (1, 0, 0, W, H, W * H, H * W * (W - 1) // 2, W * H * (H - 1) // 2)
        with pytest.raises(ValueError):
            ctx.components(mask, connectivity=5)
        with pytest.raises(ValueError):
            ctx.components_last(1, which="both")

"""JPEG decode on the device (include/mavflow_jpeg.h) held to Pillow's pixels (tests/golden/jpeg_frames.npz) and to the host build of
the same decoding source.  Bytes are compared by equality, status records field by field; there is no tolerance anywhere."""
import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
FORMATS = ("samples", "bgr", "gray")


@pytest.fixture(scope="module")
def ctx(mav):
    from mavflow import _lib
    with _lib.Context(131, 67, 2) as c:
        yield c


def _info_of(case):
    """the parser's info; for a file it refuses, the all-zero info it leaves, sent with a call of 8 x 8 x 1"""
    from mavflow import _lib
    info, _ = _lib.jpeg_info(case.file)
    return np.zeros(1, _lib.JPEG_INFO_DTYPE) if info is None else info


def _shape_of(case, info):
    return (8, 8, 1) if info["W"][0] == 0 else (int(info["W"][0]), int(info["H"][0]), int(info["components"][0]))


def _pack(cases):
    from mavflow import _lib
    infos = np.concatenate([_info_of(c) for c in cases])
    sizes = np.array([len(c.file) for c in cases], np.uint64)
    index = np.stack([np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64), sizes], 1)
    return np.frombuffer(b"".join(c.file for c in cases) + b"\0", np.uint8), index, infos


_HOST = {}


def _host(case, fmt, shape):
    """mav_jpeg_decode_host's pixels and status for the case as the device call sees it"""
    from mavflow import _lib
    key = (case.name, fmt)
    if key not in _HOST:
        W, H, comps = shape
        oc = {"samples": comps, "bgr": 3, "gray": 1}[fmt]
        raw = np.frombuffer(case.file + b"\0", np.uint8)
        info = _info_of(case)
        img, st = np.zeros((H, W, oc), np.uint8), np.zeros(1, _lib.JPEG_STATUS_DTYPE)
        if info["W"][0] == 0:
            st["code"] = jc.E["UNSUPPORTED"]                    # (the host form has no call sizes to hold the info against)
        else:
            _lib.check(_lib.load().mav_jpeg_decode_host(raw.ctypes.data, len(case.file), info.ctypes.data, _lib.JPEG_OUT[fmt], img.ctypes.data,
                                                        st.ctypes.data))
        _HOST[key] = (img[..., 0] if oc == 1 else img, st[0])
    return _HOST[key]


def _hold(cases, fmt, shape, imgs, status):
    for k, c in enumerate(cases):
        want, st = _host(c, fmt, shape)
        assert status[k].tobytes() == st.tobytes(), (c.name, fmt, status[k], st)
        assert status[k]["code"] == (jc.E["UNSUPPORTED"] if c.parser is not None else c.code), (c.name, status[k])     # (a refused file's info is all zero)
        assert np.array_equal(imgs[k], want), (c.name, fmt)
        if c.code:
            assert not imgs[k].any(), c.name
        elif fmt == "bgr":
            assert np.array_equal(imgs[k], c.bgr), c.name
        if c.parser is None:
            assert c.claim({n: int(status[k][n]) for n in status.dtype.names}), (c.name, status[k])


def _dev_call(ctx, cases, fmt, shape, poison=0xFF):
    """mav_jpeg_decode_dev with pointers from ctx.alloc; scratch, output and statuses poisoned before the call"""
    from mavflow import _lib
    W, H, comps = shape
    packed, index, infos = _pack(cases)
    n = len(cases)
    oc = {"samples": comps, "bgr": 3, "gray": 1}[fmt]
    scratch = ctx.jpeg_decode_scratch_bytes(W, H, comps, n)
    bufs = [ctx.alloc(packed.nbytes).upload(packed), ctx.alloc(index.nbytes).upload(index), ctx.alloc(infos.nbytes).upload(infos),
            ctx.alloc(n * H * W * oc).upload(np.full(n * H * W * oc, 0xAB, np.uint8)),
            ctx.alloc(40 * n).upload(np.full(40 * n, poison, np.uint8)), ctx.alloc(scratch).upload(np.full(scratch, poison, np.uint8))]
    try:
        ctx.jpeg_decode_dev(bufs[0], bufs[1], bufs[2], n, W, H, fmt, bufs[3], bufs[4], bufs[5])
        status = bufs[4].download(_lib.JPEG_STATUS_DTYPE, (n,))
        imgs = bufs[3].download(np.uint8, (n, H, W, oc))
    finally:
        ctx.sync()
        for b in bufs:
            b.free()
    return (imgs[..., 0] if oc == 1 else imgs), status


def test_every_case_through_the_host_pointer_form(ctx):
    for c in jc.cases():
        packed, index, infos = _pack([c])
        shape = _shape_of(c, infos)
        for fmt in FORMATS:
            imgs, status = ctx.jpeg_decode_packed(packed, index, infos, shape[0], shape[1], fmt, return_status=True)
            _hold([c], fmt, shape, imgs, status)


def test_every_case_through_the_device_pointer_form_with_poisoned_scratch(ctx):
    for c in jc.cases():
        shape = _shape_of(c, _info_of(c))
        imgs, status = _dev_call(ctx, [c], "bgr", shape)
        _hold([c], "bgr", shape, imgs, status)


def _batch_33x31():
    pool = [c for c in jc.valid() if c.name.startswith("pil_33x31_") and "gray" not in c.name]
    assert len({c.name.split("_")[2] for c in pool}) == 3 and any("rmb2" in c.name for c in pool) and any("plain" in c.name for c in pool)
    return pool


@pytest.mark.parametrize("count", [1, 3, 65])
def test_batches_of_mixed_samplings_and_restart_intervals(ctx, count):
    pool = _batch_33x31()
    cases = [pool[k % len(pool)] for k in range(count)]
    packed, index, infos = _pack(cases)
    for fmt in FORMATS:
        imgs, status = ctx.jpeg_decode_packed(packed, index, infos, 33, 31, fmt, return_status=True)
        _hold(cases, fmt, (33, 31, 3), imgs, status)
    imgs, status = _dev_call(ctx, cases, "bgr", (33, 31, 3), poison=0x5A)
    _hold(cases, "bgr", (33, 31, 3), imgs, status)


def test_refused_images_are_zero_and_their_neighbours_intact(ctx):
    pool = _batch_33x31()
    bad = {0: "restart_marker_missing", 31: "restart_marker_wrong_number", 64: "restart_marker_surplus"}
    by_name = {c.name: c for c in jc.cases()}
    cases = [by_name[bad[k]] if k in bad else pool[k % len(pool)] for k in range(65)]
    imgs, status = _dev_call(ctx, cases, "bgr", (33, 31, 3))
    _hold(cases, "bgr", (33, 31, 3), imgs, status)
    assert [k for k in range(65) if status["code"][k]] == [0, 31, 64]
    with pytest.raises(ValueError, match=r"file 0: MAV_JPEG_E_RESTART \(4\).*files \[0, 31, 64\] failed"):
        ctx.jpeg_decode([c.file for c in cases])


def test_an_info_the_parser_would_not_produce_is_refused_on_the_device(ctx):
    pool = _batch_33x31()
    packed, index, infos = _pack(pool[:3])
    infos = infos.copy()
    infos["comp"][1, 0]["ta"] = 3                                  # an AC table no DHT defined
    imgs, status = ctx.jpeg_decode_packed(packed, index, infos, 33, 31, "bgr", return_status=True)
    assert status["code"].tolist() == [0, jc.E["UNSUPPORTED"], 0] and not imgs[1].any()
    assert np.array_equal(imgs[0], pool[0].bgr) and np.array_equal(imgs[2], pool[2].bgr)


def test_two_calls_in_a_row_with_different_sizes(ctx):
    a = next(c for c in jc.valid() if c.name.startswith("pil_70x130_420"))
    b = next(c for c in jc.valid() if c.name.startswith("pil_9x17_422"))
    for _ in range(2):
        for c, shape in ((a, (70, 130, 3)), (b, (9, 17, 3))):
            imgs, status = _dev_call(ctx, [c], "bgr", shape)
            _hold([c], "bgr", shape, imgs, status)


def test_python_forms(ctx):
    pool = _batch_33x31()
    files = [c.file for c in pool]
    assert np.array_equal(ctx.jpeg_decode(files), np.stack([c.bgr for c in pool]))
    d_out, shape = ctx.jpeg_decode_to_device(files, "gray")
    try:
        assert shape == (len(pool), 31, 33)
        assert np.array_equal(d_out.download(np.uint8, shape), ctx.jpeg_decode(files, "gray"))
    finally:
        d_out.free()
    with pytest.raises(ValueError, match="file 1 is 70 x 130 x 3, file 0 is 33 x 31 x 3"):
        ctx.jpeg_decode([files[0], next(c for c in jc.valid() if c.name.startswith("pil_70x130_444")).file])
    with pytest.raises(ValueError, match="file 0: MAV_JPEG_E_UNSUPPORTED.*SOF2"):
        ctx.jpeg_decode([next(c for c in jc.cases() if c.name == "pil_progressive").file])

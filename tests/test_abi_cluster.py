"""The C boundary of include/mavflow_cluster.h: the header declares and the cross-compiled library exports every entry point of
mavflow.clustering.EXPORTS (none of them in include/mavflow.h or _lib.EXPORTS), the layouts of mav_kmeans_params and mav_kmeans_record
match their Python mirrors (a small C program compiled against the header, here and now), and calls that must be refused are refused with
MAV_ERR_ARG, the function's name in the message and the outputs untouched -- whatever the arguments alone decide, before the context is
looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_cluster.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, clustering
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_kmeans[a-z0-9_]*)\s*\(", txt)
    assert sorted(declared) == sorted(clustering.EXPORTS)
    lib = clustering.load()
    for s in clustering.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    for other in ("mavflow.h", "mavflow_truth.h", "mavflow_validation.h"):
        main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert "kmeans" not in main
    for phrase in ('#include "mavflow.h"', "THE ORDER OF THE SUMS depends on N alone", "the FIRST k minimising", "the HIGHEST index among equals",
                   "FIRST strictly smallest compactness", "No floating-point atomic", "every byte is written"):
        assert phrase in raw, phrase
    for member in ("kmeans", "kmeans_enqueue", "kmeans_workspace_bytes", "kmeans_paint", "kmeans_paint_enqueue"):
        assert hasattr(_lib.Context, member), member
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_cluster.o") == 4             # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_cluster.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2]


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, clustering as K
    import kmeans_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_cluster.h"', "int main(void) {",
             '  printf("mav_kmeans_params %zu\\n", sizeof(mav_kmeans_params));', '  printf("mav_kmeans_record %zu\\n", sizeof(mav_kmeans_record));']
    for struct, mirror in (("mav_kmeans_params", K.KmeansParams), ("mav_kmeans_record", K.KmeansRecord)):
        for name, _ in mirror._fields_:
            lines.append(f'  printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));')
    for macro in ("MAV_KMEANS_F32", "MAV_KMEANS_U8", "MAV_KMEANS_MAX_K", "MAV_KMEANS_MAX_ATTEMPTS", "MAV_KMEANS_MAX_DIMS", "MAV_KMEANS_MAX_N", "MAV_KMEANS_CHUNK"):
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_kmeans_params"] == C.sizeof(K.KmeansParams) == 32
    assert got["mav_kmeans_record"] == C.sizeof(K.KmeansRecord) == K.RECORD_DTYPE.itemsize == 96 and 96 % 16 == 0
    for name, _ in K.KmeansParams._fields_:
        assert got[f"mav_kmeans_params.{name}"] == getattr(K.KmeansParams, name).offset, name
    for name, _ in K.KmeansRecord._fields_:
        assert got[f"mav_kmeans_record.{name}"] == getattr(K.KmeansRecord, name).offset == K.RECORD_DTYPE.fields[name][1], name
    assert K.RECORD_DTYPE == R.RECORD_DTYPE                                  # the restatement's records are the library's
    assert sum(K.RECORD_DTYPE.fields[n][0].itemsize for n in K.RECORD_DTYPE.names) == 96       # no padding inside or behind
    assert (got["MAV_KMEANS_F32"], got["MAV_KMEANS_U8"]) == (K.KMEANS_F32, K.KMEANS_U8) == (0, 1)
    assert (got["MAV_KMEANS_MAX_K"], got["MAV_KMEANS_MAX_ATTEMPTS"], got["MAV_KMEANS_MAX_DIMS"], got["MAV_KMEANS_CHUNK"]) == \
        (K.KMEANS_MAX_K, K.KMEANS_MAX_ATTEMPTS, K.KMEANS_MAX_DIMS, K.KMEANS_CHUNK) == (16, 16, 4, 4096)
    assert got["MAV_KMEANS_MAX_N"] == 1 << 30
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct


def test_defaults_and_workspace_query(mav):
    from mavflow import clustering as K
    lib = K.load()
    p = K.KmeansParams()
    p.flags = 7
    lib.mav_kmeans_defaults(C.byref(p))
    assert (p.K, p.attempts, p.max_iter, p.dims, p.depth, p.flags, p.eps) == (8, 10, 10, 3, K.KMEANS_F32, 0, 1.0)
    lib.mav_kmeans_defaults(None)                                           # harmless
    a = lib.mav_kmeans_workspace_bytes(1920 * 1080 // 3, 1, C.byref(p))
    assert a > 10 * (1920 * 1080 // 3) and a % 16 == 0                      # at least the per-attempt u8 labels
    assert lib.mav_kmeans_workspace_bytes(1920 * 1080 // 3, 4, C.byref(p)) == 4 * a
    assert lib.mav_kmeans_workspace_bytes(7, 1, C.byref(p)) == 0 and lib.mav_kmeans_workspace_bytes(100, 0, C.byref(p)) == 0
    assert lib.mav_kmeans_workspace_bytes(100, 1, None) == 0
    q = K.kmeans_params(K=4, attempts=2, dims=1, dtype=np.uint8)
    assert (q.K, q.attempts, q.dims, q.depth) == (4, 2, 1, K.KMEANS_U8)
    assert 0 < lib.mav_kmeans_workspace_bytes(100, 1, C.byref(q)) < a
    with pytest.raises(TypeError):
        K.kmeans_params(dtype=np.float64)


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, clustering as K
    lib, ptr = K.load(), _lib._ptr
    x = np.ones((64, 3), np.float32)
    init = np.ones((10, 8, 3), np.float32)
    labels = np.full(64, CANARY, np.uint64)
    centers = np.full(64, CANARY, np.uint64)
    rec = np.full(96 // 8 + 8, CANARY, np.uint64)
    ws = np.full(1 << 16, CANARY, np.uint64)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    good = K.kmeans_params()
    s, i, l, c, r, w, p = ptr(x), ptr(init), ptr(labels), ptr(centers), ptr(rec), ptr(ws), C.cast(C.byref(good), C.c_void_p)
    assert r.value % 16 == 0 and w.value % 16 == 0
    off = lambda v, n: C.c_void_p(v.value + n)
    keep = []

    def bad(**kw):
        q = K.kmeans_params()
        for key, v in kw.items():
            setattr(q, key, v)
        keep.append(q)
        return C.cast(C.byref(q), C.c_void_p)

    for name in ("mav_kmeans", "mav_kmeans_dev"):
        fn = getattr(lib, name)
        tail = (w, ws.nbytes) if name.endswith("_dev") else ()
        ok = (fake_ctx, s, 64, 1, p, i, l, c, r) + tail
        sub = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        calls = {"NULL context": sub(0, None), "NULL samples": sub(1, None), "NULL params": sub(4, None), "NULL init": sub(5, None),
                 "NULL labels": sub(6, None), "NULL centers": sub(7, None), "NULL records": sub(8, None), "batch 0": sub(3, 0), "batch -2": sub(3, -2),
                 "n 7": sub(2, 7), "n -1": sub(2, -1), "K 0": sub(4, bad(K=0)), "K 17": sub(4, bad(K=17)), "attempts 0": sub(4, bad(attempts=0)),
                 "attempts 17": sub(4, bad(attempts=17)), "dims 0": sub(4, bad(dims=0)), "dims 5": sub(4, bad(dims=5)), "depth 2": sub(4, bad(depth=2)),
                 "max_iter 0": sub(4, bad(max_iter=0)), "flags 0x1": sub(4, bad(flags=1)), "eps is not finite": sub(4, bad(eps=float("nan")))}
        if name.endswith("_dev"):
            calls.update({"samples is not aligned": sub(1, off(s, 2)), "init is not aligned": sub(5, off(i, 2)), "labels is not aligned": sub(6, off(l, 2)),
                          "centers is not aligned": sub(7, off(c, 2)), "records is not aligned": sub(8, off(r, 8)), "workspace is not aligned": sub(9, off(w, 8)),
                          "NULL workspace": sub(9, None), "workspace of 64 bytes": sub(10, 64)})
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)
    lut_res, lut_mask = np.full(64, CANARY, np.uint64), np.full(64, CANARY, np.uint64)
    lab32, cen = np.zeros(64, np.int32), np.ones((8, 3), np.float32)
    for name in ("mav_kmeans_paint", "mav_kmeans_paint_dev"):
        fn = getattr(lib, name)
        ok = (fake_ctx, ptr(lab32), ptr(cen), 64, 1, 8, 3, ptr(lut_res), ptr(lut_mask))
        sub = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        calls = {"NULL context": sub(0, None), "NULL labels": sub(1, None), "NULL centers": sub(2, None), "NULL res": sub(7, None), "n 7": sub(3, 7),
                 "batch 0": sub(4, 0), "K 17": sub(5, 17), "dims 5": sub(6, 5)}
        if name.endswith("_dev"):
            calls.update({"labels is not aligned": sub(1, off(ptr(lab32), 2)), "centers is not aligned": sub(2, off(ptr(cen), 2))})
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)
    for a in (labels, centers, rec, ws, lut_res, lut_mask):
        assert np.all(a == CANARY)


def test_python_layer(mav):
    from mavflow import clustering as K
    x = np.arange(24, dtype=np.float32).reshape(8, 3)
    a, b = K.random_centers(x, 4, 3, rng=11), K.random_centers(x, 4, 3, rng=np.random.default_rng(11))
    assert a.shape == (3, 4, 3) and a.dtype == np.float32 and np.array_equal(a, b)
    lo, hi = x.min(0), x.max(0)
    span = hi - lo
    assert np.all(a >= lo - span / 3 - 1e-4) and np.all(a <= hi + span / 3 + 1e-4)       # the box with its margin 1 / D
    np.random.seed(3)
    c = K.random_centers(x, 4, 3, rng=np.random)
    np.random.seed(3)
    assert np.array_equal(c, K.random_centers(x, 4, 3, rng=np.random)) and not np.array_equal(a, c)
    assert K.random_centers(np.stack([x, x + 5]), 2, 2, rng=1).shape == (2, 2, 2, 3)
    assert (K.KMEANS_RANDOM_CENTERS, K.KMEANS_PP_CENTERS, K.KMEANS_USE_INITIAL_LABELS, K.TERM_CRITERIA_EPS, K.TERM_CRITERIA_MAX_ITER) == (0, 2, 1, 2, 1)
    crit = (K.TERM_CRITERIA_EPS + K.TERM_CRITERIA_MAX_ITER, 10, 1.0)
    for flag in (K.KMEANS_PP_CENTERS, K.KMEANS_USE_INITIAL_LABELS):
        with pytest.raises(NotImplementedError):
            K.kmeans(x, 2, None, crit, 3, flag)
    with pytest.raises(TypeError):
        K.kmeans(x.astype(np.float64), 2, None, crit, 3, K.KMEANS_RANDOM_CENTERS)


def test_detector_has_the_switch_off(mav):
    import inspect
    from mavflow.detector import Detector
    sig = inspect.signature(Detector.clustering)
    assert list(sig.parameters) == ["self", "img", "enable_raw"] and sig.parameters["enable_raw"].default is False

    class DS:
        capture_size = (64, 48)
    d = Detector(DS(), Detector.Algorithm.HOMOGRAPHY)
    assert d.use_clustering is False and d.cluster_rng is None
    with pytest.raises(ValueError):
        d.clustering(np.zeros((4, 5), np.float32))                          # numpy's: 20 values are no triples

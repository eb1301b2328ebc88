"""The C boundary of include/mavflow_affine.h: the header declares and the cross-compiled library exports exactly
mavflow.affine.EXPORTS (none of them in another header or in _lib.EXPORTS), a host form and a _dev form of each call, the params' and the
record's size and offsets match the Python mirrors (a small C program compiled against the header, here and now), and calls that must be
refused from their arguments alone are refused with MAV_ERR_ARG, the function's name in the message and the outputs untouched -- before
the context is looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_affine.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, affine
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_(?:affine|estimate_affine|flow_affine)[a-z0-9_]*)\s*\(", txt)
    assert sorted(declared) == sorted(affine.EXPORTS) and len(declared) == 6
    lib = affine.load()
    for s in affine.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    for s in ("mav_estimate_affine", "mav_flow_affine"):   # a host form and a _dev form each
        assert s in affine.EXPORTS and s + "_dev" in affine.EXPORTS
    for other in ("mavflow.h", "mavflow_truth.h", "mavflow_validation.h", "mavflow_cluster.h", "mavflow_warp.h"):
        main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not re.search(r"mav_affine_|mav_estimate_affine|mav_flow_affine", main), other
    for phrase in ('#include "mavflow.h"', "NOT pinned against a cv2 build", "float32 Point2f", "subset check", "Levenberg-Marquardt", "getSubset retry loop",
                   "THE HOST BUILDS need[]", "THE LIBRARY FILLS IT", "The first of equal counts wins", "every byte is written", "RANK TEST",
                   "A refused call has enqueued and written nothing"):
        assert phrase in raw, phrase
    for member in ("estimate_affine", "flow_affine"):
        assert hasattr(_lib.Context, member) and hasattr(_lib.Context, member + "_enqueue"), member
    assert hasattr(_lib.Context, "estimate_affine_workspace_bytes")
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_affine.o") == 4              # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_affine.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2]
    prereq = [line for line in mk.split("\n") if line.startswith("$(BUILD)/mavflow.o:")][0]
    assert "mavflow_affine.h" in prereq


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, affine as K
    import affine_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_affine.h"', "int main(void) {", "  mav_affine_params p;",
             '  printf("mav_affine_record %zu\\n", sizeof(mav_affine_record));', '  printf("mav_affine_params %zu\\n", sizeof(mav_affine_params));']
    for name, _ in K.AffineRecord._fields_:
        lines.append(f'  printf("mav_affine_record.{name} %zu\\n", offsetof(mav_affine_record, {name}));')
    for name, _ in K.AffineParams._fields_:
        lines.append(f'  printf("mav_affine_params.{name} %zu\\n", offsetof(mav_affine_params, {name}));')
    for macro in ("MAV_AFFINE_MAX_PAIRS", "MAV_AFFINE_MAX_ITERS", "MAV_HOMOGRAPHY_MAX_PAIRS"):
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("rank_ratio_e15 %d\\n", (int)(MAV_AFFINE_RANK_RATIO * 1e15 + 0.5));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  (void)p; return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_affine_record"] == C.sizeof(K.AffineRecord) == K.RECORD_DTYPE.itemsize == 32 and got["mav_affine_record"] % 16 == 0
    assert got["mav_affine_params"] == C.sizeof(K.AffineParams) == 32
    for name, _ in K.AffineRecord._fields_:
        assert got[f"mav_affine_record.{name}"] == getattr(K.AffineRecord, name).offset == K.RECORD_DTYPE.fields[name][1], name
    for name, _ in K.AffineParams._fields_:
        assert got[f"mav_affine_params.{name}"] == getattr(K.AffineParams, name).offset, name
    assert [got[f"mav_affine_record.{n}"] for n in ("ok", "inliers", "best_iter", "iters_run", "valid", "refined", "sq_error")] == [0, 4, 8, 12, 16, 20, 24]
    assert K.RECORD_DTYPE == R.RECORD_DTYPE                                  # the restatement's records are the library's
    assert got["MAV_AFFINE_MAX_PAIRS"] == got["MAV_HOMOGRAPHY_MAX_PAIRS"] == K.AFFINE_MAX_PAIRS == R.MAX_PAIRS == 65536
    assert got["MAV_AFFINE_MAX_ITERS"] == K.AFFINE_MAX_ITERS == R.MAX_ITERS == 4096
    assert got["rank_ratio_e15"] == 1000 and K.AFFINE_RANK_RATIO == R.RANK_RATIO == 1e-12
    assert (K.RANSAC, K.LMEDS) == (8, 4)                                     # cv2's values
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct
    p = K.AffineParams()
    K.load().mav_affine_defaults(C.byref(p))
    assert (p.threshold, p.confidence, p.max_iters, p.refine, p.flags) == (3.0, 0.99, 2000, 1, 0)


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, affine as K
    lib, ptr = K.load(), _lib._ptr
    n, mi = 8, 4
    src = np.arange(2.0 * n + 2)
    flow = np.ones(64, np.float32)
    coords = np.zeros((n, 2), np.int32)
    tri = np.array([[0, 1, 2], [3, 4, 5], [1, 2, 3], [5, 6, 7]], np.int32)
    M, inl, rec, ws = (np.full(64, CANARY, np.uint64) for _ in range(4))
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    off = lambda v, k: C.c_void_p(v.value + k)

    def params(**kw):
        p = K.affine_params(max_iters=mi)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.cast(C.pointer(p), C.c_void_p), p

    good, keep = params()
    bad_params = {"threshold -1": params(threshold=-1.0), "threshold nan": params(threshold=float("nan")), "threshold inf": params(threshold=float("inf")),
                  "confidence 0": params(confidence=0.0), "confidence 1": params(confidence=1.0), "confidence nan": params(confidence=float("nan")),
                  "flags 0x1": params(flags=1), "max_iters 0": params(max_iters=0), "max_iters 4097": params(max_iters=4097)}

    def run(name, ok, calls):
        fn = getattr(lib, name)
        sub = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        for what, (k, v) in calls.items():
            assert fn(*sub(k, v)) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)

    for name in K.EXPORTS[2:]:
        dev, flow_form = name.endswith("_dev"), "flow" in name
        a, b = ("flow", "coords") if flow_form else ("src", "dst")
        calls = {"NULL context": (0, None), f"NULL {a}": (1, None), f"NULL {b}": (2, None), "n 2": (3, 2), "n 65537": (3, 65537), "batch 0": (4, 0),
                 "batch -2": (4, -2), "NULL params": (5, None), "NULL triples": (6, None), "NULL M": (7, None), "NULL inliers": (8, None),
                 "NULL records": (9, None)}
        calls.update({what: (5, p[0]) for what, p in bad_params.items()})
        ok = (fake_ctx, ptr(flow) if flow_form else ptr(src), ptr(coords) if flow_form else ptr(src), n, 1, good, ptr(tri), ptr(M), ptr(inl), ptr(rec))
        if dev:
            ok += (ptr(ws), 1 << 30)
            calls.update({"NULL workspace": (10, None), "workspace of 16 bytes": (11, 16), f"{a} is not aligned": (1, off(ok[1], 4)),
                          "triples is not aligned": (6, off(ptr(tri), 2)), "M is not aligned": (7, off(ptr(M), 4)),
                          "records is not aligned": (9, off(ptr(rec), 8)), "workspace is not aligned": (10, off(ptr(ws), 8))})
            if not flow_form:
                calls["dst is not aligned"] = (2, off(ok[2], 4))
        else:
            if flow_form:
                ok += (None,)
            for what, t in {"triples[1][2] = 8 outside": (3, 4, 8), "triples[1][0] = -1 outside": (-1, 4, 5), "triples[1] = (3, 4, 3) repeats": (3, 4, 3)}.items():
                tt = tri.copy()
                tt[1] = t
                calls[what] = (6, ptr(tt))
                calls[what + " "] = (6, ptr(tt))               # (keeps tt alive until run() has used it)
        run(name, ok, calls)
    assert lib.mav_estimate_affine_workspace_bytes(2, 1, good) == 0 and b"mav_estimate_affine_workspace_bytes:" in lib.mav_last_error()
    assert lib.mav_estimate_affine_workspace_bytes(8, 0, good) == 0
    assert lib.mav_estimate_affine_workspace_bytes(8, 1, bad_params["flags 0x1"][0]) == 0
    small, large = lib.mav_estimate_affine_workspace_bytes(8, 1, good), lib.mav_estimate_affine_workspace_bytes(1000, 64, good)
    assert 0 < small < large and small % 16 == 0
    for a in (M, inl, rec, ws):
        assert np.all(a == CANARY)


def test_python_layer_refuses_what_is_not_built(mav):
    import inspect
    import pytest
    from mavflow import affine as K
    from mavflow.detector import Detector
    pts = np.zeros((5, 2), np.float32)
    with pytest.raises(NotImplementedError):
        K.estimateAffine2D(pts, pts, method=K.LMEDS)
    with pytest.raises(ValueError):
        K.estimateAffine2D(pts, pts, method=0)
    assert list(inspect.signature(K.estimateAffine2D).parameters) == ["from_", "to", "inliers", "method", "ransacReprojThreshold", "maxIters", "confidence",
                                                                      "refineIters", "rng"]
    sig = inspect.signature(K.estimateAffine2D).parameters
    assert (sig["method"].default, sig["ransacReprojThreshold"].default, sig["maxIters"].default, sig["confidence"].default, sig["refineIters"].default) == \
        (K.RANSAC, 3, 2000, 0.99, 10)
    assert list(inspect.signature(Detector.get_transformation_matrix).parameters) == ["self", "orig_frame", "flow_uv"]

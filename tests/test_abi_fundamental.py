"""The C boundary of include/mavflow_fundamental.h: the header declares and the cross-compiled library exports exactly
mavflow.fundamental.EXPORTS (none of them in another header or in _lib.EXPORTS), a host form and a _dev form of each call, the params'
and the records' size and offsets match the Python mirrors (a small C program compiled against the header, here and now), and calls that
must be refused from their arguments alone are refused with MAV_ERR_ARG, the function's name in the message and the outputs untouched --
before the context is looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_fundamental.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, fundamental
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_(?:fundamental|find_fundamental|flow_fundamental|epipolar)[a-z0-9_]*)\s*\(", txt)
    assert sorted(declared) == sorted(fundamental.EXPORTS) and len(declared) == 8
    lib = fundamental.load()
    for s in fundamental.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    for s in ("mav_find_fundamental", "mav_flow_fundamental", "mav_epipolar_residual"):   # a host form and a _dev form each
        assert s in fundamental.EXPORTS and s + "_dev" in fundamental.EXPORTS
    for other in ("mavflow.h", "mavflow_truth.h", "mavflow_validation.h", "mavflow_cluster.h", "mavflow_warp.h", "mavflow_affine.h"):
        main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not re.search(r"mav_fundamental_|mav_find_fundamental|mav_flow_fundamental|mav_epipolar", main), other
    for phrase in ('#include "mavflow.h"', "AS REMEMBERED, PINNED TO NO cv2 BUILD", "float32 point arithmetic", "SVD null space", "solveCubic",
                   "F[2][2] = 1", "direct 7-point path at n == 7", "getSubset retry loop", "THE HOST BUILDS need[]", "first of equal counts wins",
                   "every byte is written", "FULL PIVOTING", "BISECTION", "det3(m) =", "A refused call has enqueued and written nothing"):
        assert phrase in raw, phrase
    for member in ("find_fundamental", "flow_fundamental", "epipolar_residual"):
        assert hasattr(_lib.Context, member) and hasattr(_lib.Context, member + "_enqueue"), member
    assert hasattr(_lib.Context, "find_fundamental_workspace_bytes")
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_fundamental.o") == 4         # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_fundamental.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2]
    prereq = [line for line in mk.split("\n") if line.startswith("$(BUILD)/mavflow.o:")][0]
    assert "mavflow_fundamental.h" in prereq


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, fundamental as K
    import fundamental_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    structs = {"mav_fundamental_params": K.FundamentalParams, "mav_fundamental_record": K.FundamentalRecord, "mav_epipolar_record": K.EpipolarRecord}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_affine.h"', '#include "mavflow_fundamental.h"', "int main(void) {"]
    for sname, mirror in structs.items():
        lines.append(f'  printf("{sname} %zu\\n", sizeof({sname}));')
        for name, _ in mirror._fields_:
            lines.append(f'  printf("{sname}.{name} %zu\\n", offsetof({sname}, {name}));')
    for macro in ("MAV_FUNDAMENTAL_MAX_PAIRS", "MAV_FUNDAMENTAL_MAX_ITERS", "MAV_AFFINE_MAX_PAIRS"):
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for sname, mirror in structs.items():
        assert got[sname] == C.sizeof(mirror) == 32, sname
        for name, _ in mirror._fields_:
            assert got[f"{sname}.{name}"] == getattr(mirror, name).offset, (sname, name)
    for name in K.RECORD_DTYPE.names:
        assert got[f"mav_fundamental_record.{name}"] == K.RECORD_DTYPE.fields[name][1], name
    for name in K.EPI_DTYPE.names:
        assert got[f"mav_epipolar_record.{name}"] == K.EPI_DTYPE.fields[name][1], name
    assert [got[f"mav_fundamental_record.{n}"] for n in ("ok", "inliers", "best_iter", "best_slot", "iters_run", "valid", "sq_error")] == [0, 4, 8, 12, 16, 20, 24]
    assert K.RECORD_DTYPE == R.RECORD_DTYPE and K.EPI_DTYPE == R.EPI_DTYPE   # the restatement's records are the library's
    assert got["MAV_FUNDAMENTAL_MAX_PAIRS"] == got["MAV_AFFINE_MAX_PAIRS"] == K.FUNDAMENTAL_MAX_PAIRS == R.MAX_PAIRS == 65536
    assert got["MAV_FUNDAMENTAL_MAX_ITERS"] == K.FUNDAMENTAL_MAX_ITERS == R.MAX_ITERS == 4096
    assert (K.FM_7POINT, K.FM_8POINT, K.FM_LMEDS, K.FM_RANSAC) == (1, 2, 4, 8)        # cv2's values
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct
    p = K.FundamentalParams()
    K.load().mav_fundamental_defaults(C.byref(p))
    assert (p.threshold, p.confidence, p.max_iters, p.flags) == (3.0, 0.99, 1000, 0)


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, fundamental as K
    lib, ptr = K.load(), _lib._ptr
    n, mi = 9, 3
    src = np.arange(2.0 * n + 2)
    flow = np.ones(64, np.float32)
    coords = np.zeros((n, 2), np.int32)
    sub = np.array([[0, 1, 2, 3, 4, 5, 6], [2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 1]], np.int32)
    Fm, inl, rec, ws, res, mask = (np.full(64, CANARY, np.uint64) for _ in range(6))
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    off = lambda v, k: C.c_void_p(v.value + k)

    def params(**kw):
        p = K.fundamental_params(max_iters=mi)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.cast(C.pointer(p), C.c_void_p), p

    good, keep = params()
    bad_params = {"threshold -1": params(threshold=-1.0), "threshold nan": params(threshold=float("nan")), "threshold inf": params(threshold=float("inf")),
                  "confidence 0": params(confidence=0.0), "confidence 1": params(confidence=1.0), "confidence nan": params(confidence=float("nan")),
                  "flags 0x1": params(flags=1), "max_iters 0": params(max_iters=0), "max_iters 4097": params(max_iters=4097)}

    def run(name, ok, calls):
        fn = getattr(lib, name)
        put = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        for what, (k, v) in calls.items():
            assert fn(*put(k, v)) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)

    for name in K.EXPORTS[2:6]:
        dev, flow_form = name.endswith("_dev"), "flow" in name
        a, b = ("flow", "coords") if flow_form else ("src", "dst")
        calls = {"NULL context": (0, None), f"NULL {a}": (1, None), f"NULL {b}": (2, None), "n 6": (3, 6), "n 65537": (3, 65537), "batch 0": (4, 0),
                 "batch -2": (4, -2), "NULL params": (5, None), "NULL subsets": (6, None), "NULL F": (7, None), "NULL inliers": (8, None),
                 "NULL records": (9, None)}
        calls.update({what: (5, p[0]) for what, p in bad_params.items()})
        ok = (fake_ctx, ptr(flow) if flow_form else ptr(src), ptr(coords) if flow_form else ptr(src), n, 1, good, ptr(sub), ptr(Fm), ptr(inl), ptr(rec))
        if dev:
            ok += (ptr(ws), 1 << 30)
            calls.update({"NULL workspace": (10, None), "workspace of 16 bytes": (11, 16), f"{a} is not aligned": (1, off(ok[1], 4)),
                          "subsets is not aligned": (6, off(ptr(sub), 2)), "F is not aligned": (7, off(ptr(Fm), 4)),
                          "records is not aligned": (9, off(ptr(rec), 8)), "workspace is not aligned": (10, off(ptr(ws), 8))})
            if not flow_form:
                calls["dst is not aligned"] = (2, off(ok[2], 4))
        else:
            if flow_form:
                ok += (None,)
            for what, t in {"subsets[1][6] = 9 outside": (2, 3, 4, 5, 6, 7, 9), "subsets[1][0] = -1 outside": (-1, 3, 4, 5, 6, 7, 8),
                            "subsets[1] repeats": (2, 3, 4, 5, 6, 7, 2)}.items():
                tt = sub.copy()
                tt[1] = t
                calls[what] = (6, ptr(tt))
                calls[what + " "] = (6, ptr(tt))               # (keeps tt alive until run() has used it)
        run(name, ok, calls)
    for name in K.EXPORTS[6:]:                                  # the dense pass: ctx, flow, F, threshold, batch, residual, mask, records
        ok = (fake_ctx, ptr(flow), ptr(src), 1.0, 1, ptr(res), ptr(mask), ptr(rec))
        calls = {"NULL context": (0, None), "NULL flow": (1, None), "NULL F": (2, None), "threshold -1": (3, -1.0), "threshold nan": (3, float("nan")),
                 "threshold inf": (3, float("inf")), "batch 0": (4, 0), "NULL records": (7, None)}
        if name.endswith("_dev"):
            calls.update({"flow is not aligned": (1, off(ptr(flow), 2)), "F is not aligned": (2, off(ptr(src), 4)),
                          "residual is not aligned": (5, off(ptr(res), 2)), "records is not aligned": (7, off(ptr(rec), 8))})
        run(name, ok, calls)
    assert lib.mav_find_fundamental_workspace_bytes(6, 1, good) == 0 and b"mav_find_fundamental_workspace_bytes:" in lib.mav_last_error()
    assert lib.mav_find_fundamental_workspace_bytes(8, 0, good) == 0
    assert lib.mav_find_fundamental_workspace_bytes(8, 1, bad_params["flags 0x1"][0]) == 0
    small, large = lib.mav_find_fundamental_workspace_bytes(8, 1, good), lib.mav_find_fundamental_workspace_bytes(1000, 64, good)
    assert 0 < small < large and small % 16 == 0
    for a in (Fm, inl, rec, ws, res, mask):
        assert np.all(a == CANARY)


def test_python_layer_refuses_what_is_not_built(mav):
    import inspect
    import pytest
    from mavflow import fundamental as K
    from mavflow.detector import Detector
    pts = np.zeros((9, 2), np.float32)
    for method in (K.FM_7POINT, K.FM_8POINT, K.FM_LMEDS, 0):
        with pytest.raises(NotImplementedError):
            K.findFundamentalMat(pts, pts, method=method)
    Fm, mask = K.findFundamentalMat(pts[:6], pts[:6])          # n < 7: no GPU is touched
    assert Fm is None and mask.shape == (6, 1) and mask.dtype == np.uint8 and not mask.any()
    sig = inspect.signature(K.findFundamentalMat).parameters
    assert list(sig) == ["points1", "points2", "method", "ransacReprojThreshold", "confidence", "maxIters", "mask", "rng"]
    assert (sig["method"].default, sig["ransacReprojThreshold"].default, sig["confidence"].default, sig["maxIters"].default) == (K.FM_RANSAC, 3.0, 0.99, 1000)
    eps = np.finfo(np.float64).eps
    assert K.repaired(0.999, 1.0) == (0.999, 0.99) and K.repaired(0.0, 0.5) == (3.0, 0.5) and K.repaired(-1.0, 0.0) == (3.0, 0.99)
    assert K.repaired(2.0, 1 - eps) == (2.0, 1 - eps) and K.repaired(2.0, eps) == (2.0, eps) and K.repaired(2.0, eps / 2) == (2.0, 0.99)
    assert np.array_equal(K.scaled(np.full((3, 3), 2.0)), np.ones((3, 3))) and np.array_equal(K.scaled(np.diag([1.0, 1.0, 0.0])), np.diag([1.0, 1.0, 0.0]))
    assert list(inspect.signature(Detector.get_transformation_matrix).parameters) == ["self", "orig_frame", "flow_uv"]
    assert "five-point" in open(os.path.join(ROOT, "DESIGN.md")).read()     # why ESSENTIAL stays out is written down

"""The C boundary of include/mavflow_essential.h: the header declares and the cross-compiled library exports exactly
mavflow.essential.EXPORTS (none of them in another header or in _lib.EXPORTS), a host form and a _dev form of each call, the params'
and the record's size and offsets match the Python mirrors (a small C program compiled against the header, here and now), the Makefile
builds the kernels without FMA contraction, and calls that must be refused from their arguments alone are refused with MAV_ERR_ARG, the
function's name in the message and the outputs untouched -- before the context is looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_essential.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, essential
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_(?:essential|find_essential|flow_essential)[a-z0-9_]*)\s*\(", txt)
    assert sorted(declared) == sorted(essential.EXPORTS) and len(declared) == 6
    lib = essential.load()
    for s in essential.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    assert not any("essential" in s for s in _lib.EXPORTS)
    for s in ("mav_find_essential", "mav_flow_essential"):   # a host form and a _dev form each
        assert s in essential.EXPORTS and s + "_dev" in essential.EXPORTS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other == "mavflow_essential.h":
            continue
        main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not re.search(r"mav_essential_|mav_find_essential|mav_flow_essential", main), other
    for phrase in ('#include "mavflow.h"', "AS REMEMBERED, PINNED TO NO cv2 BUILD", "action-matrix eigen-solver", "SVD null space", "float32 points",
                   "getSubset retry loop", "returned scale and sign", "stacked E matrices", "n == 5", "THE HOST BUILDS need[]",
                   "first of equal\n *   counts wins", "every byte is written", "FULL PIVOTING", "PARTIAL (ROW) PIVOTING", "BISECTION",
                   "A refused call has enqueued and written nothing", "K^-T E K^-1", "best_count = 4"):
        assert phrase in raw, phrase
    for member in ("find_essential", "flow_essential"):
        assert hasattr(_lib.Context, member) and hasattr(_lib.Context, member + "_enqueue"), member
    assert hasattr(_lib.Context, "find_essential_workspace_bytes")
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_essential.o") == 4           # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_essential.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2] and "mavflow_essential.h" in rule.split("\n")[0]
    prereq = [line for line in mk.split("\n") if line.startswith("$(BUILD)/mavflow.o:")][0]
    assert "mavflow_essential.h" in prereq and "mavflow_fundamental.h" in prereq


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, essential as K
    import essential_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    structs = {"mav_essential_params": K.EssentialParams, "mav_essential_record": K.EssentialRecord}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_fundamental.h"', '#include "mavflow_essential.h"', "int main(void) {"]
    for sname, mirror in structs.items():
        lines.append(f'  printf("{sname} %zu\\n", sizeof({sname}));')
        for name, _ in mirror._fields_:
            lines.append(f'  printf("{sname}.{name} %zu\\n", offsetof({sname}, {name}));')
    for macro in ("MAV_ESSENTIAL_MAX_PAIRS", "MAV_ESSENTIAL_MAX_ITERS", "MAV_FUNDAMENTAL_MAX_PAIRS"):
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_essential_params"] == C.sizeof(K.EssentialParams) == 56 and got["mav_essential_record"] == C.sizeof(K.EssentialRecord) == 32
    for sname, mirror in structs.items():
        for name, _ in mirror._fields_:
            assert got[f"{sname}.{name}"] == getattr(mirror, name).offset, (sname, name)
    for name in K.RECORD_DTYPE.names:
        assert got[f"mav_essential_record.{name}"] == K.RECORD_DTYPE.fields[name][1], name
    assert [got[f"mav_essential_record.{n}"] for n in ("ok", "inliers", "best_iter", "best_slot", "iters_run", "valid", "sq_error")] == [0, 4, 8, 12, 16, 20, 24]
    assert K.RECORD_DTYPE == R.RECORD_DTYPE                         # the restatement's record is the library's
    assert got["MAV_ESSENTIAL_MAX_PAIRS"] == got["MAV_FUNDAMENTAL_MAX_PAIRS"] == K.ESSENTIAL_MAX_PAIRS == R.MAX_PAIRS == 65536
    assert got["MAV_ESSENTIAL_MAX_ITERS"] == K.ESSENTIAL_MAX_ITERS == R.MAX_ITERS == 4096
    assert (K.LMEDS, K.RANSAC) == (4, 8)                            # cv2's values
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488           # nothing was added to the loop's struct
    p = K.EssentialParams()
    K.load().mav_essential_defaults(C.byref(p))
    assert (p.threshold, p.confidence, p.fx, p.fy, p.cx, p.cy, p.max_iters, p.flags) == (1.0, 0.999, 1.0, 1.0, 0.0, 0.0, 1000, 0)
    assert (p.fx, p.fy, p.cx, p.cy) == R.CAMERA


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, essential as K
    lib, ptr = K.load(), _lib._ptr
    n, mi = 9, 3
    src = np.arange(2.0 * n + 2)
    flow = np.ones(64, np.float32)
    coords = np.zeros((n, 2), np.int32)
    sub = np.array([[0, 1, 2, 3, 4], [2, 3, 4, 5, 6], [8, 7, 6, 5, 4]], np.int32)
    E, Fm, inl, rec, ws = (np.full(64, CANARY, np.uint64) for _ in range(5))
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    off = lambda v, k: C.c_void_p(v.value + k)

    def params(**kw):
        p = K.essential_params(max_iters=mi)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.cast(C.pointer(p), C.c_void_p), p

    good, keep = params()
    nan, inf = float("nan"), float("inf")
    bad_params = {"threshold -1": params(threshold=-1.0), "threshold nan": params(threshold=nan), "threshold inf": params(threshold=inf),
                  "confidence 0": params(confidence=0.0), "confidence 1": params(confidence=1.0), "confidence nan": params(confidence=nan),
                  "flags 0x1": params(flags=1), "max_iters 0": params(max_iters=0), "max_iters 4097": params(max_iters=4097),
                  "camera fx 0": params(fx=0.0), "camera fx -1": params(fx=-1.0), "camera fx nan": params(fx=nan), "camera fx inf": params(fx=inf),
                  "camera fx 1, fy 0": params(fy=0.0), "camera fx 1, fy -2": params(fy=-2.0), "camera fx 1, fy nan": params(fy=nan),
                  "camera fx 1, fy inf": params(fy=inf), "camera cx nan": params(cx=nan), "camera cx inf": params(cx=inf),
                  "camera cx 0, cy nan": params(cy=nan), "camera cx 0, cy -inf": params(cy=-inf)}

    def run(name, ok, calls):
        fn = getattr(lib, name)
        put = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        for what, (k, v) in calls.items():
            assert fn(*put(k, v)) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)

    for name in K.EXPORTS[2:]:
        dev, flow_form = name.endswith("_dev"), "flow" in name
        a, b = ("flow", "coords") if flow_form else ("src", "dst")
        calls = {"NULL context": (0, None), f"NULL {a}": (1, None), f"NULL {b}": (2, None), "n 4": (3, 4), "n 65537": (3, 65537), "batch 0": (4, 0),
                 "batch -2": (4, -2), "NULL params": (5, None), "NULL subsets": (6, None), "NULL E": (7, None), "NULL F": (8, None),
                 "NULL inliers": (9, None), "NULL records": (10, None)}
        calls.update({what: (5, p[0]) for what, p in bad_params.items()})
        ok = (fake_ctx, ptr(flow) if flow_form else ptr(src), ptr(coords) if flow_form else ptr(src), n, 1, good, ptr(sub), ptr(E), ptr(Fm), ptr(inl),
              ptr(rec))
        if dev:
            ok += (ptr(ws), 1 << 30)
            calls.update({"NULL workspace": (11, None), "workspace of 16 bytes": (12, 16), f"{a} is not aligned": (1, off(ok[1], 4)),
                          "subsets is not aligned": (6, off(ptr(sub), 2)), "E is not aligned": (7, off(ptr(E), 4)), "F is not aligned": (8, off(ptr(Fm), 4)),
                          "records is not aligned": (10, off(ptr(rec), 8)), "workspace is not aligned": (11, off(ptr(ws), 8))})
            if not flow_form:
                calls["dst is not aligned"] = (2, off(ok[2], 4))
        else:
            if flow_form:
                ok += (None,)
            for what, t in {"subsets[1][4] = 9 outside": (2, 3, 4, 5, 9), "subsets[1][0] = -1 outside": (-1, 3, 4, 5, 6), "subsets[1] repeats": (2, 3, 4, 5, 2)}.items():
                tt = sub.copy()
                tt[1] = t
                calls[what] = (6, ptr(tt))
                calls[what + " "] = (6, ptr(tt))               # (keeps tt alive until run() has used it)
        run(name, ok, calls)
    assert lib.mav_find_essential_workspace_bytes(4, 1, good) == 0 and b"mav_find_essential_workspace_bytes:" in lib.mav_last_error()
    assert lib.mav_find_essential_workspace_bytes(8, 0, good) == 0
    assert lib.mav_find_essential_workspace_bytes(8, 1, bad_params["flags 0x1"][0]) == 0
    assert lib.mav_find_essential_workspace_bytes(8, 1, bad_params["camera fx 0"][0]) == 0
    small, large = lib.mav_find_essential_workspace_bytes(5, 1, good), lib.mav_find_essential_workspace_bytes(1000, 64, good)
    assert 0 < small < large and small % 16 == 0
    for a in (E, Fm, inl, rec, ws):
        assert np.all(a == CANARY)

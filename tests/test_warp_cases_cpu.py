"""tests/warp_cases.py held to its own promises without a GPU: the table lists exactly the (coordinate policy x pixel format) instances
csrc/kernels_warp.hip names (read as text: a listed form that no longer exists, or an existing one that is unlisted, fails here), and
every feature an input is noted for is reached -- computed from the restatement's trace."""
import re

import numpy as np
import pytest

import warp_cases as T
import warp_ref as R

BIG = [f for f in T.FRAMES if f[0] * f[1] >= T.FEATURE_FRAME]


def test_the_table_lists_the_instances_the_source_names():
    s = T.source_forms()
    assert s["structs"] == s["dispatched"] == set(T.POLICIES.values())
    assert s["formats"] == s["fmt_structs"] == set(T.FORMATS)
    assert s["method"] == {"CoordAffine", "CoordPerspective"}
    assert len(T.INSTANCES) == len(set(T.INSTANCES)) == len(s["dispatched"]) * len(s["formats"]) == 20
    for name, value in T.FORMATS.items():
        assert re.search(rf"#define MAV_WARP_{name}\s+{value}\b", open(T.KERNELS.replace("mav-detection_amd/csrc/kernels_warp.hip", "include/mavflow_warp.h")).read())
    # one sampling body, no floating-point atomics, the inverse once per workgroup
    assert len(re.findall(r"void warp_sample\(", s["text"])) == 1
    assert not re.search(r"atomicAdd|unsafeAtomic|atomicMax\s*\(\s*\(?\s*(float|double)", s["text"])
    assert s["text"].count("if (threadIdx.x == 0) pol.setup(k, img, lds);") == 2 and s["text"].count("__syncthreads();") == 3
    assert T.FRAMES == [(1, 1), (2, 3), (5, 3), (37, 23), (131, 67)] and T.B == 3
    assert sum(1 for W, H in T.FRAMES if W * H > 256) >= 2                # more than one workgroup


def _traces(policy, W, H, fmt):
    """name -> (the coordinate trace or None, the sampling trace) of every operand of the policy on image item 0"""
    img = T.images(fmt, W, H)[0]
    out = {}
    for name, op, flags in T.operands(policy, W, H):
        tr = []
        T.reference(policy, img, op, flags, tr)
        out[name] = (tr[0] if len(tr) == 2 else None, tr[-1])
    return out


@pytest.mark.parametrize("frame", BIG, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("policy", ["map", "planes", "flow"])
def test_map_inputs_reach_what_they_are_noted_for(policy, frame):
    W, H = frame
    tr = _traces(policy, W, H, R.F32C2)
    c, s = tr["smooth"]
    assert s["inside"].mean() > 0.5 and (~s["inside"]).any() and s["partial"].any()          # mostly inside; wholly outside and clamped taps at the rim
    assert ((s["ax"] != 0) & (s["ay"] != 0) & s["inside"]).any()
    sp = T.special_coords(W, H)
    n0 = W * H
    seen = set()
    for i, (mx, my, note) in enumerate(sp):
        c, s = tr[f"special {i // n0}"]
        at = np.unravel_index(i % n0, (H, W))
        if policy == "flow" and not (np.isfinite(mx) and np.isfinite(my) and abs(mx) < 1e6 and abs(my) < 1e6):
            continue                    # grid - (grid - m) is m only where the subtractions are exact; the flow route's own cases are below
        if policy == "flow":
            assert c["px"][at] == np.float32(mx) * np.float32(32) and c["py"][at] == np.float32(my) * np.float32(32), note
        axis, what = note.split(" ", 1) if note[1] == " " else ("", note)
        q, sq, a, n = (s["qx"], s["sx"], s["ax"], W) if axis == "x" else (s["qy"], s["sy"], s["ay"], H)
        if what == "-1":
            assert sq[at] == -1 and a[at] == 0 and s["inside"][at] and s["partial"][at]
        elif what == "-1/32":
            assert sq[at] == -1 and a[at] == 31 and s["inside"][at]
        elif what == "0":
            assert sq[at] == 0 and a[at] == 0 and s["inside"][at]
        elif what == "n-1":
            assert sq[at] == n - 1 and a[at] == 0 and s["inside"][at] and s["partial"][at]
        elif what == "n-1/32":
            assert sq[at] == n - 1 and a[at] == 31 and s["inside"][at]
        elif what == "n":
            assert sq[at] == n and not s["inside"][at] and s["fits"][at]
        elif what == "tie +":
            assert c["tie_pos"][at] and q[at] % 2 == 0
        elif what == "tie -":
            assert c["tie_neg"][at] and q[at] % 2 == 0
        elif what in ("NaN", "+inf", "-inf", "+3e9", "-3e9"):
            assert not s["fits"][at] and not s["inside"][at]
        elif what == "past int16":
            assert s["fits"][at] and s["int16_clamped"][at] and not s["inside"][at]
        elif note == "NaN tap under zero weight":
            assert s["nan_zero_w"][at], (frame, policy, i)
        seen.add(what if axis else note)
    want = {"-1", "-1/32", "0", "n-1", "n-1/32", "n", "tie +", "tie -", "NaN tap under zero weight"}
    assert want <= seen and (policy == "flow" or {"NaN", "+inf", "-inf", "+3e9", "-3e9", "past int16"} <= seen)


@pytest.mark.parametrize("frame", BIG, ids=lambda f: f"{f[0]}x{f[1]}")
def test_flow_route_reaches_the_non_finite_cases_through_its_own_sum(frame):
    """x + (-u) with u = NaN, +-inf, +-3e9 -- the flow fields made from the special maps carry them (x - NaN, x - inf, ...)"""
    W, H = frame
    tr = _traces("flow", W, H, R.U8C3)
    unfit = sum(int((~s["fits"]).sum()) for _, s in tr.values())
    assert unfit >= 10
    assert any(s["int16_clamped"].any() for _, s in tr.values())
    c, s = tr["noise"]
    assert s["inside"].any() and s["partial"].any()


@pytest.mark.parametrize("frame", BIG, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("policy", ["affine", "perspective"])
def test_matrix_inputs_reach_what_they_are_noted_for(policy, frame):
    W, H = frame
    tr = _traces(policy, W, H, R.F32C1)
    inv = R.INVERSE_MAP
    for fl in (0, inv):
        c, s = tr[f"identity, flags {fl}"]
        assert s["inside"].all() and (s["ax"] == 0).all() and (s["ay"] == 0).all() and s["nan_zero_w"].any()
        assert np.array_equal(s["sx"], np.broadcast_to(np.arange(W), (H, W))) and np.array_equal(s["sy"], np.broadcast_to(np.arange(H)[:, None], (H, W)))
        c, s = tr[f"half pixel, flags {fl}"]
        assert (s["ax"] == 16).all() and (s["ay"] == 16).all()
        c, s = tr[f"shift (1, -1), flags {fl}"]
        assert (~s["inside"]).any() or s["partial"].any()
        c, s = tr[f"rotation with scale, flags {fl}"]
        assert ((s["ax"] != 0) & (s["ay"] != 0) & s["inside"]).any() and (s["partial"].any() or (~s["inside"]).any())
        assert W * H < 256 or (~s["inside"]).any()                                            # a frame with corners to turn out of sight
        c, s = tr[f"reflection, flags {fl}"]
        assert np.array_equal(s["sx"][0], np.arange(W)[::-1])
    assert np.array_equal(tr["half pixel, flags 16"][1]["sx"][0], np.arange(W))               # sampling at x + 0.5
    assert np.array_equal(tr["half pixel, flags 0"][1]["sx"][0], np.arange(W) - 1)           # the inverse: x - 0.5 -> sx = x - 1, ax = 16
    c, s = tr["zero determinant, flags 0"]
    assert (c["m"] == 0).all() and (s["qx"] == 0).all() and (s["qy"] == 0).all()             # the zero matrix samples (0, 0) everywhere
    if policy == "affine":
        assert tr["huge, flags 16"][0]["saturated"] and tr["tiny, flags 0"][0]["saturated"]
        assert not tr["rotation with scale, flags 0"][0]["saturated"]
    else:
        c, s = tr["tilt, W crosses zero, flags 16"]
        assert c["w_pos"] and c["w_neg"] and not c["w_zero"].any()
        c, s = tr["W zero on a pixel, flags 16"]
        assert c["w_zero"][:, W // 2].all() and c["w_pos"] and c["w_neg"]
        assert (s["qx"][:, W // 2] == 0).all() and s["fits"][:, W // 2].all()                # W = 0 -> 0: the formulas, not a division by zero
        for fl in (0, inv):
            c, s = tr[f"zero matrix, flags {fl}"]
            assert c["w_zero"].all() and (s["qx"] == 0).all() and s["inside"].all()
        assert tr["huge, flags 16"][0]["clamped"]                                             # fX past int32: clamped, not wrapped


def test_every_instance_has_inputs_at_every_frame_and_the_batches_differ():
    for W, H in T.FRAMES:
        for policy, fmt in T.INSTANCES:
            ops = T.operands(policy, W, H)
            assert len(ops) >= 2 and len({n for n, _, _ in ops}) == len(ops)
            img = T.images(T.FORMATS[fmt], W, H)
            assert img.shape[0] == T.B and img.dtype == R.FORMATS[T.FORMATS[fmt]][0]
            if W * H > 1:
                assert not np.array_equal(img[1], img[2])
            for g in T.groups(ops):
                assert len(g) == T.B
        for policy in ("affine", "perspective"):
            ms = T.matrices(policy, W, H)
            assert any(T.host_refuses(m.M, 0) for m in ms) and not T.host_refuses(ms[0].M, 0)
            assert any(T.host_refuses(m.M, 0) and not T.host_refuses(m.M, R.INVERSE_MAP) for m in ms)


def test_uint8_images_are_checkerboards_and_noise():
    for fmt in (R.U8C1, R.U8C3):
        a = T.images(fmt, 37, 23)
        assert set(np.unique(a[0])) == {0, 255} and a[0].reshape(23, 37, -1)[0, 0, 0] != a[0].reshape(23, 37, -1)[0, 1, 0]
        assert len(np.unique(a[1])) > 100
    f = T.images(R.F32C2, 37, 23)
    assert np.isnan(f[0]).sum() == 1 and np.isnan(f[0][T.nan_pixel(37, 23)][0]) and not np.isnan(f[1:]).any()


@pytest.mark.parametrize("frame", BIG, ids=lambda f: f"{f[0]}x{f[1]}")
def test_warp_method_fields_reach_the_mask_and_the_tie(frame):
    W, H = frame
    flow = T.method_flow(W, H)
    for kind in (R.AFFINE, R.PERSPECTIVE):
        ms = T.method_matrices(kind, W, H)
        assert len(ms) >= 6
        ident = [m for m in ms if m.name == "identity"][0]
        diff, mag, rec = R.warp_method(flow[1], ident.M, kind)
        assert (diff == 0).all() and rec["max_mag"] == 0 and (rec["row"], rec["col"]) == (0, 0)   # every byte of the record from an all-zero image
        rot = [m for m in ms if m.name == "rotation with scale"][0]
        stable = (R.warp_affine if kind == R.AFFINE else R.warp_perspective)(flow[1], rot.M, 0)
        assert (W * H < 256 or ((stable == 0) & (flow[1] != 0)).any()) and (stable != 0).any()               # the mask changes elements, element-wise
        diff, mag, rec = R.warp_method(flow[1], rot.M, kind)
        assert rec["max_mag"] == mag.max() > 0 and mag[rec["row"], rec["col"]] == mag.max()
        half = [m for m in ms if m.name == "shift (1, -1)"][0]
        diff, mag, rec = R.warp_method(flow[2], half.M, kind)
        assert (mag == mag.max()).sum() >= 1
    # the first raster position wins among equals
    f = np.zeros((H, W, 2), np.float32)
    f[H - 1, W - 2] = f[0, 0] = (3.0, 4.0)                               # both land inside, one pixel to the right
    diff, mag, rec = R.warp_method(f, [[1, 0, 1], [0, 1, 0]], R.AFFINE)
    assert (mag == mag.max()).sum() >= 2 and (rec["row"], rec["col"]) == tuple(np.argwhere(mag == mag.max())[0])


# ---- past the caps: the second trip of the grid-stride loops ---------------------------------------------------------------------------------
def test_the_cap_frames_sit_just_past_the_caps_the_source_defines():
    c = T.source_caps()
    wg = c["WARP_WG"]
    for name, frame, cap in (("CAP_FRAME", T.CAP_FRAME, c["WARP_CAP"]), ("METHOD_CAP_FRAME", T.METHOD_CAP_FRAME, c["WARP_METHOD_CAP"])):
        n0 = frame[0] * frame[1]
        assert 0 < n0 - cap * wg <= 2 * wg, (name, frame, "is not within two workgroups past cap * WG =", cap * wg)
        assert ">1:partial-last" in T.stride_forms(n0, cap, wg), (name, "does not reach the form >1:partial-last")
        assert frame[0] % 2 and frame[1] % 2 and frame not in T.FRAMES
    # the launches read as text: the caps are the ones warp_grid is given
    s = T.source_forms()["text"]
    assert re.search(r"warp_grid\(int W, int H, int B, size_t cap = WARP_CAP\)", s) and len(re.findall(r"warp_grid\(W, H, B, WARP_METHOD_CAP\)", s)) == 2
    assert len(re.findall(r"p \+= \(size_t\)gridDim\.x \* WARP_WG", s)) == 2
    # with the two frames removed no case reaches a second trip, under either cap
    for W, H in T.FRAMES:
        assert T.stride_forms(W * H, c["WARP_CAP"], wg) == T.stride_forms(W * H, c["WARP_METHOD_CAP"], wg) == {"1"}, ("a frame of FRAMES reaches >1", W, H)
    assert T.stride_forms(cap * wg, cap, wg) == {"1"} and T.stride_forms(2 * cap * wg, cap, wg) == {">1"}
    assert T.stride_forms(cap * wg + 1, cap, wg) == {">1", ">1:partial-last"} and T.stride_forms(0, cap, wg) == {"1"}


def _weighted_inside_tap(s):
    """per pixel: some tap lies inside the image under a nonzero weight (the restatement's trace)"""
    W, H, ax, ay = s["W"], s["H"], s["ax"], s["ay"]
    out = np.zeros(s["inside"].shape, bool)
    for dy, wy in ((0, 32 - ay), (1, ay)):
        for dx, wx in ((0, 32 - ax), (1, ax)):
            r, c = s["sy"] + dy, s["sx"] + dx
            out |= s["inside"] & (r >= 0) & (r < H) & (c >= 0) & (c < W) & (wy * wx != 0)
    return out


@pytest.mark.parametrize("policy,fmt", T.INSTANCES, ids=lambda v: str(v))
def test_every_instance_samples_the_image_past_the_cap(policy, fmt):
    """at least half of the pixels past cap * WG have an inside tap under a nonzero weight: per item, but for "rotation with scale"
    at flags 0 -- the operand the affine instances are to run -- which turns four fifths of the last row out of sight (0.198 inside);
    for that call the share is counted over its two items, the second of which keeps every pixel in"""
    c = T.source_caps()
    thr = c["WARP_CAP"] * c["WARP_WG"]
    W, H = T.CAP_FRAME
    names, src, ops, fl, want, traces = T.cap_reference(policy, fmt)
    assert len(names) == T.CAP_B == 2 and src.shape[0] == ops.shape[0] == want.shape[0] == 2 and not np.array_equal(ops[0], ops[1]) and not np.array_equal(src[0], src[1])
    tail = np.concatenate([_weighted_inside_tap(s).ravel()[thr:] for s in traces])
    assert len(tail) == 2 * (W * H - thr) > 0 and tail.mean() >= 0.5, (policy, fmt, tail.mean())
    for b in range(2):
        region = want[b].reshape(W * H, -1)[thr:]
        share = _weighted_inside_tap(traces[b]).ravel()[thr:].mean()
        assert share >= 0.5 or (names[b] == "rotation with scale" and share >= 0.15), (policy, fmt, names[b], share)
        assert len(np.unique(R.bits(region) if region.dtype == np.float32 else region)) > 2, (policy, fmt, b)
    if policy in ("map", "planes", "flow"):
        # every special coordinate lands on the second trip as well as the first
        sp = T.special_coords(W, H)
        assert W * H - len(sp) >= thr
        s = traces[0]
        last = lambda k: s[k].ravel()[W * H - len(sp):]
        assert np.array_equal(last("qx"), s["qx"].ravel()[:len(sp)]) and np.array_equal(last("fits"), s["fits"].ravel()[:len(sp)])
        notes = [n.split(" ", 1)[1] for _, _, n in sp]
        for what in ("NaN", "+inf", "-inf", "+3e9", "-3e9"):
            assert not any(last("fits")[i] for i, n in enumerate(notes) if n == what), what
        assert all(last("fits")[i] and last("int16_clamped")[i] and not last("inside")[i] for i, n in enumerate(notes) if n == "past int16")
        assert any(last("fits")[i] and not last("inside")[i] for i, n in enumerate(notes) if n == "n")                        # the outside cases
        assert any(last("inside")[i] and last("partial")[i] for i, n in enumerate(notes) if n in ("-1", "n-1"))
    else:
        assert fl == 0 and names[0] in ("rotation with scale", "mild tilt") and names[1] in ("half pixel", "tilt, W crosses zero")


def test_warp_method_references_past_the_cap():
    c = T.source_caps()
    thr = c["WARP_METHOD_CAP"] * c["WARP_WG"]
    W, H = T.METHOD_CAP_FRAME
    for kind in (R.AFFINE, R.PERSPECTIVE):
        calls = T.method_cap_reference(kind)
        recs = [(n, r) for names, f, M, d, m, rec in calls for n, r in zip(names, rec)]
        assert any(int(r["row"]) * W + int(r["col"]) >= thr for _, r in recs[:-T.B])                     # among method_matrices over method_flow
        ident = [r for n, r in recs if n == "identity"]
        assert ident and all(r.tobytes() == np.zeros((), R.RECORD_DTYPE).tobytes() for r in ident)      # every pixel ties at +0.0 across both trips: the first
        names, f, M, d, mag, rec = calls[-1]
        assert names == ("tie", "the later is larger", "the earlier is larger")
        at = np.flatnonzero(mag[0].ravel() == mag[0].max())
        assert len(at) == 2 and at[0] < thr <= at[1] and at[0] // c["WARP_WG"] % c["WARP_METHOD_CAP"] != at[1] // c["WARP_WG"] % c["WARP_METHOD_CAP"]
        assert R.bits(mag[0].ravel()[at[0]]) == R.bits(mag[0].ravel()[at[1]]) and mag[0].max() == 5
        assert (int(rec[0]["row"]), int(rec[0]["col"])) == divmod(int(at[0]), W) and rec[0]["max_mag"] == 5
        assert (int(rec[1]["row"]), int(rec[1]["col"])) == divmod(int(at[1]), W) and rec[1]["max_mag"] == 10
        assert (int(rec[2]["row"]), int(rec[2]["col"])) == divmod(int(at[0]), W) and rec[2]["max_mag"] == 10
        for y, x in T.method_cap_plants(W, H, thr):
            assert 0 < y < H - 1 and 0 < x < W - 1 and y == H - 2                                        # sources off the rim, landing in the last row

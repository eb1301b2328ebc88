"""The flow-history case table (tests/history_cases.py) is what it claims to be -- checked from the predicates and the numpy
restatement alone, without a GPU: every form is reached by a case, every case reaches what it names (the element forms read from
history_ref's trace of the case's own inputs), the thresholds of the grid-stride loops are where the table says, and the planted
fields send their pixels where the table takes them to go."""
import os
import re

import numpy as np
import pytest

import history_cases as hc
import history_ref as R

# Every entry of CASES by name: a case taken out of the table has to be taken out here too, and then test_every_form_is_reached says
# what it was the only one to reach.
NAMES = [f"planted37x23_{i}to{r}_{a}_{o}" for r, i, a, o in hc.INSTANCES] + [
    "tiny1x1_L3", "tiny7x1", "tiny1x7_xy", "tiny5x3_f64", "tiny6x2_flow", "smooth41x29_L5", "count3_37x23", "count2_37x23_f64_flow",
    "count11_smooth16x16_L5", "dev37x23_aligned", "dev37x23_flow+4B", "dev37x23_out+8B", "dev37x23_flowform_out+4B",
    "dev37x23_f64_flow+8B_out+8B", "dev37x23_f32tof64_flow+4B", "cap1025x1025_L3"]


def _reached(cases):
    reached = {g: set() for g in hc.FORMS}
    for c in cases:
        for g, f in hc.case_forms(c):
            reached[g].add(f)
    return reached


def test_every_form_is_reached():
    assert [c.name for c in hc.CASES] == NAMES and len(hc.INSTANCES) == 12
    for c in hc.CASES:
        names = {f"{g}={f}" for g, f in hc.case_forms(c)}
        assert c.expects and c.expects <= names, (c.name, sorted(c.expects - names))
        assert c.n_pushes >= 2 * c.L + 1 or c.name == hc.LARGE, c.name
    reached = _reached(hc.CASES)
    for g, forms in hc.FORMS.items():
        assert reached[g] <= forms, (g, sorted(reached[g] - forms))                 # a predicate invented a form FORMS does not name
        assert forms <= reached[g], (g, sorted(forms - reached[g]))


def test_the_table_needs_its_cases():
    def missing(keep):
        reached = _reached([c for c in hc.CASES if keep(c)])
        return {f"{g}={f}" for g, forms in hc.FORMS.items() for f in forms - reached[g]}
    assert missing(lambda c: c.name != hc.LARGE) == {"trace.stride=>1", "trace.stride=>1:partial-last", "put.stride=>1"}
    assert [c.name for c in hc.CASES if c.n0 > 10 ** 4] == [hc.LARGE]                # the only large case
    assert {"frame=1x1", "frame=1xN", "frame=Nx1", "frame=few-pixels"} <= missing(lambda c: not c.name.startswith("tiny") and "16x16" not in c.name)
    assert {f"ptr={f}" for f in hc.FORMS["ptr"] - {"staged"}} | {"put.access=scalar", "out.access=scalar"} == missing(lambda c: c.entry == "host")
    assert {"count=>1", "count=>1:short-last-call"} <= missing(lambda c: c.count == 1)
    assert {"coord=" + f for f in ("nan", "+inf", "-inf", "past-int32", "beyond+32768", "beyond-32768", "nan-tap-zero-weight")} <= \
        missing(lambda c: c.kind != "planted")
    assert "axes=xy" in missing(lambda c: c.axes == "reference") and "out=flow" in missing(lambda c: c.out == "reference")
    assert {"ring=f64", "input=f32->f64", "input=f64->f64"} <= missing(lambda c: c.ring == "f32")


def test_thresholds_of_the_grid_stride_loops():
    """The arithmetic of history_blocks() and of the loops, spelled out: a changed constant in kernels_history.hip must change these."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "mav-detection_amd", "csrc", "kernels_history.hip")).read()
    for name, v in (("HIST_WG", hc.WG), ("HIST_PX", hc.PX), ("HIST_CAP", hc.CAP)):
        assert re.search(rf"#define {name} {v}\b", src), name
    assert hc.second_iteration_pixel() == 4096 * 256 * 1 == 1_048_576
    assert [hc.history_blocks(n) for n in (0, 1, 256, 257, 4095 * 256, 4095 * 256 + 1, 10 ** 7)] == [1, 1, 1, 2, 4095, 4096, 4096]
    for W, H, forms in ((37, 23, {"1"}), (1024, 512, {"1"}), (1024, 1024, {"1"}), (1280, 720, {"1"}), (1025, 1025, {">1", ">1:partial-last"}),
                        (2048, 1024, {">1"}), (1920, 1080, {">1", ">1:partial-last"})):
        assert hc.stride_forms(hc.trace_items(W * H)) == forms == hc.stride_forms(W * H), (W, H)     # one pixel per thread: the ring write's grid too
    c = hc.BY_NAME[hc.LARGE]
    assert hc.trace_items(c.n0) - 4096 * 256 == 2049 and c.L == 3 and c.n_pushes == 3
    assert 1025 == min(s for s in range(3, 1500, 2) if s * s > hc.second_iteration_pixel())
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mavflow.h")).read()
    assert f"#define MAV_HISTORY_MAX_LENGTH {hc.MAX_LENGTH}\n" in hdr


def test_access_predicates():
    assert hc.put_vec(4, 0) and hc.put_vec(4, 8) and not hc.put_vec(4, 4) and hc.put_vec(8, 16) and not hc.put_vec(8, 8)
    assert hc.out_vec(8, 0) and not hc.out_vec(8, 8) and hc.out_vec(4, 8) and not hc.out_vec(4, 4)
    for c in hc.CASES:                                   # an offset keeps the element's own alignment: the library refuses less
        assert c.flow_off % hc.ELEM[c.inp] == 0 and c.out_off % hc.OUT_ELEM[c.out] == 0, c.name
        assert (c.entry == "dev") or (c.flow_off == 0 and c.out_off == 0), c.name


@pytest.mark.parametrize("axes", ["reference", "xy"])
def test_planted_pixels_go_where_the_table_sends_them(axes):
    """Read at its own integer positions (weights 1, 0, 0, 0) a planted field moves the k-th planted pixel exactly to targets[k]: the
    second step of the push that reads it first samples there.  Checked with the restatement on a zero field as the second one."""
    W, H = 37, 23
    f = hc.planted(W, H, axes)
    yy, xx = np.mgrid[0:H, 0:W]
    step = R.remap_linear_ref(f, xx.astype(np.float32), yy.astype(np.float32))
    if axes == "xy":
        step = step[..., ::-1]
    t, k = hc.targets(W, H), 0
    assert (W + 1) // 2 * ((H + 1) // 2) >= len(t)                                  # every target is planted at least once
    for y in range(0, H, 2):
        for x in range(0, W, 2):
            tx, ty = t[k % len(t)]
            k += 1
            with np.errstate(all="ignore"):
                r, c = np.float32(y + step[y, x, 0]), np.float32(x + step[y, x, 1])
            for got, want in ((r, ty), (c, tx)):
                assert (np.isnan(got) and np.isnan(want)) or got == np.float32(want), (x, y, got, want)
    # ties: odd multiples of 1/64 give a product with fraction one half, rounded to the even neighbour -- both ways
    q = np.rint(np.array([1 / 64, 3 / 64, -1 / 64, -3 / 64], np.float32) * np.float32(32))
    assert q.tolist() == [0.0, 2.0, -0.0, -2.0]


def test_reference_outputs_are_shared_and_read_only():
    a, _ = hc.reference("tiny5x3_f64")
    b, _ = hc.reference("tiny5x3_f64")
    assert a is b and not a.flags.writeable and a.shape == (9, 3, 5, 2) and a.dtype == np.float64
    assert hc.reference("tiny6x2_flow")[0].dtype == np.float32


def test_host_and_device_cases_share_their_reference():
    """The caller's-pointer cases push the fields of the staged case with the same policies: tests/test_gpu_history.py holds both entry
    points to these bytes, so it holds them to each other."""
    host = hc.reference("planted37x23_f32tof32_reference_reference")[0]
    for name in ("dev37x23_aligned", "dev37x23_flow+4B", "dev37x23_out+8B", "count3_37x23"):
        assert np.array_equal(R.bits(hc.reference(name)[0]), R.bits(host)), name
    assert np.array_equal(R.bits(hc.reference("dev37x23_f64_flow+8B_out+8B")[0]), R.bits(hc.reference("planted37x23_f64tof64_reference_reference")[0]))
    assert np.array_equal(R.bits(hc.reference("dev37x23_flowform_out+4B")[0]), R.bits(hc.reference("planted37x23_f32tof32_xy_flow")[0]))

"""mav_radial_error_hist on the device (csrc/kernels_truth.hip: k_radial_hist, both counter forms) held to tests/truth_ref.py by
equality on every case of tests/truth_cases.py -- fields in which no pixel lies near a bin edge (tests/test_truth_cases_cpu.py), since
the device's atan2f is not glibc's -- and on the fields of tests/golden/truth.npz against numpy.histogram2d of what the reference saved."""
import os

import numpy as np
import pytest

import truth_cases as T
import truth_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truth.npz")


def _equal(got, want, what):
    assert got["counts"].dtype == np.int64 and got["counts"].shape == want["counts"].shape, what
    assert (got["non_sky"], got["in_range"]) == (want["non_sky"], want["in_range"]), (what, got["non_sky"], got["in_range"], want["non_sky"], want["in_range"])
    if not np.array_equal(got["counts"], want["counts"]):
        bad = np.argwhere(got["counts"] != want["counts"])
        raise AssertionError((what, len(bad), "cells differ; first", bad[0].tolist(), int(got["counts"][tuple(bad[0])]), int(want["counts"][tuple(bad[0])])))


def _host(ctx, x, **kw):
    return ctx.radial_error_hist(x["flow"], x["gt"], x["sky"], mag_edges=x["mag_edges"], err_edges=x["err_edges"], **kw)


@pytest.mark.parametrize("name", [c.name for c in T.HIST_CASES])
def test_table_equals_the_restatement(name):
    from mavflow import _lib
    c = {k.name: k for k in T.HIST_CASES}[name]
    x = T.hist_inputs(name)
    with _lib.Context(c.W, c.H, c.B) as ctx:
        host = _host(ctx, x)
        _equal(host, x["ref"], (name, "host form"))
        acc = ctx.radial_error_accumulator(x["mag_edges"], x["err_edges"])
        try:
            acc.add(x["flow"], x["gt"], x["sky"])                          # the device form on staged copies
            _equal(acc.counts(), x["ref"], (name, "device form"))
            acc.add(x["flow"], x["gt"], x["sky"])                          # accumulates: twice the table
            twice = acc.counts()
            assert np.array_equal(twice["counts"], 2 * x["ref"]["counts"]) and twice["non_sky"] == 2 * x["ref"]["non_sky"]
            acc.reset()
            assert not acc.counts()["counts"].any() and acc.counts()["non_sky"] == 0
        finally:
            acc.close()
        if c.field == "one cell":
            cell = np.argwhere(host["counts"])
            assert len(cell) == 1 and host["counts"][tuple(cell[0])] == host["non_sky"] == host["in_range"] > 0


def test_two_calls_accumulate_to_the_sum_of_their_tables():
    from mavflow import _lib, _truth
    a = T.hist_inputs("97x71")                                             # two different fields of one size, the default bins
    flow, gt, sky = T.scene(4242, 97, 71, 1, *T.DEFAULT_EDGES)
    b = dict(flow=flow, gt=gt, sky=sky.astype(np.uint8))
    dm, de = R.edge_distance(flow, gt, sky)
    assert dm >= T.MIN_EDGE_DISTANCE_PX and de >= T.MIN_EDGE_DISTANCE_DEG
    with _lib.Context(97, 71, 1) as ctx:
        ta = ctx.radial_error_hist(a["flow"], a["gt"], a["sky"])
        tb = ctx.radial_error_hist(b["flow"], b["gt"], b["sky"])
        _equal(tb, R.radial_hist(b["flow"], b["gt"], b["sky"]), "second field, default bins")
        # the host form adds into the caller's table
        lib, ptr = _truth.load(), _lib._ptr
        em, ee = _truth.DEFAULT_MAG_EDGES, _truth.DEFAULT_ERR_EDGES
        table = np.zeros(_truth.table_words(159, 159), np.int64)
        for x in (a, b):
            _lib.check(lib.mav_radial_error_hist(ctx.h, ptr(x["flow"]), ptr(x["gt"]), ptr(x["sky"]), 1, ptr(em), em.size, ptr(ee), ee.size, ptr(table)))
        assert np.array_equal(table, R.table_of(ta) + R.table_of(tb))
        acc = ctx.radial_error_accumulator()
        try:
            acc.add(a["flow"][0], a["gt"][0], a["sky"][0])
            acc.add(b["flow"], b["gt"], b["sky"])
            assert np.array_equal(R.table_of(acc.counts()), table) and acc.frames == 2
        finally:
            acc.close()


def test_sky_all_sky_adds_nothing_and_null_sky_is_no_sky():
    from mavflow import _lib
    x = T.hist_inputs("97x71")
    with _lib.Context(97, 71, 1) as ctx:
        none = ctx.radial_error_hist(x["flow"], x["gt"], np.full((1, 71, 97), 255, np.uint8))
        assert none["non_sky"] == none["in_range"] == 0 and not none["counts"].any()
        null, zero = ctx.radial_error_hist(x["flow"], x["gt"], None), ctx.radial_error_hist(x["flow"], x["gt"], np.zeros((1, 71, 97), np.uint8))
        _equal(null, zero, "sky = NULL against an all-zero sky")
        _equal(null, R.radial_hist(x["flow"], x["gt"], None), "no sky")
        assert null["non_sky"] == 97 * 71


def test_special_values_fall_in_no_cell():
    from mavflow import _lib
    flow = np.array([[[np.nan, 1.0], [np.inf, 0.0], [0.0, 0.0], [10.0, 0.0], [3.0, 4.0]]], np.float32)       # NaN, inf, zero, the last edge, 5
    gt = np.array([[[1.0, 0.0], [1.0, 0.0], [0.0, 0.0], [2.0, 0.0], [6.0, 8.0]]], np.float32)
    with _lib.Context(5, 1, 1) as ctx:
        got = ctx.radial_error_hist(flow, gt, None)
    want = R.radial_hist(flow, gt, None)
    _equal(got, want, "special values")
    # zero flow: magnitude 0 is the first edge (bin 0), atan2(0, 0) - atan2(0, 0) = 0; magnitude 10 is the last edge: the last bin, closed
    assert want["in_range"] == 3 and want["counts"][0].sum() == 1 and want["counts"][158].sum() == 1


def test_reference_fields_give_histogram2d_of_what_it_saved():
    from mavflow import _lib
    g = np.load(GOLDEN, allow_pickle=False)
    for name in g["hist_cases"]:
        flow, gt, sky = g[f"{name}_flow"], g[f"{name}_gt"], g[f"{name}_sky"]
        dm, de = R.edge_distance(flow, gt, sky)
        assert dm >= T.MIN_EDGE_DISTANCE_PX and de >= T.MIN_EDGE_DISTANCE_DEG
        H, W = sky.shape
        with _lib.Context(W, H, 1) as ctx:
            got = ctx.radial_error_hist(flow, gt, sky)
        assert np.array_equal(got["counts"], g[f"{name}_counts"]) and got["non_sky"] == int((~sky).sum()), name


def test_refusals_with_a_context():
    from mavflow import _lib
    x = T.hist_inputs("5x3")
    with _lib.Context(5, 3, 1) as ctx:
        with pytest.raises(ValueError, match="mav_radial_error_hist: batch 2"):
            ctx.radial_error_hist(np.concatenate([x["flow"]] * 2), np.concatenate([x["gt"]] * 2), None)
        with pytest.raises(ValueError, match="strictly increasing"):
            ctx.radial_error_hist(x["flow"], x["gt"], None, mag_edges=[0.0, 2.0, 1.0])
        with pytest.raises(ValueError):
            ctx.radial_error_accumulator(np.linspace(0, 1, 258))
        _equal(_host(ctx, x), x["ref"], "after the refusals")


def test_edge_lists_may_change_from_call_to_call():
    """the context sends a call's edge lists to the device only when they differ from the last call's: alternate two sets and repeat one"""
    from mavflow import _lib
    a, b = T.hist_inputs("97x71"), T.hist_inputs("3 edges")
    with _lib.Context(97, 71, 1) as ctx:
        for x, what in ((a, "default"), (b, "3 edges"), (b, "3 edges again"), (a, "default again"), (a, "default a third time")):
            _equal(_host(ctx, x), x["ref"], what)
        # same lengths, other values: the comparison is of the values
        em = x["mag_edges"] * 1.0
        em[40] += 0.01
        dm, _ = R.edge_distance(a["flow"], a["gt"], a["sky"], em, a["err_edges"])
        assert dm >= T.MIN_EDGE_DISTANCE_PX
        _equal(ctx.radial_error_hist(a["flow"], a["gt"], a["sky"], mag_edges=em), R.radial_hist(a["flow"], a["gt"], a["sky"], em), "one edge moved")

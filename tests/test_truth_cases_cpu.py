"""tests/truth_cases.py held to its own rules without a GPU: every histogram field keeps every non-sky pixel away from every bin edge
(the GPU tests demand equality although the device's atan2f is not glibc's), has most pixels in range, some out on each side and some
wrapped; every dispatch form of the two launchers is reached; the launchers' constants are the source's."""
import numpy as np
import pytest

import truth_cases as T
import truth_ref as R


def test_constants_are_the_sources():
    got = T.internal_constants()
    assert got == {"MAV_GT_FLOW_GRID_CAP": T.GT_FLOW_GRID_CAP, "MAV_RADIAL_LDS_CELLS": T.RADIAL_LDS_CELLS, "MAV_RADIAL_GRID_CAP": T.RADIAL_GRID_CAP}
    src = open(T.INTERNAL.replace("mavflow_internal.h", "kernels_truth.hip")).read()
    assert "(npx + 255) / 256" in src and "dim3(256)" in src and "(npx + 2047) / 2048" in src and "dim3(1024)" in src


def test_every_dispatch_form_is_reached():
    reached = set().union(*(c.forms() for c in T.GT_CASES))
    assert reached == T.GT_FORMS, T.GT_FORMS ^ reached
    reached = set().union(*(c.forms() for c in T.HIST_CASES))
    assert reached == T.HIST_FORMS, T.HIST_FORMS ^ reached
    # the shapes the GPU tests are asked to run
    assert {(c.W, c.H) for c in T.GT_CASES} >= {(1, 1), (5, 3), (97, 71), (516, 37)} and {(c.W, c.H) for c in T.HIST_CASES} >= {(1, 1), (5, 3), (97, 71), (516, 37)}
    cap = {c.name: c for c in T.GT_CASES}["past the grid cap"]
    assert 0 < cap.npx - T.GT_FLOW_GRID_CAP * T.GT_FLOW_BLOCK <= T.GT_FLOW_BLOCK              # exactly one workgroup's worth past it
    cap = {c.name: c for c in T.HIST_CASES}["past the grid cap"]
    assert 0 < cap.npx - cap.grid() * T.RADIAL_STEP <= T.RADIAL_STEP and cap.B == 3
    b3 = {c.name: c for c in T.GT_CASES}["batch 3"]
    x = T.gt_inputs("batch 3")
    assert b3.B == 3 and len({x["vp1"][b].tobytes() for b in range(3)}) == 3 and len({x["disp"][b].tobytes() for b in range(3)}) == 3
    one = {c.name: c for c in T.HIST_CASES}["516x37 one cell"]
    assert (one.W, one.H, one.B) == (516, 37, 3)


@pytest.mark.parametrize("name", [c.name for c in T.HIST_CASES])
def test_histogram_fields_stay_clear_of_the_edges(name):
    c = {k.name: k for k in T.HIST_CASES}[name]
    x = T.hist_inputs(name)
    dm, de = R.edge_distance(x["flow"], x["gt"], x["sky"], x["mag_edges"], x["err_edges"])
    print(f"{name}: nearest magnitude edge {dm:.3g} px, nearest error edge {de:.3g} deg")
    assert dm >= T.MIN_EDGE_DISTANCE_PX and de >= T.MIN_EDGE_DISTANCE_DEG
    ref = x["ref"]
    assert ref["counts"].sum() == ref["in_range"] <= ref["non_sky"] <= c.B * c.npx
    if c.field == "one cell":
        assert ref["in_range"] == ref["non_sky"] and np.count_nonzero(ref["counts"]) == 1
        return
    assert 2 * ref["in_range"] >= ref["non_sky"]
    if c.npx >= 1000:
        mag, err = R.radial_values(x["flow"], x["gt"], x["sky"])
        em, ee = x["mag_edges"], x["err_edges"]
        assert (mag > em[-1]).any() and (err > ee[-1]).any() and (err < ee[0]).any() and (np.abs(err) > 180).any()
        assert (mag < em[0]).any() == (em[0] > 0)
        assert np.count_nonzero(ref["counts"]) > min(ref["counts"].size, ref["in_range"]) // 4      # spread over the cells, not piled up


def test_one_cell_values_sit_inside_a_bin_of_every_edge_set():
    f, g = np.array(T.ONE_CELL_FLOW, np.float32), np.array(T.ONE_CELL_GT, np.float32)
    for name, (em, ee) in T.EDGE_SETS.items():
        dm, de = R.edge_distance(f[None, None], g[None, None], None, em, ee)
        assert dm > 5e-3 and de > 5e-2, name

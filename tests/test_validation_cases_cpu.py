"""tests/validation_cases.py held to its own rules without a GPU: every case reaches what it is there for (computed from its inputs),
the table as a whole reaches every shape, phase edge and call form, and the launch arithmetic it assumes is the source's."""
import numpy as np
import pytest

import validation_cases as T
import validation_ref as R


def test_constants_are_the_sources():
    assert T.internal_constants() == {"MAV_GT_STATS_GRID_CAP": T.GRID_CAP}
    src = open(T.KERNELS).read()
    assert "(npx + 255) / 256" in src and "blockIdx.x * 4 + wv" in src and "x += 64" in src and "xb += 64" in src and "(k.H + 3) / 4" in src
    assert T.BLOCK == 256 and T.ROWS_PER_BLOCK == 4 and T.CHUNK == 64
    assert f"#define GTS_SUM_STEP {T.SUM_STEP}\n" in src and "dim3(GTS_SUM_STEP)" in src


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_reaches_what_it_is_there_for(name):
    c = T.CASES[name]
    got = T.reaches(name)
    assert c.wants and set(c.wants) <= got, (name, set(c.wants) - got)
    rec, idx = T.inputs(name)["ref"]
    assert rec.dtype == R.RECORD_DTYPE and rec.shape == (c.B,) and idx.shape == (c.B, c.max_pixels)
    assert (rec["listed"] == np.minimum(rec["drone_pixels"], c.max_pixels)).all() and not rec["pad"].any()


def test_the_table_reaches_every_phase_and_form():
    reached = set().union(*(T.reaches(n) for n in T.CASES))
    assert T.REQUIRED <= reached, T.REQUIRED - reached
    cap = T.CASES["past the grid cap"]
    assert 0 < cap.npx - T.GRID_CAP * T.BLOCK <= 8 * T.BLOCK
    b3 = T.inputs("batch 3")
    assert len({b3["seg"][b].tobytes() for b in range(3)}) == 3 and len({b3["omega"][b].tobytes() for b in range(3)}) == 3
    assert [int(v) for v in T.inputs("batch 3 at the cap")["ref"][0]["drone_pixels"]] == [7, 8, 9]


def test_inputs_are_deterministic_and_read_only():
    a = T.inputs("97x71")
    T.inputs.cache_clear()
    b = T.inputs("97x71")
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("seg", "gt_flow", "sky", "depth", "omega", "dt", "flags"))
    assert a["ref"][0].tobytes() == b["ref"][0].tobytes()
    with pytest.raises(ValueError):
        b["seg"][0, 0, 0] = 1

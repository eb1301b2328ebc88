"""The host scheduler's launch sequence, pinned: for every case of tests/schedule_pin_cases.py the `mav_schedule_info` string (byte
for byte) and the (kernel class, stream) of every launch of one `farneback` call in host enqueue order must equal
tests/golden/schedule_pin.json.  Bit-identical flow (tests/test_gpu_flow.py) cannot see a launch that moved to the other stream or
changed places with a neighbour; this can.  What it cannot see: which M slot a launch uses, and a band launch's tile-row range.
tests/test_gpu_schedule_forms.py covers both: the tile-row ranges at every band edge of tests/schedule_cases.py, the M slots under
buffers another picture has dirtied.

The fixture is a recording (tools/gen_schedule_pin.py).  A change that alters the schedule ON PURPOSE regenerates it with that tool and
says so; any other difference is a regression.  Timestamps are not compared."""
import json
import os

import pytest

import schedule_pin_cases as pin

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_pin.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_holds_exactly_the_cases(recorded):
    assert sorted(recorded) == sorted(pin.NAMES)


@pytest.mark.parametrize("case", pin.CASES, ids=pin.NAMES)
def test_schedule_is_the_recorded_one(mav, recorded, case):
    want, got = recorded[case[0]], pin.record(case)
    assert got["info"] == want["info"]
    assert any(s == 1 for _, s, _ in want["launches"]) == pin.expects_second_stream(case)
    if got["launches"] != want["launches"]:
        first = next((i for i, (a, b) in enumerate(zip(got["launches"], want["launches"])) if a != b), min(len(got["launches"]), len(want["launches"])))
        pytest.fail(f"launch sequence differs from the recording at run {first}: got {got['launches'][first:first + 4]}, "
                    f"recorded {want['launches'][first:first + 4]} ({len(got['launches'])} vs {len(want['launches'])} runs)")

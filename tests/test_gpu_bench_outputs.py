"""bench.py's plain run, its --full run and --dump-outputs, on a small shape.  A plain run times the steps and prints the line, nothing
more; --full adds the checks and legs; --dump-outputs writes the last timed step's records and masks, the same bytes on every run with
the same arguments -- and the same bytes whether or not --full re-runs the batch afterwards.  bench.py runs as a CHILD process (it owns
its GPU context)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE = ["--width", "320", "--height", "240", "--batch", "4", "--steps", "3", "--warmup", "1"]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MAVFLOW_BENCH_DIST", "MAVFLOW_RDZV")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SHAPE + list(extra), env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_full_and_dumped_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in CONTRACT), plain
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["unit"] == "frame-pairs/s" and plain["higher_is_better"] is True
    assert abs(plain["value"] - 4 / (plain["ms_per_step"] * 1e-3)) < 1e-2 * plain["value"]        # (both rounded in the line)
    for k in ("verified_pairs", "verification", "roofline", "cpu_baseline", "video_sequence", "value_incl_h2d", "configs", "api_loop"):
        assert k not in plain, k

    full = _bench("--full", "--cpu-pairs", "1", "--dump-outputs", str(tmp_path / "full"))
    assert full["verified_pairs"] == [0, 3] and full["verification"]["all_pairs_equal_plain_schedule"], full.get("verification")
    assert "roofline" in full and "cpu_baseline" in full and "video_sequence" in full

    again = _bench("--dump-outputs", str(tmp_path / "again"))
    a, f, b = _load(tmp_path / "plain"), _load(tmp_path / "full"), _load(tmp_path / "again")
    assert sorted(a) == sorted(f) == sorted(b) and "records_foe" in a and "mask_dyn_sample" in a
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), (name, a[name].dtype)
        assert a[name].tobytes() == b[name].tobytes() == f[name].tobytes(), name
    assert a["records_box"].shape == (4, 4) and a["mask_fixed_sample"].size == 4 * 320 * 240      # small masks are dumped whole
    assert a["mask_dyn_row_counts"].sum() == a["mask_dyn_sample"].sum()

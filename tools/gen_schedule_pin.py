#!/usr/bin/env python3
"""Record tests/golden/schedule_pin.json: what the Farneback host scheduler launches, case by case (tests/schedule_pin_cases.py),
for tests/test_gpu_schedule_pin.py to compare against.  Needs the GPU and the built library:

    python tools/gen_schedule_pin.py [--out FILE]

Run it on the commit whose schedule is to be pinned -- the parent of a refactor, or a change that alters the schedule on purpose (say
so in that change).  The file holds recorded results only: per case the mav_schedule_info string and the run-length encoded
(kernel class, stream, count) sequence of one call.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import schedule_pin_cases as pin
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "schedule_pin.json"))
    args = ap.parse_args()
    cases = {}
    for case in pin.CASES:
        rec = cases[case[0]] = pin.record(case)
        on_second = sum(n for _, s, n in rec["launches"] if s == 1)
        # an all-zero stream column must not pass silently
        assert (on_second > 0) == pin.expects_second_stream(case), (case[0], on_second)
        print(f"{case[0]}: {sum(n for _, _, n in rec['launches'])} launches, {on_second} on the second stream", flush=True)
    with open(args.out, "w") as f:                      # one case per line: diffs of a regenerated file stay readable
        f.write('{"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()))
        f.write("\n}}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

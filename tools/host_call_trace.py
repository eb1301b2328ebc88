"""What one traced run put on the device, as text to diff between two builds: every kernel dispatch (name, grid, workgroup size) queue
by queue in start order -- dispatches of two queues overlap, so their order against each other is not a property of the build --, then
every memory copy in start order (direction, bytes), then the counts.

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv json -d DIR -o t -- python tools/host_call_pin.py <libmavflow.so>
    python tools/host_call_trace.py DIR > summary.txt

The CSV copy trace carries no sizes; they are taken from the JSON output's copy records, matched by start time."""
import collections
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    out = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)):
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    return sorted(out, key=lambda r: int(r["Start_Timestamp"]))


def copy_bytes(d):
    """{start timestamp: bytes} of every copy record of the JSON output"""
    out = {}

    def walk(v, key=None):
        if isinstance(v, dict):
            if key == "memory_copy" and "bytes" in v and "start_timestamp" in v:
                out[int(v["start_timestamp"])] = int(v["bytes"])
            for k, e in v.items():
                walk(e, k if not isinstance(e, dict) else k)
        elif isinstance(v, list):
            for e in v:
                walk(e, key)
    for f in glob.glob(os.path.join(d, "**", "*_results.json"), recursive=True):
        with open(f) as fh:
            walk(json.load(fh))
    return out


def main(d):
    kernels, copies, sizes = rows(d, "kernel_trace.csv"), rows(d, "memory_copy_trace.csv"), copy_bytes(d)
    queues = {}
    for r in kernels:
        queues.setdefault(r.get("Queue_Id", "?"), []).append(r)
    for i, q in enumerate(queues.values()):              # queues in the order of their first dispatch
        for r in q:
            print("queue %d kernel %s grid %s,%s,%s workgroup %s,%s,%s" % ((i, r["Kernel_Name"]) + tuple(r[f"Grid_Size_{a}"] for a in "XYZ")
                                                                          + tuple(r[f"Workgroup_Size_{a}"] for a in "XYZ")))
    tally = collections.Counter()
    for r in copies:
        n = str(sizes.get(int(r["Start_Timestamp"]), "?"))
        print(f"copy {r.get('Direction', '?')} {n} bytes")
        tally[(r.get("Direction", "?"), n)] += 1
    print(f"{len(kernels)} kernel dispatches, {len(copies)} copies")
    for (direction, n), count in sorted(tally.items(), key=lambda kv: (kv[0][0], int(kv[0][1]) if kv[0][1].isdigit() else 0)):
        print(f"copies {direction} of {n} bytes: {count}")


if __name__ == "__main__":
    main(sys.argv[1])

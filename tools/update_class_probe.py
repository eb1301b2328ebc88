"""The initial-M kernel class (update_matrices) of one BUILD of libmavflow, for comparing two builds: the sum of its launches' HIP-event durations in one profiled Farneback call (Context.profile_get), five calls per shape: the headline 1080p x 64, 4K x 16 / 5 layers, one 720p pair.
python tools/update_class_probe.py <libmavflow.so>"""
import sys
sys.path.insert(0, "mav-detection_amd")
import numpy as np
from mavflow import _lib
_lib.load(sys.argv[1])
from mavflow import synth
out = []
for (W, H, B, levels) in ((1920, 1080, 64, 1), (3840, 2160, 16, 5), (1280, 720, 1, 1)):
    ctx = _lib.Context(W, H, B, _lib.fb_defaults(levels=levels))
    prev, nxt = synth.make_batch(W, H, B, distinct=min(B, 4))
    dp, dn = ctx.alloc(prev.nbytes).upload(prev), ctx.alloc(nxt.nbytes).upload(nxt)
    df = ctx.alloc(8 * B * W * H)
    call = lambda: ctx.farneback_dev(dp.ptr, dn.ptr, B, df.ptr)
    for _ in range(3):
        call()
    ctx.sync()
    vals = []
    for _ in range(5):
        ctx.profile_enable(True)
        call()
        ctx.sync()
        p = ctx.profile_get()
        ctx.profile_enable(False)
        vals.append(p)
    names = [k for k in vals[0] if "update" in k]
    for k in names:
        ms = sorted(v[k][0] for v in vals)
        out.append(f"{W}x{H}x{B} {k}: median {ms[2]:.4f} ms of {vals[0][k][1]} launches (min {ms[0]:.4f}, max {ms[4]:.4f})")
    ctx.close()
print(sys.argv[1].split("/")[-1], " | ".join(out), flush=True)

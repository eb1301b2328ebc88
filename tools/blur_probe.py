#!/usr/bin/env python3
"""Layer-image stage alone: HIP-event time of the blur_resize kernel class (3x3 finest layer + coarse layers) per farneback call,
1080p batch 64 / 1 level, 3840x2160 batch 16 / 5 levels, one 1280x720 pair (the whole pyramid through k_blur_multi) and 1080p batch 64
of uint16 frames.   python tools/blur_probe.py [libmavflow.so]      (another build of the same ABI: alternate two builds to compare)"""
import sys
sys.path.insert(0, "mav-detection_amd")
import numpy as np
from mavflow import _lib, synth

if len(sys.argv) > 1:
    _lib.load(sys.argv[1])

for (W, H, B, L, dt) in ((1920, 1080, 64, 1, np.uint8), (3840, 2160, 16, 5, np.uint8), (1280, 720, 1, 1, np.uint8), (1920, 1080, 64, 1, np.uint16)):
    ctx = _lib.Context(W, H, B, _lib.fb_defaults(levels=L))
    prev, nxt = (a.astype(dt) for a in synth.make_batch(W, H, B, distinct=2))
    dp, dn = ctx.alloc(prev.nbytes).upload(prev), ctx.alloc(nxt.nbytes).upload(nxt)
    flow = ctx.alloc(B * W * H * 8)
    for _ in range(2):
        ctx.farneback_dev(dp.ptr, dn.ptr, B, flow.ptr, depth=dt)
    ctx.sync()
    ctx.profile_enable(1)
    n = 20 if B == 1 else 5
    for _ in range(n):
        ctx.farneback_dev(dp.ptr, dn.ptr, B, flow.ptr, depth=dt)
    ctx.sync()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    print(f"{W}x{H} b{B} L{L} {np.dtype(dt).name}: blur_resize {prof['blur_resize'][0] / n:.4f} ms per call in {prof['blur_resize'][1] // n} launches; "
          f"polyexp {prof['polyexp'][0] / n:.3f} ms")
    ctx.close()

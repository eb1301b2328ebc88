"""The bits of the layer-image kernels of one BUILD of libmavflow, one CRC32 per line: run it on two builds and diff the outputs.

    python tools/layer_bits.py <libmavflow.so> > bits.txt

Stage lines: mav_stage_blur_resize's layer image for every case, layer and depth of tests/stage_cases.py BLUR_CASES, as dispatched
and (where that is a fused form) forced to the two-pass form, for the texture frame and the noise frame.  Pyramid lines:
Context.farneback at 200x200, 3 levels, per depth -- batch 1 takes the whole pyramid through k_blur_multi (5- and 13-tap jobs in one
launch of the mixed tile code), batch 3 the per-layer launches."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests"), ROOT]      # tests/stage_cases.py imports oracle/
import numpy as np
from mavflow import _lib

_lib.load(sys.argv[1])
from mavflow import synth
from stage_cases import BLUR_CASES, DEPTH_DTYPES, blur_form, blur_frames, pyramid


def crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


for case in BLUR_CASES:
    with _lib.Context(case.W, case.H, 1, case.fb()) as ctx:
        for depth in case.depths:
            for k, layer in enumerate(pyramid(case.W, case.H, case.pyr_scale, case.levels)):
                tex, noise = blur_frames(case, depth)
                for two_pass in (False, True):
                    form = blur_form(case.W, case.H, layer, depth, two_pass)
                    if two_pass and form == blur_form(case.W, case.H, layer, depth):
                        continue
                    print(f"stage {case.name} {depth} layer {k} {layer[0]}x{layer[1]} ks {layer[2]} {form}: "
                          f"texture {crc(ctx.stage_blur_resize(tex, k, two_pass=two_pass))} "
                          f"noise {crc(ctx.stage_blur_resize(noise, k, two_pass=two_pass))}")


def frames_of(depth, a, off):
    """u8 frames as they are; the wide depths with values between the u8 levels (16-bit steps, fractions on the 0 .. 255 scale)"""
    if depth == "u8":
        return a
    v = a.astype(np.uint16) * 257 + off
    return v if depth == "u16" else v.astype(np.float32) / np.float32(257)


W, H = 200, 200
for B in (1, 3):
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    with _lib.Context(W, H, B, _lib.fb_defaults(levels=3)) as ctx:
        for depth, dt in DEPTH_DTYPES.items():
            blur = "/".join(l["blur"] for l in ctx.schedule_info(B, dt)["layers"])
            flow = ctx.farneback(frames_of(depth, prev, 3), frames_of(depth, nxt, 5))
            print(f"farneback {W}x{H} levels 3 batch {B} {depth} {blur}: {crc(flow)}")

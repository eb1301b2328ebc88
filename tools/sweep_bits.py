"""The bits of the sweep kernels and of the initial M of one BUILD of libmavflow, one CRC32 per line: run it on two builds and diff the outputs.

    python tools/sweep_bits.py <libmavflow.so> > bits.txt

The box window has no bit-exact reference (its CPU original sums in double), so a change that must not move it is held to the
build before it.  Stage lines: mav_stage_blur_iter's flow and M', update true and false, both windows, on every layer of the small
cases of tests/stage_cases.py with smooth_flow and crafted_flow as the flow M is built from (R0, R1 and M come from the library's own
expansion and UpdateMatrices stages); each also carries the CRC of that M (k_update_matrices MODE 2) and of the zero-flow initial M
(MODE 0).  Initial-M lines: stage_update_matrices_from on a smooth_flow of the coarser layer's size (MODE 1), for every layer that has
a coarser one.  Schedule lines: Context.farneback at 640x480, 3 levels, batch 3, both windows, bands 1 / 2 / 3 x
pairs_in_flight 1 / 2 (the write-through instantiations run in the two-stream schedules)."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests"), ROOT]      # tests/stage_cases.py imports oracle/
import numpy as np
from mavflow import _lib

_lib.load(sys.argv[1])
from mavflow import synth
from stage_cases import CASES, crafted_flow, images, smooth_flow, sweep_form


def crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


for case in CASES:
    if (case.W, case.H) in ((1920, 1080), (3840, 2160)):
        continue
    with _lib.Context(case.W, case.H, 1, case.fb()) as ctx:
        for k in range(ctx.num_layers()):
            w, h = ctx.layer_dims(k)[:2]
            R0, R1 = (ctx.stage_polyexp(ctx.stage_blur_resize(img, k), k) for img in images(case))
            zero = crc(ctx.stage_update_matrices_from(R0, R1, None, k))
            if k + 1 < ctx.num_layers():
                pw, ph = ctx.layer_dims(k + 1)[:2]
                print(f"initial M {case.name} layer {k} {w}x{h} from {pw}x{ph}: "
                      f"{crc(ctx.stage_update_matrices_from(R0, R1, smooth_flow(pw, ph), k))}")
            for tag, flow in (("smooth", smooth_flow(w, h)), ("crafted", crafted_flow(w, h))):
                M = ctx.stage_update_matrices(R0, R1, flow, k)
                for window in ("box", "gaussian"):
                    ctx.set_window(window)
                    f1, M1 = ctx.stage_blur_iter(R0, R1, M, k, True)
                    f0, _ = ctx.stage_blur_iter(R0, R1, M, k, False)
                    print(f"stage {case.name} layer {k} {w}x{h} {sweep_form(w, case.winsize)} {tag} {window}: "
                          f"flow {crc(f1)} M' {crc(M1)} flow(no update) {crc(f0)} M {crc(M)} M(zero flow) {zero}")
                ctx.set_window("box")

W, H, B = 640, 480, 3
prev, nxt = synth.make_batch(W, H, B, distinct=3)
for window in ("box", "gaussian"):
    with _lib.Context(W, H, B, _lib.fb_defaults(levels=3), window=window) as ctx:
        for pif in (1, 2):
            ctx.set_option("pairs_in_flight", pif)
            for bands in (1, 2, 3):
                ctx.set_option("bands", bands)
                print(f"farneback {W}x{H} levels 3 batch {B} {window} pairs_in_flight {pif} bands {bands}: {crc(ctx.farneback(prev, nxt))}")

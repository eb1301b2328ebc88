"""Every host-pointer entry point of one BUILD of libmavflow, called once in a fixed order on seeded inputs, one line per call: the
call, a CRC32 of every buffer it returned, and mav_mem_info's ctx_bytes / workspace_bytes after it.  Run it on two builds and diff:

    python tools/host_call_pin.py <libmavflow.so> > calls.txt

The host entry points stage their arrays in the context's scratch blocks, block i of a call re-using block i of the call before
(grow-only).  A change that must not move what they compute, nor the order and sizes in which they take their blocks, is held to the
build before it: equal CRCs say the first, equal memory figures after every call the second.  One context at 66x33, max_batch 3,
Farneback levels 2 (the frame reaches one layer: a layer below 32 pixels is not built), window-search scale 1.05 (two levels).  The
order includes the awkward cases: process_batch on one run of four frames (next == prev + one frame) and on two arrays, every
call that reads what a host detect left resident twice in a row, and flow_to_color of a float64 field last, because it grows block 0."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np
from mavflow import _lib

_lib.load(sys.argv[1])
from mavflow import synth
import detect_cases as dc

W, H, B = 66, 33, 3
PYR_SCALE = 1.05
N_PAIRS = dc.DETECT_PAIRS


def crc(a):
    if isinstance(a, (bytes, bytearray)):
        return "%08x" % zlib.crc32(a)
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def flat(v):
    """the buffers of a result, in a fixed order: arrays, bytes, and tuples / lists / dicts of them; None for an output not asked for"""
    if v is None:
        return []
    if isinstance(v, dict):
        return [x for k in v for x in flat(v[k])]
    if isinstance(v, (tuple, list)):
        return [x for e in v for x in flat(e)]
    return [v]


def inputs():
    rng = np.random.default_rng(66033)
    frames = np.stack([synth.make_pair(W, H, i)[0] for i in range(B + 1)])          # one run of B + 1 frames
    flow32 = np.array(dc.noise_fields(W, H))
    fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
    fp.n_pairs, fp.mag_threshold = N_PAIRS, dc.DETECT_GATE
    gt = np.where(rng.random((B, H, W)) < 0.3, 255, 0).astype(np.uint8)
    return dict(frames=frames, prev=frames[:-1].copy(), next=frames[1:].copy(), flow32=flow32, flow64=flow32.astype(np.float64),
                foe=dc.foes(W, H), sky=dc.sky_masks(W, H), samples=dc.detect_samples(W, H, B, N_PAIRS), omega=dc.OMEGA, dt=dc.DT,
                frame0=np.array([1, 0, 0], np.uint8), fp=fp, tp=tp, gt=gt, imgs=rng.integers(0, 256, (B, H, W), dtype=np.uint8),
                bgr=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), foe_gt=dc.foes(W, H)[::-1].copy(),
                windows=np.array([[5, 4, 20, 12], [40, 10, 20, 20], [0, 0, 8, 8]], np.int32),
                init=(0.25 * flow32).astype(np.float32))


def calls(ctx, x):
    """(name, thunk) in the pinned order"""
    det = dict(omega=x["omega"], dt=x["dt"], sky=x["sky"], foe_params=x["fp"], thr_params=x["tp"], frame0=x["frame0"])
    k = ctx.num_layers() - 1
    w, h = ctx.layer_dims(k)[:2]
    stage = {}

    def polyexp():
        stage["I"] = [ctx.stage_blur_resize(f, k) for f in x["frames"][:2]]
        stage["R"] = [ctx.stage_polyexp(i, k) for i in stage["I"]]
        return stage["R"]

    def update():
        stage["flow"] = np.ascontiguousarray(x["flow32"][0, :h, :w])
        stage["M"] = ctx.stage_update_matrices(stage["R"][0], stage["R"][1], stage["flow"], k)
        return stage["M"]

    def host_detect():
        return ctx.detect(x["flow32"], x["samples"], want_phi=True, **det)

    out = [
        ("bbox", lambda: ctx.bbox(x["imgs"])),
        ("bgr2gray", lambda: ctx.bgr2gray(x["bgr"])),
        ("window_max", lambda: ctx.window_max(x["imgs"])),
        ("analyze_pyramid", lambda: ctx.analyze_pyramid(x["imgs"], PYR_SCALE)),
        ("stage_pyramid_level 0", lambda: ctx.pyramid_level(x["imgs"], 0, PYR_SCALE)),
        ("stage_pyramid_level 1", lambda: ctx.pyramid_level(x["imgs"], 1, PYR_SCALE)),
        ("optimize_window", lambda: ctx.optimize_window(x["imgs"], x["windows"])),
        ("tpr_fpr_counts", lambda: ctx.tpr_fpr_counts(x["gt"], x["sky"], 255)),
        ("derotate", lambda: ctx.derotate(x["flow32"], x["omega"], x["dt"])),
        ("foe_dense", lambda: ctx.foe_dense(x["flow64"], x["samples"], x["fp"])),
        ("foe_dense_f32", lambda: ctx.foe_dense(x["flow32"], x["samples"], x["fp"])),
        ("phi_mask", lambda: ctx.phi_mask(x["flow64"], x["foe"], x["sky"], x["tp"])),
        ("phi_mask_f32", lambda: ctx.phi_mask(x["flow32"], x["foe"], x["sky"], x["tp"])),
        ("phi_mask masks only", lambda: ctx.phi_mask(x["flow64"], x["foe"], None, x["tp"], want_phi=False)),
        ("farneback", lambda: ctx.farneback(x["prev"], x["next"])),
        ("farneback one run", lambda: ctx.farneback_sequence(x["frames"])),
        ("farneback_init", lambda: ctx.farneback(x["prev"], x["next"], x["init"])),
        ("farneback_ex u16", lambda: ctx.farneback(x["prev"].astype(np.uint16) * 257, x["next"].astype(np.uint16) * 257)),
        ("farneback_ex f32 init", lambda: ctx.farneback(x["prev"].astype(np.float32), x["next"].astype(np.float32), x["init"])),
        ("process_batch one run", lambda: ctx.process_batch(x["frames"][:-1], x["frames"][1:], x["samples"], want_phi=True, **det)),
        ("process_batch two arrays", lambda: ctx.process_batch(x["prev"], x["next"], x["samples"], want_phi=True, **det)),
        ("process_batch records only", lambda: ctx.process_batch(x["prev"], x["next"], x["samples"], foe_params=x["fp"], want_flow=False,
                                                                   want_masks=False)),
        ("detect", host_detect),
    ]
    for name, fn in (("last_masks_tpr_fpr", lambda: ctx.last_masks_tpr_fpr(x["gt"])),
                     ("last_render", lambda: ctx.render_last(B)),
                     ("last_overlay", lambda: ctx.overlay_last(x["bgr"], x["foe_gt"])),
                     ("last_render_png", lambda: ctx.render_last_png(B)),
                     ("last_overlay_png", lambda: ctx.overlay_last_png(x["bgr"], x["foe_gt"]))):
        out += [(name, fn), (name + " again", fn)]
    out += [
        ("last_render flow only", lambda: ctx.render_last(B, images=("flow",))),
        ("render", lambda: ctx.render(x["flow32"], x["foe"], x["omega"], x["dt"], x["sky"], x["tp"], x["frame0"])),
        ("render phi only", lambda: ctx.render(x["flow32"], x["foe"], images=("phi",))),
        ("overlay", lambda: ctx.overlay(x["bgr"], x["sky"], x["foe"], x["foe_gt"])),
        ("png_encode bgr", lambda: ctx.png_encode(x["bgr"])),
        ("png_encode gray", lambda: ctx.png_encode(x["imgs"][0])),
        ("colormap_jet", lambda: ctx.colormap_jet(x["imgs"])),
        ("stage_phi_mask", lambda: ctx.stage_phi_mask(x["flow32"], x["foe"], x["omega"], x["dt"], x["sky"], x["tp"], want_phi=True)),
        ("stage_phi_mask no rates", lambda: ctx.stage_phi_mask(x["flow32"], x["foe"], params=x["tp"])),
        ("stage_coefficients", lambda: ctx.stage_coefficients(k)),
        ("stage_blur_resize + stage_polyexp", polyexp),
        ("stage_blur_resize two-pass", lambda: ctx.stage_blur_resize(x["frames"][0], k, two_pass=True)),
        ("stage_blur_resize u16", lambda: ctx.stage_blur_resize(x["frames"][0].astype(np.uint16) * 257, k)),
        ("stage_blur_resize f32 two-pass", lambda: ctx.stage_blur_resize(x["frames"][0].astype(np.float32), k, two_pass=True)),
        ("stage_update_matrices", update),
        ("stage_update_matrices_from zero", lambda: ctx.stage_update_matrices_from(stage["R"][0], stage["R"][1], None, k)),
        ("stage_initial_flow", lambda: ctx.stage_initial_flow(x["flow32"][0], k)),
        ("stage_blur_iter", lambda: ctx.stage_blur_iter(stage["R"][0], stage["R"][1], stage["M"], k, True)),
        ("stage_blur_iter no update", lambda: ctx.stage_blur_iter(stage["R"][0], stage["R"][1], stage["M"], k, False)),
        ("flow_to_color f32", lambda: ctx.flow_to_color(x["flow32"])),
        ("flow_to_color f64", lambda: ctx.flow_to_color(x["flow64"])),
    ]
    return out


def main():
    x = inputs()
    with _lib.Context(W, H, B, _lib.fb_defaults(levels=2)) as ctx:
        print(f"context {W}x{H} max_batch {B}: {ctx.num_layers()} Farneback layer(s), window-search levels {ctx.pyramid_dims(PYR_SCALE)}")
        for name, fn in calls(ctx, x):
            got = fn()
            m = ctx.mem_info()
            print(f"{name}: {' '.join(crc(b) for b in flat(got))} | ctx_bytes {m['ctx_bytes']} workspace_bytes {m['workspace_bytes']}", flush=True)


if __name__ == "__main__":
    main()

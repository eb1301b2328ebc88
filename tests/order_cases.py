"""What a context keeps between calls, as a table, and the pairs of calls that hold it to "a call's result does not depend on what the
context ran before it".

SCRATCH   every member of mav_ctx and of its sub-structs (FoeScratch, Motion, LkState, WorkSet, DeepSet, mav_history) that is device
          memory outliving a call: who writes it, the rule that makes it safe for the next call, and the source line the rule restates.
FAMILIES  one entry per family of entry points: a `heavy` call, a `light` call on a context of the same (W, H, max_batch), and
          `leaves_more()`, which proves on the CPU -- from the numpy restatements, not from the device -- that heavy leaves strictly more
          behind than light touches.  A stale counter, a short memset or a missing init shows only then.
EXEMPT    entry points that own no device memory surviving a call.
DEFERRED  the Farneback entry points: held by schedule_cases.dirty, their pair of calls here taken out (see there).

tests/test_order_cases_cpu.py reads the table against the headers and the source; tests/test_gpu_call_order.py runs the pairs:
light alone on a fresh context gives the reference bytes L0, and light after heavy (after heavy twice, after the family's part-way
refused forms, with its input at every batch position, after every family's heavy call on one context) must give L0 again.

A family's calls take (ctx, st): st is a dict that lives as long as the context and carries what must persist between a heavy and a
light call of one family (the history ring, the accumulator).  light returns {name: bytes or tuples of bytes}.  Device forms run on the
caller's own blocks (Dev), pre-filled with a canary and longer than the call promises: the tail must come back untouched."""
import ctypes as C
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

import components_cases as cc_cases
import detect_cases as dc
import resident_cases as rc
from resident_cases import p_, vp

ROOT = rc.ROOT
HEADERS = tuple(os.path.join(ROOT, "include", h) for h in ("mavflow.h", "mavflow_truth.h", "mavflow_validation.h"))
CSRC = os.path.join(ROOT, "mav-detection_amd", "csrc")
FRAME = cc_cases.FRAMES[-1]              # (131, 67): no multiple of any tile, more than one workgroup of every per-pixel pass
WALK_FRAME = (rc.W, rc.H)                # (66, 33): resident_cases' frame, for the walk through every family on one context
B = 3                                    # max_batch of every context here
CANARY, SLACK = 0xA5, 64                 # the byte a caller's block is filled with, and how much longer it is than the call promises

RULES = ("memset per call", "init kernel", "self-resetting", "fully overwritten before read", "persistent by contract")


def header_names() -> list:
    """every function the three headers declare"""
    out = []
    for h in HEADERS:
        with open(h) as f:
            out += rc.header_functions(f.read())
    return out


# ---- SCRATCH ----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Scratch:
    struct: str                  # the struct that declares the member (searched in mavflow.cpp, then in mavflow_internal.h)
    member: str
    writers: tuple               # families (FAMILIES' names) or "lifecycle" whose entry points write it
    rule: str                    # one of RULES
    file: str                    # the file under csrc/ the rule restates ...
    line: int                    # ... the line ...
    pattern: str                 # ... and what that line must contain (a regular expression)
    guard: str = ""              # the existing test that already holds it, if it is not this table's

    @property
    def key(self):
        return f"{self.struct}.{self.member}"


def S(struct, member, writers, rule, file, line, pattern, guard=""):
    return Scratch(struct, member, tuple(writers.split()), rule, file, line, pattern, guard)


CPP, DET, VAL, INT = "mavflow.cpp", "kernels_detect.hip", "kernels_validation.hip", "mavflow_internal.h"
FB_GUARD = "schedule_cases.dirty"
SCRATCH = [
    # -- detection scratch (max_batch), allocated by mav_create
    S("FoeScratch", "done", "detect parts", "self-resetting", DET, 192, r"atomic_store\(&sc\.done\[2 \* b\], 0u"),
    S("FoeScratch", "best_key", "detect parts", "init kernel", DET, 76, r"sc\.best_key\[b\] = 0ull"),
    S("FoeScratch", "cand", "detect parts", "fully overwritten before read", DET, 74, r"cand = sc\.cand \+ \(size_t\)b \* 2 \* N"),
    S("FoeScratch", "count", "detect parts", "fully overwritten before read", CPP, 787, r"&c->foe_sc\.count, sizeof\(int\) \* B"),
    S("mav_ctx", "foe_dev", "detect parts", "persistent by contract", CPP, 2011, r"c->last_render\.foe = c->foe_dev"),
    S("mav_ctx", "box_acc", "detect parts", "init kernel", DET, 78, r"box_acc\[4 \* b\] = INT_MAX"),
    S("mav_ctx", "u64_scratch", "detect parts pyramid", "memset per call", CPP, 2792, r"hipMemsetAsync\(c->u64_scratch, 0, sizeof\(unsigned long long\) \* batch"),
    S("mav_ctx", "i32_scratch", "parts", "memset per call", DET, 615, r"hipMemsetAsync\(maxv, 0, sizeof\(int\) \* B"),
    S("mav_ctx", "derot_dev", "detect parts", "persistent by contract", CPP, 2011, r"c->last_render\.derot = a\.derot"),
    S("mav_ctx", "render_max", "parts png global_motion", "memset per call", DET, 1183, r"hipMemsetAsync\(radmax, 0, sizeof\(unsigned long long\) \* B"),
    S("mav_ctx", "render_derot", "parts png", "fully overwritten before read", CPP, 3208, r"&c->render_derot, sizeof\(DerotParams\) \* c->max_batch"),
    S("mav_ctx", "scratch", "detect parts components roc png gt_stats radial history global_motion pyramid farneback",
      "fully overwritten before read", CPP, 475, r"slot i of a call re-uses the block slot i of the previous call"),
    S("mav_ctx", "flow_ws", "detect global_motion", "fully overwritten before read", CPP, 655, r"c->flow_ws \? MAV_OK : c->mem\.alloc\(&c->flow_ws"),
    # -- grow-only workspaces whose contents are not kept
    S("mav_ctx", "cc_ws", "components detect", "fully overwritten before read", CPP, 2066, r"grow_buffer\(c, &c->cc_ws, &c->cc_ws_cap"),
    S("mav_ctx", "png_ws", "png", "fully overwritten before read", CPP, 3628, r"grow_buffer\(c, &c->png_ws, &c->png_ws_cap"),
    S("mav_ctx", "pyr_ws", "pyramid global_motion", "fully overwritten before read", CPP, 2751, r"grow_buffer\(c, &c->pyr_ws, &c->pyr_ws_cap"),
    S("mav_ctx", "sat", "pyramid global_motion", "fully overwritten before read", CPP, 2831, r"launch_optimize_window\(c->stream, di, batch, c->W, c->H, c->sat"),
    S("mav_ctx", "gts_scratch", "gt_stats", "init kernel", VAL, 276, r"hipLaunchKernelGGL\(k_gts_init,"),
    S("mav_ctx", "radial_edges", "radial", "fully overwritten before read", CPP, 4519, r"launch_radial_hist\(c->stream, .*c->radial_edges, resident"),
    # -- global motion (Motion)
    S("Motion", "key", "global_motion", "memset per call", CPP, 2947, r"hipMemsetAsync\(c->gm\.key, 0, sizeof\(unsigned long long\) \* 2 \* batch"),
    S("Motion", "H", "global_motion", "fully overwritten before read", CPP, 496, r"double\* H = nullptr"),
    S("Motion", "ok", "global_motion", "fully overwritten before read", CPP, 496, r"int\* ok = nullptr"),
    S("Motion", "pyr", "global_motion", "fully overwritten before read", CPP, 2953, r"launch_pyramid_finalize\(c->stream, kwin, p, gray, c->pyr_ws, batch, c->gm\.pyr\)"),
    S("Motion", "win", "global_motion", "fully overwritten before read", CPP, 2955, r"c->gm\.win, c->gm\.opt_score, c->gm\.opt_win"),
    S("Motion", "opt_win", "global_motion", "fully overwritten before read", CPP, 2955, r"c->gm\.win, c->gm\.opt_score, c->gm\.opt_win"),
    S("Motion", "opt_score", "global_motion", "fully overwritten before read", CPP, 2955, r"c->gm\.win, c->gm\.opt_score, c->gm\.opt_win"),
    S("Motion", "gray", "global_motion", "fully overwritten before read", CPP, 498, r"the normalised image of a call whose caller does not want it"),
    S("Motion", "src", "global_motion", "fully overwritten before read", CPP, 499, r"double \*src = nullptr, \*dst = nullptr, \*work = nullptr"),
    S("Motion", "dst", "global_motion", "fully overwritten before read", CPP, 499, r"double \*src = nullptr, \*dst = nullptr, \*work = nullptr"),
    S("Motion", "work", "global_motion", "fully overwritten before read", CPP, 499, r"double \*src = nullptr, \*dst = nullptr, \*work = nullptr"),
    S("Motion", "coords", "global_motion", "fully overwritten before read", CPP, 500, r"int32_t\* coords = nullptr"),
    # -- sparse optical flow (LkState)
    S("LkState", "pyr", "good_features lk", "persistent by contract", CPP, 344, r"two frame slots: the resident frame and the one before / after it"),
    S("LkState", "deriv", "lk", "fully overwritten before read", CPP, 4089, r"launch_lk_scharr\(c->stream, k\.pyr\[slot\], k\.dims, levels, k\.deriv\)"),
    S("LkState", "eig", "good_features", "memset per call", CPP, 4112, r"hipMemsetAsync\(a\.grid, 0, words \* sizeof\(unsigned\)"),
    S("LkState", "cand", "good_features lk", "fully overwritten before read", CPP, 4135, r"launch_corner_candidates\(.*k\.cand, k\.counters \+ 1"),
    S("LkState", "counters", "good_features lk", "memset per call", CPP, 4241, r"hipMemsetAsync\(k\.counters \+ 2, 0, MAV_LK_HIST \* sizeof\(unsigned\)"),
    S("LkState", "pts", "lk", "fully overwritten before read", CPP, 4272, r"hipMemcpyAsync\(k\.pts, pts, \(size_t\)n \* 2 \* sizeof\(float\)"),
    S("LkState", "out", "good_features lk", "fully overwritten before read", CPP, 4275, r"hipMemcpyAsync\(next_pts, k\.out, \(size_t\)n \* 2 \* sizeof\(float\)"),
    S("LkState", "status", "lk", "fully overwritten before read", CPP, 4276, r"hipMemcpyAsync\(status, k\.status, \(size_t\)n"),
    # -- flow history
    S("mav_history", "ring", "history", "persistent by contract", CPP, 3400, r"hipMemsetAsync\(h->ring, 0, h->ring_bytes, c->stream\)"),
    # -- the Farneback workspace: every slot is dirtied before every compared call of the schedule tests
    S("WorkSet", "Htmp", "farneback detect global_motion", "fully overwritten before read", CPP, 388, r"float \*Htmp = nullptr", FB_GUARD),
    S("WorkSet", "I", "farneback detect global_motion", "fully overwritten before read", CPP, 391, r"float \*I = nullptr, \*R = nullptr", FB_GUARD),
    S("WorkSet", "R", "farneback detect global_motion", "fully overwritten before read", CPP, 391, r"float \*I = nullptr, \*R = nullptr", FB_GUARD),
    S("WorkSet", "Ma", "farneback detect global_motion", "fully overwritten before read", CPP, 391, r"\*Ma = nullptr, \*Mb = nullptr", FB_GUARD),
    S("WorkSet", "Mb", "farneback detect global_motion", "fully overwritten before read", CPP, 391, r"\*Ma = nullptr, \*Mb = nullptr", FB_GUARD),
    S("WorkSet", "fc", "farneback detect global_motion", "fully overwritten before read", CPP, 391, r"\*fc\[2\] = \{nullptr, nullptr\}", FB_GUARD),
    S("WorkSet", "Ic", "farneback detect global_motion", "fully overwritten before read", CPP, 394, r"float \*Ic = nullptr, \*Rc = nullptr", FB_GUARD),
    S("WorkSet", "Rc", "farneback detect global_motion", "fully overwritten before read", CPP, 394, r"float \*Ic = nullptr, \*Rc = nullptr", FB_GUARD),
    S("DeepSet", "I", "farneback detect global_motion", "fully overwritten before read", CPP, 402, r"struct DeepSet \{ float \*I = nullptr", FB_GUARD),
    S("DeepSet", "R", "farneback detect global_motion", "fully overwritten before read", CPP, 402, r"struct DeepSet \{ float \*I = nullptr, \*R = nullptr", FB_GUARD),
    S("DeepSet", "Ma", "farneback detect global_motion", "fully overwritten before read", CPP, 402, r"\*Ma = nullptr, \*Mb = nullptr", FB_GUARD),
    S("DeepSet", "Mb", "farneback detect global_motion", "fully overwritten before read", CPP, 402, r"\*Ma = nullptr, \*Mb = nullptr", FB_GUARD),
    S("DeepSet", "f", "farneback detect global_motion", "fully overwritten before read", CPP, 402, r"\*f\[2\] = \{nullptr, nullptr\}", FB_GUARD),
    S("mav_ctx", "init_snap", "farneback", "fully overwritten before read", CPP, 1771, r"launch_area_resize_flow\(c->stream, flow0, .*c->init_snap, c->init_stride"),
]


def struct_body(name: str) -> str:
    """the text between the braces of `struct name {` in mavflow.cpp or mavflow_internal.h"""
    for fn in (CPP, INT):
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        m = re.search(rf"\bstruct {name}\s*\{{", src)
        if not m:
            continue
        depth, j = 0, m.end() - 1
        while True:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            j += 1
            if depth == 0:
                return src[m.end():j - 1]
    raise KeyError(name)


def device_pointers(name: str) -> set:
    """the members of struct `name` declared as pointers to device data (nested structs left out): what SCRATCH must list"""
    body = struct_body(name)
    flat, depth, out = [], 0, set()
    for ch in body:                                   # drop nested struct bodies
        depth += ch == "{"
        if depth == 0:
            flat.append(ch)
        depth -= ch == "}"
    text = re.sub(r"//[^\n]*", "", "".join(flat))
    for stmt in text.split(";"):
        if "*" not in stmt or "(" in stmt:
            continue
        for m in re.finditer(r"\*\s*(\w+)", stmt):
            out.add(m.group(1))
    return out


# members that are pointers but no device memory of a call's: host objects, views into somebody else's block, device state that is not data
NOT_SCRATCH = {
    "mav_ctx": {"stager": "host object", "worker": "host object", "last_flow": "a view: where the newest flow call wrote (resident_cases)",
                "last_mf": "a view into the staging blocks (resident_cases)", "last_md": "a view into the staging blocks (resident_cases)"},
    "LkState": {}, "FoeScratch": {}, "Motion": {}, "WorkSet": {}, "DeepSet": {}, "mav_history": {},
}
STRUCTS = tuple(NOT_SCRATCH)


# ---- device blocks of the caller's ------------------------------------------------------------------------------------------------------
class Dev:
    """The caller-owned device blocks of one call.  inp(array): made and filled.  out(nbytes): filled with CANARY, SLACK bytes longer
    than promised.  get(ptr, dtype, shape): the promised bytes, after the tail was seen untouched."""

    def __init__(self, ctx):
        self.ctx, self.bufs, self.outs = ctx, [], {}

    def inp(self, a):
        a = np.ascontiguousarray(a)
        b = self.ctx.alloc(max(a.nbytes, 1)).upload(a)
        self.bufs.append(b)
        return b.ptr

    def out(self, nbytes):
        nbytes = int(nbytes)
        b = self.ctx.alloc(nbytes + SLACK).upload(np.full(nbytes + SLACK, CANARY, np.uint8))
        self.bufs.append(b)
        self.outs[b.ptr] = (b, nbytes)
        return b.ptr

    def raw(self, ptr) -> np.ndarray:
        """the whole block as bytes (the stream is drained first); the tail is checked"""
        b, n = self.outs[ptr]
        self.ctx.sync()
        a = b.download(np.uint8, (n + SLACK,))
        assert (a[n:] == CANARY).all(), f"a device form wrote past the {n} bytes it promises"
        return a[:n]

    def get(self, ptr, dtype, shape) -> np.ndarray:
        a = self.raw(ptr)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return a[:n].view(dtype).reshape(shape).copy()

    def close(self):
        self.ctx.sync()
        for b in self.bufs:
            b.free()
        self.bufs, self.outs = [], {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def by(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


# ---- inputs (functions of the frame, computed once, read-only) ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_u8(W, H, n=B + 1, first=0):
    from mavflow import synth
    a = np.stack([synth.make_pair(W, H, first + i)[0] for i in range(n)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def detect_inputs(W, H) -> dict:
    from mavflow import _lib
    rng = np.random.default_rng(131067 + W)
    fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
    fp.n_pairs, fp.mag_threshold = dc.DETECT_PAIRS, dc.DETECT_GATE
    tp.fixed_deg, tp.fixed_min_mag = 2.0, 0.25                   # dense fixed masks: most pixels of a noise field are 2 degrees off radial
    fl = _lib.foe_defaults()
    fl.n_pairs, fl.mag_threshold = 4, dc.DETECT_GATE
    f = frames_u8(W, H)
    v = dict(flow=np.array(dc.noise_fields(W, H)), samples=dc.detect_samples(W, H, B, dc.DETECT_PAIRS), omega=dc.OMEGA.copy(), dt=dc.DT.copy(),
             sky=dc.sky_masks(W, H).astype(np.uint8), frame0=np.array([1, 0, 0], np.uint8), fp=fp, tp=tp, foe=dc.foes(W, H),
             prev=f[:-1].copy(), next=f[1:].copy(), gt=np.where(rng.random((B, H, W)) < 0.3, 255, 0).astype(np.uint8),
             bgr=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8),
             # the light call: one pair, four line pairs, a field without motion -- no candidate passes the gate, no pixel a threshold
             l_flow=np.zeros((1, H, W, 2), np.float32), l_samples=dc.detect_samples(W, H, 1, 4, seed=3), l_fp=fl, l_tp=_lib.thr_defaults(),
             l_frames=np.full((1, H, W), 90, np.uint8), l_gt=np.where(rng.random((1, H, W)) < 0.5, 255, 0).astype(np.uint8),
             l_bgr=np.full((1, H, W, 3), 77, np.uint8))
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


def _par_block(samples, omega, dt, frame0):
    """samples | omega | dt | frame0 packed as a frame step reads them; -> (bytes, offsets)"""
    parts = [np.ascontiguousarray(samples, np.uint32), np.ascontiguousarray(omega, np.float64), np.ascontiguousarray(dt, np.float64),
             np.ascontiguousarray(frame0, np.uint8)]
    off, blob = [], b""
    for a in parts:
        blob += b"\0" * (-len(blob) % 8)
        off.append(len(blob))
        blob += a.tobytes()
    return np.frombuffer(blob, np.uint8).copy(), off


def frame_step(ctx, d: Dev, n, prev, nxt, samples, fp, tp, omega=None, dt=None, frame0=None, sky=None, gt=None, compute_flow=1, out_words=0):
    """(step, pointers) of one mav_frame_step on the caller's blocks: Farneback of the frames, the detection, and with gt the counts
    (and, armed, the sweep tables) behind the records in the out block"""
    from mavflow import _lib
    W, H = ctx.W, ctx.H
    om = np.zeros((n, 3)) if omega is None else omega
    par, off = _par_block(samples, om, np.ones(n) if dt is None else dt, np.zeros(n, np.uint8) if frame0 is None else frame0)
    s = _lib.FrameStep()
    s.n, s.par_dev, s.compute_flow = n, d.inp(par), compute_flow
    p = dict(flow=d.out(8 * W * H * n), mf=d.out(W * H * n), md=d.out(W * H * n), res=d.out(32 * n + 64 * n + 8 * out_words))
    s.prev_dev, s.next_dev, s.flow_dev = d.inp(prev), d.inp(nxt), p["flow"]
    s.detect = 1
    s.off_samples, s.off_omega, s.off_dt, s.off_frame0 = off
    s.has_omega, s.has_frame0 = int(omega is not None), int(frame0 is not None)
    s.sky_dev = None if sky is None else d.inp(sky)
    if gt is not None:
        s.gt_dev, s.gt_images = d.inp(gt), n
        s.off_counts_fixed, s.off_counts_dyn = 32 * n, 32 * n + 32 * n
    s.foe, s.thr = fp, tp
    s.mask_fixed_dev, s.mask_dyn_dev, s.out_dev = p["mf"], p["md"], p["res"]
    return s, p


def _step_outputs(ctx, d, p, n):
    W, H = ctx.W, ctx.H
    return (by(d.get(p["flow"], np.float32, (n, H, W, 2))), by(d.get(p["mf"], np.uint8, (n, H, W))), by(d.get(p["md"], np.uint8, (n, H, W))),
            by(d.raw(p["res"])))


# ---- family: detect -------------------------------------------------------------------------------------------------------------------------
def detect_heavy(ctx, st):
    from mavflow import _lib
    x = detect_inputs(ctx.W, ctx.H)
    kw = dict(omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"], foe_params=x["fp"], thr_params=x["tp"])
    ctx.detect(x["flow"], x["samples"], want_phi=True, **kw)
    ctx.process_batch(x["prev"], x["next"], x["samples"], want_phi=True, **kw)
    with Dev(ctx) as d:
        s, p = frame_step(ctx, d, B, x["prev"], x["next"], x["samples"], x["fp"], x["tp"], x["omega"], x["dt"], x["frame0"], x["sky"], gt=x["gt"])
        _lib.check(ctx.lib.mav_frame_step_dev(ctx.h, C.byref(s)))
        ctx.wait_step(ctx.post_step(s))
        ctx.drain()
        res = d.out(32 * B)
        ctx.process_batch_dev(s.prev_dev, s.next_dev, d.inp(x["samples"]), B, res, omega_ptr=d.inp(x["omega"]), dt_ptr=d.inp(x["dt"]),
                              sky_ptr=s.sky_dev, mf_ptr=p["mf"], md_ptr=p["md"], foe_params=x["fp"], thr_params=x["tp"], frame0_ptr=d.inp(x["frame0"]))
        ctx.sync()


def detect_light(ctx, st) -> dict:
    from mavflow import _lib
    x, W, H = detect_inputs(ctx.W, ctx.H), ctx.W, ctx.H
    out = {}
    got = ctx.detect(x["l_flow"], x["l_samples"], foe_params=x["l_fp"], thr_params=x["l_tp"])
    out["detect"] = (by(got["results"]), by(got["mask_fixed"]), by(got["mask_dyn"]))
    out["render_last"] = tuple(by(v) for v in ctx.render_last(1).values())
    out["counts_last"] = tuple(by(v) for v in ctx.last_masks_tpr_fpr(x["l_gt"]))
    ov, wr = ctx.overlay_last(x["l_bgr"], [(5.0, 6.0)])
    out["overlay_last"] = (by(ov), by(wr))
    got = ctx.process_batch(x["l_frames"], x["l_frames"], x["l_samples"], foe_params=x["l_fp"], thr_params=x["l_tp"])
    out["process_batch"] = (by(got["flow"]), by(got["results"]), by(got["mask_fixed"]), by(got["mask_dyn"]))
    out["last_flow"] = by(ctx.last_flow(0))
    with Dev(ctx) as d:
        # mav_detect_dev, mav_process_batch_dev, the frame step (direct and posted) on the caller's own blocks
        mf, md, res = d.out(W * H), d.out(W * H), d.out(32)
        _lib.check(ctx.lib.mav_detect_dev(ctx.h, vp(d.inp(x["l_flow"])), vp(d.inp(x["l_samples"])), None, None, None, None, 1, C.byref(x["l_fp"]),
                                          C.byref(x["l_tp"]), None, vp(mf), vp(md), vp(res)))
        out["detect_dev"] = (by(d.raw(res)), by(d.raw(mf)), by(d.raw(md)))
        s, p = frame_step(ctx, d, 1, x["l_frames"], x["l_frames"], x["l_samples"], x["l_fp"], x["l_tp"], gt=x["l_gt"])
        _lib.check(ctx.lib.mav_frame_step_dev(ctx.h, C.byref(s)))
        out["frame_step_dev"] = _step_outputs(ctx, d, p, 1)
        s, p = frame_step(ctx, d, 1, x["l_frames"], x["l_frames"], x["l_samples"], x["l_fp"], x["l_tp"], gt=x["l_gt"])
        t = ctx.post_step(s)
        _lib.check(ctx.lib.mav_worker_wait_enqueued(ctx._h, C.c_uint64(t)))
        ctx.wait_step(t)
        ctx.drain()
        out["frame_step_post"] = _step_outputs(ctx, d, p, 1)
        flow, res = d.out(8 * W * H), d.out(32)
        ctx.process_batch_dev(s.prev_dev, s.next_dev, d.inp(x["l_samples"]), 1, res, flow_ptr=flow, mf_ptr=p["mf"], md_ptr=p["md"],
                              foe_params=x["l_fp"], thr_params=x["l_tp"])
        out["process_batch_dev"] = (by(d.raw(flow)), by(d.raw(res)), by(d.raw(p["mf"])), by(d.raw(p["md"])))
    return out


def detect_restate(L0, W, H):
    """a field without motion: no pixel passes a magnitude gate, both masks are empty, no candidate reaches the vote: FoE (0, 0)"""
    from mavflow import _lib
    zeros = bytes(W * H)
    for k in ("detect", "detect_dev"):
        assert L0[k][1] == zeros and L0[k][2] == zeros, k
        assert np.frombuffer(L0[k][0], _lib.RESULT_DTYPE)["foe"].tolist() == [[0.0, 0.0]], k
    for k in ("process_batch", "frame_step_dev"):                # equal frames: zero flow
        assert not np.frombuffer(L0[k][0], np.float32).any(), k
    assert L0["process_batch"][2] == zeros and L0["frame_step_dev"][1] == zeros and L0["frame_step_post"] == L0["frame_step_dev"]


@functools.lru_cache(maxsize=None)
def detect_left(W, H) -> dict:
    """what the oracle says the heavy and the light detection leave: vote candidates, set pixels of both masks"""
    from oracle import foe_oracle as fo
    x = detect_inputs(W, H)
    tp = x["tp"]
    cand = fixed = dyn = 0
    for b in range(B):
        der = fo.derotate(x["flow"][b], x["omega"][b], float(x["dt"][b]), 0 if x["frame0"][b] else 1)
        inter = fo.line_intersections(der, x["samples"][b], dc.DETECT_GATE)
        cand += int((inter[:, 0] != 0.0).sum())
        foe = fo.get_foe_dense(der, x["samples"][b], dc.DETECT_GATE)
        with np.errstate(all="ignore"):
            f, t = fo.threshold_masks(fo.get_phi(der, foe), fo.get_magnitude(der), x["sky"][b] != 0, fixed_deg=tp.fixed_deg, fixed_min_mag=tp.fixed_min_mag)
        fixed, dyn = fixed + int(f.sum()), dyn + int(t.sum())
    lz = x["l_flow"][0]
    l_cand = int((fo.line_intersections(lz, x["l_samples"][0], dc.DETECT_GATE)[:, 0] != 0.0).sum())
    return dict(heavy=dict(batch=B, n_pairs=dc.DETECT_PAIRS, cand=cand, fixed=fixed, dyn=dyn),
                light=dict(batch=1, n_pairs=4, cand=l_cand, fixed=int((fo.get_magnitude(lz) > 1.0).sum()), dyn=int((fo.get_magnitude(lz) > 0.5).sum())))


def detect_leaves_more() -> bool:
    v = detect_left(*FRAME)
    h, l = v["heavy"], v["light"]
    return all(h[k] > l[k] for k in h) and l["cand"] == l["fixed"] == l["dyn"] == 0 and h["fixed"] > FRAME[0] * FRAME[1]     # more than a third of 3 frames


def detect_refused(ctx, st):
    """resident_cases.ENQUEUED_BEFORE_REFUSAL: the frame step that computes flow and is then refused inside its detection (n_pairs = 0):
    its gathers and its Farneback have run.  And the host calls whose HostCall::fresh has run when the refusal comes."""
    from mavflow import _lib
    x = detect_inputs(ctx.W, ctx.H)
    bad = _lib.foe_defaults()
    bad.n_pairs, bad.mag_threshold = 0, dc.DETECT_GATE
    with Dev(ctx) as d:
        s, p = frame_step(ctx, d, B, x["prev"], x["next"], x["samples"], bad, x["tp"], x["omega"], x["dt"], x["frame0"], x["sky"])
        assert ctx.lib.mav_frame_step_dev(ctx.h, C.byref(s)) == rc.ERR_ARG
    kw = dict(omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"], foe_params=bad, thr_params=x["tp"])
    empty = np.zeros((B, 0, 2), np.uint32)
    assert rc.code(ctx.detect, x["flow"], empty, **kw) == rc.ERR_ARG
    assert rc.code(ctx.process_batch, x["prev"], x["next"], empty, **kw) == rc.ERR_ARG


def detect_batched(ctx, items):
    """ctx.detect of one call; items: "light" | "heavy" per batch position -> per position the comparable outputs"""
    x = detect_inputs(ctx.W, ctx.H)
    n = len(items)
    flow = np.stack([x["l_flow"][0] if it == "light" else x["flow"][i] for i, it in enumerate(items)])
    smp = np.stack([np.concatenate([x["l_samples"][0]] * (dc.DETECT_PAIRS // 4)) if it == "light" else x["samples"][i] for i, it in enumerate(items)])
    sky = np.stack([x["sky"][1] if it == "light" else x["sky"][i] for i, it in enumerate(items)])
    got = ctx.detect(flow, smp, sky=sky, foe_params=x["fp"], thr_params=x["tp"])
    return [(by(got["results"][i]), by(got["mask_fixed"][i]), by(got["mask_dyn"][i])) for i in range(n)]


# ---- family: parts (the single stages of the detection, which share its scratch) -----------------------------------------------------------------
def _estimates(n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal((40.0, 25.0), 3.0, (n - 2, 2)), [[400.0, -90.0], [-300.0, 250.0]]])


def _parts(ctx, n, light):
    """every single-stage call at batch n; light: the one-pair inputs (other data than the heavy call's first pair)"""
    from mavflow import _lib
    x, W, H = detect_inputs(ctx.W, ctx.H), ctx.W, ctx.H
    sl = slice(2, 3) if light else slice(0, n)
    flow, foe, sky, om, dt, gt, bgr = x["flow"][sl], x["foe"][sl], x["sky"][sl], x["omega"][sl], x["dt"][sl], x["gt"][sl], x["bgr"][sl]
    fp = _lib.foe_defaults()
    fp.n_pairs, fp.mag_threshold = (8 if light else dc.DETECT_PAIRS), dc.DETECT_GATE
    smp = dc.detect_samples(W, H, n, fp.n_pairs, seed=5)
    out = {}
    out["derotate"] = by(ctx.derotate(flow, om, dt))
    out["foe_dense_f32"] = by(ctx.foe_dense(flow, smp, fp))
    out["foe_dense"] = by(ctx.foe_dense(flow.astype(np.float64), smp, fp))
    out["ransac"] = by(np.asarray(ctx.ransac(_estimates(9 if light else 400, 3 if light else 4), 30.0), np.float64))
    out["bgr2gray"] = by(ctx.bgr2gray(bgr))
    for name, f in (("phi_mask_f32", flow), ("phi_mask", flow.astype(np.float64))):
        got = ctx.phi_mask(f, foe, sky=sky, params=x["tp"] if not light else None)
        out[name] = tuple(by(v) for v in (got if isinstance(got, (tuple, list)) else got.values()) if v is not None and not np.isscalar(v))
    out["bbox"] = by(ctx.bbox(sky * np.uint8(255)))
    out["tpr_fpr_counts"] = by(ctx.tpr_fpr_counts(gt, sky))
    out["render"] = tuple(by(v) for v in ctx.render(flow, foe, omega=om, dt=dt, sky=sky, thr_params=x["tp"]).values())
    out["flow_to_color"] = by(ctx.flow_to_color(flow))
    out["colormap_jet"] = by(ctx.colormap_jet(gt))
    ov, wr = ctx.overlay(bgr, sky, foe, foe[::-1].copy() if n > 1 else foe + 3.0)
    out["overlay"] = (by(ov), by(wr))
    with Dev(ctx) as d:
        px = W * H * n
        dflow, dfoe, dsky, dgt, dbgr = d.inp(flow), d.inp(foe), d.inp(sky), d.inp(gt), d.inp(bgr)
        imgs = [d.out(3 * px) for _ in range(3)]
        ctx.render_dev(dflow, dfoe, n, imgs[0], imgs[1], imgs[2], omega_ptr=d.inp(om), dt_ptr=d.inp(dt), sky_ptr=dsky, thr_params=x["tp"])
        out["render_dev"] = tuple(by(d.raw(p)) for p in imgs)
        cnt = d.out(32 * n)
        _lib.check(ctx.lib.mav_tpr_fpr_counts_dev(ctx.h, vp(dgt), n, vp(dsky), None, 255, n, vp(cnt), None))
        out["tpr_fpr_counts_dev"] = by(d.raw(cnt))
        gray = d.out(px)
        _lib.check(ctx.lib.mav_bgr2gray_dev(ctx.h, vp(dbgr), n, vp(gray)))
        out["bgr2gray_dev"] = by(d.raw(gray))
        ov, wr = d.out(3 * px), d.out(n)
        ctx.overlay_dev(dbgr, dsky, dfoe, dfoe, n, ov, wr)
        out["overlay_dev"] = (by(d.raw(ov)), by(d.raw(wr)))
    return out


def parts_heavy(ctx, st):
    _parts(ctx, B, False)


def parts_light(ctx, st):
    out = _parts(ctx, 1, True)
    # what the device forms write is what the host forms return
    assert out["render_dev"] == out["render"] and out["tpr_fpr_counts_dev"] == out["tpr_fpr_counts"] and out["bgr2gray_dev"] == out["bgr2gray"]
    return out


def parts_restate(L0, W, H):
    """the stages a line of numpy restates: the box of an image, the four sums of calculate_tpr_fpr"""
    import roc_ref
    from oracle import foe_oracle as fo
    x = detect_inputs(W, H)
    sky, gt = x["sky"][2], x["gt"][2]
    assert tuple(int(v) for v in np.frombuffer(L0["bbox"], np.int32)) == fo.simple_bounding_box(sky * 255)
    assert tuple(int(v) for v in np.frombuffer(L0["tpr_fpr_counts"], np.int64)) == roc_ref.sums(gt.astype(np.int64), (sky != 0).astype(np.int64))


@functools.lru_cache(maxsize=None)
def parts_left(W, H) -> dict:
    """what the oracle says the single stages leave at batch 3 and at the light call's one pair: vote candidates of foe_dense, inliers of
    the winning estimate of ransac, set pixels of phi_mask's two masks, set pixels under the counts"""
    from oracle import foe_oracle as fo
    x = detect_inputs(W, H)

    def left(idx, n_pairs, n_est, seed, tp):
        smp = dc.detect_samples(W, H, len(idx), n_pairs, seed=5)
        cand = sum(int((fo.line_intersections(x["flow"][b].astype(np.float64), smp[i], dc.DETECT_GATE)[:, 0] != 0.0).sum()) for i, b in enumerate(idx))
        est = _estimates(n_est, seed)
        win = np.asarray(fo.ransac(est, 30.0), np.float64)
        inliers = int((np.hypot(*(est - win).T) < 30.0).sum())
        fixed = dyn = 0
        for b in idx:
            f64 = x["flow"][b].astype(np.float64)
            with np.errstate(all="ignore"):
                f, t = fo.threshold_masks(fo.get_phi(f64, tuple(x["foe"][b])), fo.get_magnitude(f64), x["sky"][b] != 0, **tp)
            fixed, dyn = fixed + int(f.sum()), dyn + int(t.sum())
        return dict(batch=len(idx), cand=cand, inliers=inliers, fixed=fixed, dyn=dyn, sky=int((x["sky"][idx] != 0).sum()))
    return dict(heavy=left([0, 1, 2], dc.DETECT_PAIRS, 400, 4, dict(fixed_deg=x["tp"].fixed_deg, fixed_min_mag=x["tp"].fixed_min_mag)),
                light=left([2], 8, 9, 3, {}))


def parts_leaves_more() -> bool:
    v = parts_left(*FRAME)
    return all(v["heavy"][k] > v["light"][k] for k in v["heavy"]) and v["light"]["sky"] > 0


def parts_refused(ctx, st):
    """the host calls of this family that are refused behind their HostCall::fresh (resident_cases.FRESH_BEFORE_REFUSAL)"""
    from mavflow import _lib
    x = detect_inputs(ctx.W, ctx.H)
    bad = _lib.foe_defaults()
    bad.n_pairs = 0
    assert rc.code(ctx.foe_dense, x["flow"].astype(np.float64), np.zeros((B, 0, 2), np.uint32), bad) == rc.ERR_ARG
    assert rc.code(ctx.tpr_fpr_counts, x["gt"], x["sky"], 0) == rc.ERR_ARG


def parts_batched(ctx, items):
    x = detect_inputs(ctx.W, ctx.H)
    idx = [2 if it == "light" else i % 2 for i, it in enumerate(items)]
    flow, foe, sky = x["flow"][idx], x["foe"][idx], x["sky"][idx]
    r = ctx.render(flow, foe, omega=x["omega"][idx], dt=x["dt"][idx], sky=sky)
    c = ctx.tpr_fpr_counts(x["gt"][idx], sky)
    return [tuple(by(v[i]) for v in r.values()) + (by(c[i]),) for i in range(len(items))]


# ---- family: components ---------------------------------------------------------------------------------------------------------------------
CC_HEAVY = ("noise_41",) * B
CC_LIGHT = ("corners", "empty", "full")


@functools.lru_cache(maxsize=None)
def cc_case(names, connectivity, W, H):
    return cc_cases.Case("order", W, H, names, connectivity)


def _components(ctx, c, labels, dev):
    from mavflow import _lib
    n, mb = len(c.names), c.max_blobs
    if not dev:
        got = ctx.components(c.masks, connectivity=c.connectivity, max_blobs=mb, labels=labels)
        return (by(got["n_components"]), by(got["n_blobs"])) + tuple(by(b) for b in got["blobs"]) + ((by(got["labels"]),) if labels else ())
    with Dev(ctx) as d:
        cnt, tab = d.out(8 * n), d.out(40 * mb * n)
        lab = d.out(4 * ctx.W * ctx.H * n) if labels else None
        ctx.components_dev(d.inp(c.masks), n, cnt, tab, labels_ptr=lab, connectivity=c.connectivity, max_blobs=mb)
        return (by(d.raw(cnt)), by(d.raw(tab))) + ((by(d.raw(lab)),) if labels else ())


def components_heavy(ctx, st):
    c = cc_case(CC_HEAVY, 8, ctx.W, ctx.H)
    for mb in (None, 0):                                         # "cc_workspace_mb" default, then 0: one image per sub-batch
        if mb is not None:
            ctx.set_option("cc_workspace_mb", mb)
        _components(ctx, c, True, False)
        _components(ctx, c, True, True)
    ctx.set_option("cc_workspace_mb", 256)
    x = detect_inputs(ctx.W, ctx.H)
    ctx.detect(x["flow"], x["samples"], foe_params=x["fp"], thr_params=x["tp"])
    ctx.components_last(B, "fixed", connectivity=8, max_blobs=4096, labels=True)


def components_light(ctx, st):
    out = {}
    for name in CC_LIGHT:
        c = cc_case((name,), 4, ctx.W, ctx.H)
        out[name] = _components(ctx, c, False, False)
        out[name + " dev"] = _components(ctx, c, False, True)
    x = detect_inputs(ctx.W, ctx.H)
    ctx.detect(x["l_flow"], x["l_samples"], foe_params=x["l_fp"], thr_params=x["l_tp"])
    got = ctx.components_last(1, "fixed", connectivity=4, max_blobs=8)
    out["components_last"] = (by(got["n_components"]), by(got["n_blobs"])) + tuple(by(b) for b in got["blobs"])
    return out


def components_restate(L0, W, H):
    for name in CC_LIGHT:
        c = cc_case((name,), 4, W, H)
        _, counts, tables = c.expected
        n = min(int(counts["n_blobs"][0]), c.max_blobs)
        assert L0[name] == (by(counts["n_components"]), by(counts["n_blobs"]), by(tables[0, :n])), name
        assert L0[name + " dev"] == (by(counts), by(tables)), name
    assert L0["components_last"][:2] == (by(np.zeros(1, np.int32)), by(np.zeros(1, np.int32)))      # an empty mask


def components_leaves_more() -> bool:
    h = cc_case(CC_HEAVY, 8, *FRAME)
    nh = int(h.expected[1]["n_components"].min())
    nl = max(int(cc_case((n,), 4, *FRAME).expected[1]["n_components"][0]) for n in CC_LIGHT)
    return nh > nl and nl == 4 and int((h.masks != 0).sum()) > 0 and h.max_blobs > 4


def components_batched(ctx, items):
    names = tuple("corners" if it == "light" else "noise_41" for it in items)
    masks = np.stack([cc_cases.patterns(ctx.W, ctx.H)[n] for n in names])
    got = ctx.components(masks, connectivity=4, max_blobs=4096, labels=True)
    return [(by(got["n_components"][i]), by(got["n_blobs"][i]), by(got["blobs"][i]), by(got["labels"][i])) for i in range(len(items))]


# ---- family: roc ----------------------------------------------------------------------------------------------------------------------------
def _roc_grid(light):
    import roc_cases
    return ([15.0], [1.0]) if light else roc_cases.GRIDS["max"]


def _roc(ctx, n, light):
    from mavflow import _lib
    x = detect_inputs(ctx.W, ctx.H)
    a, m = _roc_grid(light)
    sl = slice(1, 2) if light else slice(0, n)
    flow, foe, sky, gt, om, dt = x["flow"][sl], x["foe"][sl], x["sky"][sl], x["gt"][sl], x["omega"][sl], x["dt"][sl]
    out = {"roc_sweep": by(ctx.roc_sweep(flow, foe, gt, a, m, omega=om, dt=dt, sky=sky)["counts"])}
    words = _lib.roc_table_words(len(a), len(m))
    with Dev(ctx) as d:
        tab = d.out(8 * words * n)
        ctx.roc_sweep_dev(d.inp(flow), d.inp(foe), d.inp(gt), n, n, a, m, tab, omega_ptr=d.inp(om), dt_ptr=d.inp(dt), sky_ptr=d.inp(sky))
        out["roc_sweep_dev"] = by(_lib.roc_expand(d.get(tab, np.int64, (n, words)), len(a), len(m)))
    smp = x["samples"][sl]
    ctx.detect(flow, smp, omega=om, dt=dt, sky=sky, foe_params=x["fp"], thr_params=x["tp"])
    out["roc_sweep_last"] = by(ctx.roc_sweep_last(n, gt, a, m)["counts"])
    with Dev(ctx) as d:
        # a frame step while armed writes its tables behind its counts; after roc_arm(None) the same step writes none
        for armed in (True, False):
            ctx.roc_arm(a, m, off_table=96 * n) if armed else ctx.roc_arm(None)
            s, p = frame_step(ctx, d, n, x["prev"][sl], x["next"][sl], smp, x["fp"], x["tp"], om, dt, None, sky, gt=gt, out_words=words * n)
            _lib.check(ctx.lib.mav_frame_step_dev(ctx.h, C.byref(s)))
            blk = d.raw(p["res"])
            out["step armed" if armed else "step disarmed"] = by(blk)
            if not armed:
                assert (blk[96 * n:] == CANARY).all(), "a frame step after roc_arm(None) wrote a sweep table"
    return out


def roc_heavy(ctx, st):
    _roc(ctx, B, False)


def roc_light(ctx, st):
    out = _roc(ctx, 1, True)
    assert out["roc_sweep"] == out["roc_sweep_dev"]
    return out


def roc_restate(L0, W, H):
    """the 1 x 1 grid's cell is tpr_fpr_counts of the fixed mask at those two thresholds: pos + neg = every pixel, tp <= pos, fp <= neg"""
    c = np.frombuffer(L0["roc_sweep"], np.int64).reshape(1, 1, 1, 4)[0, 0, 0]
    x = detect_inputs(W, H)
    assert c[0] == int((x["gt"][1] > 127).sum()) and c[0] + c[1] == W * H and 0 <= c[2] <= c[0] and 0 <= c[3] <= c[1]


@functools.lru_cache(maxsize=None)
def roc_left(W, H) -> dict:
    """roc_ref on the oracle's phi and magnitude: table words a call writes, and cells whose counts are not zero"""
    import roc_cases
    import roc_ref
    from mavflow import _lib
    x = detect_inputs(W, H)

    def left(idx, light):
        a, m = _roc_grid(light)
        cells = 0
        for b in idx:
            phi, mag = roc_cases.oracle_fields(x["flow"][b], "derotate", x["foe"][b], x["omega"][b], float(x["dt"][b]))
            c = roc_ref.ref_counts(phi, mag, x["sky"][b] != 0, x["gt"][b].astype(np.int64), a, m)
            cells += int((c[..., 2:].sum(axis=-1) > 0).sum())
        return dict(batch=len(idx), grid=(len(a), len(m)), words=len(idx) * _lib.roc_table_words(len(a), len(m)), cells=cells)
    return dict(heavy=left([0, 1, 2], False), light=left([1], True))


def roc_leaves_more() -> bool:
    v = roc_left(*FRAME)
    h, l = v["heavy"], v["light"]
    return h["grid"] == (64, 16) and l["grid"] == (1, 1) and h["words"] > 1000 * l["words"] and h["cells"] > 100 * max(l["cells"], 1) and l["words"] == 4


def roc_batched(ctx, items):
    x = detect_inputs(ctx.W, ctx.H)
    idx = [1 if it == "light" else 2 * (i % 2) for i, it in enumerate(items)]
    a, m = _roc_grid(False)
    got = ctx.roc_sweep(x["flow"][idx], x["foe"][idx], x["gt"][idx], a, m, omega=x["omega"][idx], dt=x["dt"][idx], sky=x["sky"][idx])["counts"]
    return [by(got[i]) for i in range(len(items))]


# ---- family: png ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def png_images(W, H):
    noise = np.random.default_rng(424242).integers(0, 256, (B, H, W, 4), dtype=np.uint8)      # BGRA noise: incompressible
    flat = np.full((1, H, W), 128, np.uint8)                                                  # one flat gray image: all runs
    noise.setflags(write=False), flat.setflags(write=False)
    return noise, flat


def _png_dev(ctx, imgs, ch):
    from mavflow import _lib
    n = imgs.shape[0]
    bound = ctx.lib.mav_png_bound(ctx.W, ctx.H, ch) * n
    with Dev(ctx) as d:
        o, idx = d.out(bound), d.out(16 * n)
        _lib.check(ctx.lib.mav_png_encode_dev(ctx.h, vp(d.inp(imgs)), n, ch, vp(o), C.c_size_t(bound), vp(idx)))
        index, stream = d.get(idx, np.uint64, (n, 2)), d.raw(o)
        used = np.zeros(bound, bool)
        for off, ln in index:
            used[int(off):int(off) + int(ln)] = True
        assert (stream[~used] == CANARY).all(), "mav_png_encode_dev wrote outside the streams its index names"
        return tuple(by(stream[int(off):int(off) + int(ln)]) for off, ln in index)


def png_heavy(ctx, st):
    noise, _ = png_images(ctx.W, ctx.H)
    ctx.png_encode(noise)
    _png_dev(ctx, noise, 4)
    x = detect_inputs(ctx.W, ctx.H)
    ctx.detect(x["flow"], x["samples"], omega=x["omega"], dt=x["dt"], sky=x["sky"], foe_params=x["fp"], thr_params=x["tp"])
    ctx.render_last_png(B)
    ctx.overlay_last_png(x["bgr"], x["foe"])


def png_light(ctx, st):
    _, flat = png_images(ctx.W, ctx.H)
    x = detect_inputs(ctx.W, ctx.H)
    out = {"png_encode": tuple(ctx.png_encode(flat)), "png_encode_dev": _png_dev(ctx, flat[..., None], 1)}
    ctx.detect(x["l_flow"], x["l_samples"], foe_params=x["l_fp"], thr_params=x["l_tp"])
    out["render_last_png"] = tuple(f for v in ctx.render_last_png(1, images=("result",)).values() for f in v)
    files, wr = ctx.overlay_last_png(x["l_bgr"], [(5.0, 6.0)])
    out["overlay_last_png"] = (tuple(files), by(wr))
    return out


def png_restate(L0, W, H):
    import png_device_model as model
    from mavflow.frame_source import png_wrap
    _, flat = png_images(W, H)
    z = model.stream_of_image(flat[0])
    assert L0["png_encode_dev"] == (z,) and L0["png_encode"] == (png_wrap(W, H, 1, z),)
    black = model.stream_of_image(np.zeros((H, W, 3), np.uint8))                 # the result image of an empty mask
    assert L0["render_last_png"] == (png_wrap(W, H, 3, black),)


@functools.lru_cache(maxsize=None)
def png_left(W, H):
    import png_device_model as model
    noise, flat = png_images(W, H)
    zs = [model.stream_info(model.scanlines(noise[b])) for b in range(B)]
    zl = model.stream_info(model.scanlines(flat[0]))
    return dict(heavy=dict(segments=min(len(i) for _, i in zs), bytes=min(len(z) for z, _ in zs), stored=all(s["stored"] for _, i in zs for s in i)),
                light=dict(segments=len(zl[1]), bytes=len(zl[0]), stored=any(s["stored"] for s in zl[1])))


def png_leaves_more() -> bool:
    v = png_left(*FRAME)
    h, l = v["heavy"], v["light"]
    # two full segment slots of stored bytes against one coded segment that fills less than a 64th of its slot
    return h["segments"] == 2 and l["segments"] == 1 and h["bytes"] > model_seg() > 64 * l["bytes"] and h["stored"] and not l["stored"]


def model_seg() -> int:
    import png_device_model as model
    return model.SEG


def png_batched(ctx, items):
    noise, flat = png_images(ctx.W, ctx.H)
    imgs = np.stack([np.repeat(flat[0][..., None], 4, axis=2) if it == "light" else noise[i] for i, it in enumerate(items)])
    return list(ctx.png_encode(imgs))


# ---- family: good_features --------------------------------------------------------------------------------------------------------------
GFTT_HEAVY = (("noise", dict(quality_level=0.001, min_distance=1.0, block_size=1, max_corners=4000)),
              ("checker", dict(quality_level=0.001, min_distance=1.0, block_size=3, max_corners=4000)))
GFTT_LIGHT = ("corner", "flat")
GFTT_LIGHT_KW = dict(quality_level=0.2, min_distance=7.0, block_size=7, max_corners=50)


def _gftt(ctx, img, mask, harris, kw, dev):
    n = kw["max_corners"]
    if not dev:
        return by(ctx.good_features(img, mask=mask, useHarrisDetector=harris, **kw))
    with Dev(ctx) as d:
        corners, count = d.out(8 * n), d.out(4)
        ctx.good_features_enqueue(d.inp(img), corners, count, mask_ptr=None if mask is None else d.inp(mask), useHarrisDetector=harris, **kw)
        k = int(d.get(count, np.int32, (1,))[0])
        pts = d.raw(corners)
        assert (pts[8 * max(k, 0):] == CANARY).all(), "good_features wrote past the corners it counts"
        return (k, by(pts[:8 * max(k, 0)]))


def good_features_heavy(ctx, st):
    import sparse_cases as sc
    for kind, kw in GFTT_HEAVY:
        img = sc.image(kind, ctx.W, ctx.H)
        for harris in (False, True):
            _gftt(ctx, img, None, harris, kw, False)
            _gftt(ctx, img, None, harris, kw, True)
    with Dev(ctx) as d:
        ctx.good_features_dev(d.inp(sc.image("checker", ctx.W, ctx.H)), **GFTT_HEAVY[1][1])


def good_features_light(ctx, st):
    import sparse_cases as sc
    out = {}
    mask = sc.mask_of(ctx.W, ctx.H)
    for kind in GFTT_LIGHT:
        img = sc.image(kind, ctx.W, ctx.H)
        for m in (None, mask):
            for harris in (False, True):
                tag = f"{kind}{' mask' if m is not None else ''}{' harris' if harris else ''}"
                out[tag] = _gftt(ctx, img, m, harris, GFTT_LIGHT_KW, False)
                out[tag + " dev"] = _gftt(ctx, img, m, harris, GFTT_LIGHT_KW, True)
                out[tag + " pick"] = ctx.gftt_last_pick()
    with Dev(ctx) as d:
        out["good_features_dev"] = by(ctx.good_features_dev(d.inp(sc.image("corner", ctx.W, ctx.H)), **GFTT_LIGHT_KW))
    return out


def good_features_restate(L0, W, H):
    import gftt_pick_model as gm
    import sparse_cases as sc
    mask = sc.mask_of(W, H)
    for kind in GFTT_LIGHT:
        for m, tag in ((None, kind), (mask, kind + " mask")):
            ref = gm.good_features_masked(sc.image(kind, W, H), m, GFTT_LIGHT_KW["max_corners"], GFTT_LIGHT_KW["quality_level"],
                                          GFTT_LIGHT_KW["min_distance"], GFTT_LIGHT_KW["block_size"])
            assert L0[tag] == by(ref), tag
            assert L0[tag + " dev"] == (len(ref), by(ref)), tag


@functools.lru_cache(maxsize=None)
def gftt_left(W, H):
    import gftt_pick_model as gm
    import lk_ref
    import sparse_cases as sc
    out = {}
    for kind, kw in GFTT_HEAVY + tuple((k, GFTT_LIGHT_KW) for k in GFTT_LIGHT):
        v, idx = gm.masked_candidates(lk_ref.min_eigen(sc.image(kind, W, H), kw["block_size"]), None, kw["quality_level"])
        stats = dict(chunks=0)
        if len(v):
            _, stats = gm.good_features_from_keys(gm.keys_of(v, idx), W, H, kw["max_corners"], kw["min_distance"], want_stats=True)
        out[kind] = (len(v), stats["chunks"])
    return out


def good_features_leaves_more() -> bool:
    """iid noise has a strict 3 x 3 maximum at one interior pixel in nine: 931 of 131 x 67, short of a pick chunk -- the noise frame is
    the many-values case, sparse_cases' checkerboard (equal values side by side) the one that passes the chunk"""
    import gftt_pick_model as gm
    v = gftt_left(*FRAME)
    heavy, light = max(v[k][0] for k, _ in GFTT_HEAVY), max(v[k][0] for k in GFTT_LIGHT)
    return heavy > gm.CHUNK > v["noise"][0] > 50 * max(light, 1) and max(v[k][1] for k, _ in GFTT_HEAVY) >= 2 and v["flat"][0] == 0 and 1 <= v["corner"][0] <= 8


# ---- family: lk -------------------------------------------------------------------------------------------------------------------------------
LK_HEAVY_POINTS = 2000
LK_FLAGS = 4 | 8                         # OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_LK_GET_MIN_EIGENVALS


@functools.lru_cache(maxsize=None)
def lk_inputs(W, H):
    import sparse_cases as sc
    a, b = sc.image("blurred", W, H), sc.image("blurred-moved", W, H)
    c = np.ascontiguousarray(np.roll(b, (1, -1), axis=(0, 1)))
    pts = sc.inside_points(W, H, LK_HEAVY_POINTS)
    one = np.array([[W * 0.5 + 0.25, H * 0.5 - 0.5]], np.float32)
    return dict(a=a, b=b, c=c, pts=pts, init=(pts + np.float32(0.75)).astype(np.float32), one=one)


def lk_heavy(ctx, st):
    x = lk_inputs(ctx.W, ctx.H)
    n = LK_HEAVY_POINTS
    ctx.lk_track_err(x["c"], x["a"], x["pts"], next_pts=x["init"], flags=LK_FLAGS)
    with Dev(ctx) as d:
        o, s, e = d.out(8 * n), d.out(n), d.out(4 * n)
        ctx.lk_track_err_enqueue(d.inp(x["c"]), d.inp(x["a"]), d.inp(x["pts"]), n, d.inp(np.array([n], np.int32)), o, s, e, flags=8)
        ctx.lk_track_dev(d.inp(x["a"]), d.inp(x["c"]), d.inp(x["pts"]), n, o, s)
        ctx.sync()
    ctx.lk_track(x["b"], x["c"], x["pts"])


def lk_light(ctx, st):
    x = lk_inputs(ctx.W, ctx.H)
    out = {}
    o, s = ctx.lk_track(x["a"], x["b"], x["one"])
    out["lk_track"] = (by(o), by(s), by(ctx.lk_last_iterations()))
    o, s = ctx.lk_track(None, x["c"], x["one"])                 # prev=None: b's pyramid, resident since the call above
    out["lk_track prev=None"] = (by(o), by(s), by(ctx.lk_last_iterations()))
    o, s, e = ctx.lk_track_err(x["a"], x["b"], x["one"])
    out["lk_track_err"] = (by(o), by(s), by(e), by(ctx.lk_last_iterations()))
    with Dev(ctx) as d:
        po, ps, pe = d.out(8), d.out(1), d.out(4)
        da, db, dp = d.inp(x["a"]), d.inp(x["b"]), d.inp(x["one"])
        ctx.lk_track_dev(da, db, dp, 1, po, ps)
        out["lk_track_dev"] = (by(d.raw(po)), by(d.raw(ps)))
        po, ps = d.out(8 * 4), d.out(4)                          # sized for 4 points, the count on the device says 1
        four = np.concatenate([x["one"], np.full((3, 2), 9.5, np.float32)])
        ctx.lk_track_enqueue(da, db, d.inp(four), 4, d.inp(np.array([1], np.int32)), po, ps)
        out["lk_track_ex_dev"] = (by(d.raw(po)[:8]), by(d.raw(ps)[:1]))
        assert (d.raw(po)[8:] == CANARY).all() and (d.raw(ps)[1:] == CANARY).all()
        po, ps = d.out(8), d.out(1)
        ctx.lk_track_err_enqueue(da, db, dp, 1, None, po, ps, pe)
        out["lk_track_err_dev"] = (by(d.raw(po)), by(d.raw(ps)), by(d.raw(pe)))
    assert out["lk_track_dev"] == out["lk_track"][:2] and out["lk_track_ex_dev"] == out["lk_track"][:2]
    assert out["lk_track_err_dev"] == out["lk_track_err"][:3]
    return out


def lk_restate(L0, W, H):
    import lk_err_ref as er
    x = lk_inputs(W, H)
    res = er.lk_track_err(x["a"], x["b"], x["one"])
    assert L0["lk_track_err"][:3] == (by(np.asarray(res[0], np.float32)), by(np.asarray(res[1], np.uint8)), by(np.asarray(res[2], np.float32)))
    res = er.lk_track_err(x["b"], x["c"], x["one"], want_err=False)
    assert L0["lk_track prev=None"][0] == by(np.asarray(res[0], np.float32))


@functools.lru_cache(maxsize=None)
def lk_left(W, H) -> dict:
    """lk_err_ref on both calls: points, points still tracked, entries of the iteration histogram, non-zero err values"""
    import lk_err_ref as er
    x = lk_inputs(W, H)
    h = er.lk_track_err(x["c"], x["a"], x["pts"], x["init"], flags=LK_FLAGS)
    l = er.lk_track_err(x["a"], x["b"], x["one"])
    return {k: dict(points=len(r[0]), tracked=int(np.asarray(r[1]).sum()), iterations=int(np.asarray(r[3]).sum()), errs=int((np.asarray(r[2]) != 0).sum()))
            for k, r in (("heavy", h), ("light", l))}


def lk_leaves_more() -> bool:
    v = lk_left(*FRAME)
    h, l = v["heavy"], v["light"]
    return all(h[k] > 100 * max(l[k], 1) for k in h) and h["points"] == LK_HEAVY_POINTS and l["points"] == 1


# ---- family: gt_stats ---------------------------------------------------------------------------------------------------------------------
GTS_MAX_PIXELS = 512


@functools.lru_cache(maxsize=None)
def gts_inputs(W, H):
    rng = np.random.default_rng(6713)
    seg = rng.integers(0, 12, (B, H, W)).astype(np.uint8)
    for b in range(B):
        seg[b, H // 6:H - H // 6, W // 5:W - W // 5] = rng.integers(128, 256, (H - 2 * (H // 6), W - 2 * (W // 5))).astype(np.uint8)
    seg[:, H // 2, W // 2] = 255
    gt = rng.normal(0, 3, (B, H, W, 2)).astype(np.float32)
    depth = rng.uniform(1, 99, (B, H, W)).astype(np.float32)
    depth[:, H // 2, W // 2] = 100.0
    sky = ((depth > 80) ^ (rng.random((B, H, W)) < 0.1)).astype(np.uint8) * rng.integers(1, 256, (B, H, W)).astype(np.uint8)
    empty = rng.integers(0, 12, (1, H, W)).astype(np.uint8)      # seg_max 11: no MAV, a box of its own (pixels above 1.1)
    one = np.zeros((1, H, W), np.uint8)
    one[0, H - 2, W - 3] = 200                                    # a one-pixel MAV whose maximum is below the heavy call's 255
    v = dict(seg=seg, gt=gt, depth=depth, sky=sky, omega=rng.normal(0, 0.3, (B, 3)), dt=1 / 30.0 + 0.001 * np.arange(B), empty=empty, one=one)
    for a in v.values():
        a.setflags(write=False)
    return v


def _gts_dev(ctx, seg, gt, sky, depth, omega, dt, want_idx=True):
    from mavflow import _validation as V
    n = seg.shape[0]
    with Dev(ctx) as d:
        rec = d.out(96 * n)
        idx = d.out(4 * GTS_MAX_PIXELS * n) if want_idx else None
        par = V.gt_stats_params(omega, dt, batch=n)
        ctx.gt_stats_enqueue(d.inp(seg), d.inp(gt), None if sky is None else d.inp(sky), None if depth is None else d.inp(depth), d.inp(par), n,
                             GTS_MAX_PIXELS, rec, idx)
        r = d.get(rec, V.RECORD_DTYPE, (n,))
        if not want_idx:
            return (by(r),)
        i = d.get(idx, np.int32, (n, GTS_MAX_PIXELS))
        for b in range(n):                                        # (k_gts_list puts -1 into the entries behind the list: the whole row is the call's)
            assert (i[b, r["listed"][b]:] == -1).all(), "mav_gt_stats_dev: the entries behind the list are not -1"
        return (by(r),) + tuple(by(i[b, :r["listed"][b]]) for b in range(n))


def gt_stats_heavy(ctx, st):
    x = gts_inputs(ctx.W, ctx.H)
    ctx.gt_stats(x["seg"], x["gt"], x["sky"], x["depth"], omega=x["omega"], dt=x["dt"], max_pixels=GTS_MAX_PIXELS)
    _gts_dev(ctx, x["seg"], x["gt"], x["sky"], x["depth"], x["omega"], x["dt"])
    _gts_dev(ctx, x["seg"], x["gt"], x["sky"], x["depth"], x["omega"], x["dt"], want_idx=False)      # the list of the call's own, in gts_scratch


def gt_stats_light(ctx, st):
    x = gts_inputs(ctx.W, ctx.H)
    out = {}
    for name in ("empty", "one"):
        got = ctx.gt_stats(x[name], x["gt"][:1], None, None, omega=x["omega"][:1], dt=x["dt"][:1], max_pixels=GTS_MAX_PIXELS)
        out[name] = (by(got["records"]),) + tuple(by(i) for i in got["indices"])
        out[name + " dev"] = _gts_dev(ctx, x[name], x["gt"][:1], None, None, x["omega"][:1], x["dt"][:1])
        out[name + " dev own list"] = _gts_dev(ctx, x[name], x["gt"][:1], None, None, x["omega"][:1], x["dt"][:1], want_idx=False)
    return out


def gt_stats_restate(L0, W, H):
    import validation_ref as R
    x = gts_inputs(W, H)
    for name in ("empty", "one"):
        rec, idx = R.gt_stats_batch(x[name], x["gt"][:1], None, None, x["omega"][:1], x["dt"][:1], None, GTS_MAX_PIXELS)
        want = (by(rec), by(idx[0, :rec["listed"][0]]))
        assert L0[name] == want and L0[name + " dev"] == want and L0[name + " dev own list"] == want[:1], name


def gt_stats_leaves_more() -> bool:
    import validation_ref as R
    x = gts_inputs(*FRAME)
    rec, _ = R.gt_stats_batch(x["seg"], x["gt"], x["sky"], x["depth"], x["omega"], x["dt"], None, GTS_MAX_PIXELS)
    le, _ = R.gt_stats_batch(x["empty"], x["gt"][:1], None, None, x["omega"][:1], x["dt"][:1], None, GTS_MAX_PIXELS)
    lo, _ = R.gt_stats_batch(x["one"], x["gt"][:1], None, None, x["omega"][:1], x["dt"][:1], None, GTS_MAX_PIXELS)
    return (bool((rec["drone_pixels"] > GTS_MAX_PIXELS).all()) and bool((rec["flags"] & R.TRUNCATED).all()) and le["drone_pixels"][0] == 0
            and lo["drone_pixels"][0] == 1 and int(rec["seg_max"].min()) == 255 > int(lo["seg_max"][0]) > int(le["seg_max"][0]) > 0
            and float(rec["depth_max"].min()) > 0.0 == float(le["depth_max"][0]) and int(rec["sky"].sum()) > 0 == int(le["sky"].sum()))


def gt_stats_batched(ctx, items):
    x = gts_inputs(ctx.W, ctx.H)
    seg = np.stack([x["one"][0] if it == "light" else x["seg"][i] for i, it in enumerate(items)])
    n = len(items)
    got = ctx.gt_stats(seg, np.stack([x["gt"][0]] * n), None, None, omega=np.stack([x["omega"][0]] * n), dt=np.stack([x["dt"][0]] * n),
                       max_pixels=GTS_MAX_PIXELS)
    return [(by(got["records"][i]), by(got["indices"][i])) for i in range(n)]


# ---- family: radial ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def radial_inputs(W, H):
    import truth_cases as tc
    em, ee = tc.EDGE_SETS["default"]                                                     # 160 x 160 edges
    flow, gt, sky = tc.scene(8123, W, H, B, em, ee)
    lm, le = tc.EDGE_SETS["3 edges"]
    one_f = np.broadcast_to(np.array(tc.ONE_CELL_FLOW, np.float32), (1, H, W, 2)).copy()
    one_g = np.broadcast_to(np.array(tc.ONE_CELL_GT, np.float32), (1, H, W, 2)).copy()
    one_s = (np.random.default_rng(9).random((1, H, W)) < 0.15).astype(np.uint8)
    return dict(flow=flow, gt=gt, sky=sky.astype(np.uint8), em=em, ee=ee, lm=lm, le=le, one_f=one_f, one_g=one_g, one_s=one_s)


def _acc(ctx, st, x):
    if "radial_acc" not in st:
        st["radial_acc"] = ctx.radial_error_accumulator(x["lm"], x["le"])
    return st["radial_acc"]


def radial_heavy(ctx, st):
    x = radial_inputs(ctx.W, ctx.H)
    ctx.radial_error_hist(x["flow"], x["gt"], x["sky"], x["em"], x["ee"])
    acc = _acc(ctx, st, x)
    big = ctx.radial_error_accumulator(x["em"], x["ee"])
    big.add(x["flow"], x["gt"], x["sky"])
    big.add(x["flow"], x["gt"], x["sky"])
    big.counts()
    big.close()
    acc.add(x["flow"], x["gt"], x["sky"])                        # the family's own accumulator holds the heavy scene's counts ...
    acc.reset()                                                  # ... until it is reset


def _hist(h):
    return (by(h["counts"]), h["non_sky"], h["in_range"])


def radial_light(ctx, st):
    x = radial_inputs(ctx.W, ctx.H)
    out = {"radial_error_hist": _hist(ctx.radial_error_hist(x["one_f"], x["one_g"], x["one_s"], x["lm"], x["le"]))}
    acc = _acc(ctx, st, x)
    acc.add(x["one_f"], x["one_g"], x["one_s"])
    out["one add"] = _hist(acc.counts())
    acc.add(x["one_f"], x["one_g"], None)
    out["two adds"] = _hist(acc.counts())
    acc.reset()
    out["after reset"] = _hist(acc.counts())
    return out


def radial_restate(L0, W, H):
    import truth_ref as R
    x = radial_inputs(W, H)
    h = R.radial_hist(x["one_f"], x["one_g"], x["one_s"], x["lm"], x["le"])
    h2 = R.radial_hist(x["one_f"], x["one_g"], None, x["lm"], x["le"])
    assert L0["radial_error_hist"] == L0["one add"] == _hist(h)
    assert L0["two adds"] == (by(h["counts"] + h2["counts"]), h["non_sky"] + h2["non_sky"], h["in_range"] + h2["in_range"])
    assert L0["after reset"] == (by(np.zeros_like(h["counts"])), 0, 0)


def radial_leaves_more() -> bool:
    import truth_ref as R
    x = radial_inputs(*FRAME)
    h = R.radial_hist(x["flow"], x["gt"], x["sky"], x["em"], x["ee"])
    l = R.radial_hist(x["one_f"], x["one_g"], x["one_s"], x["lm"], x["le"])
    return (len(x["em"]), len(x["ee"])) == (160, 160) and (len(x["lm"]), len(x["le"])) == (3, 3) and int((h["counts"] > 0).sum()) > 1000 \
        and int((l["counts"] > 0).sum()) == 1


# ---- family: history ------------------------------------------------------------------------------------------------------------------------
HIST_L, HIST_LIGHT_PUSHES = 4, 5


def _ring(ctx, st):
    if "ring" not in st:
        st["ring"] = ctx.flow_history(HIST_L)
    return st["ring"]


def history_heavy(ctx, st):
    import history_cases as hc
    r = _ring(ctx, st)
    for i in range(2 * HIST_L + 1):                              # NaN and infinities into every slot, twice round the ring and one more
        r.push(hc.planted(ctx.W, ctx.H, "reference") if i % 2 == 0 else hc.sampled(ctx.W, ctx.H, 10 * i + ctx.W))
    with Dev(ctx) as d:
        r.push_enqueue(d.inp(np.stack([hc.sampled(ctx.W, ctx.H, 7 + b) for b in range(B)])), d.out(16 * ctx.W * ctx.H * B), B)
    r.reset()


def history_light(ctx, st):
    import history_cases as hc
    W, H = ctx.W, ctx.H
    r1, r2 = _ring(ctx, st), ctx.flow_history(HIST_L, np.float64, "xy")
    out = {"index before": r1.index}
    a, b = [], []
    for i in range(HIST_LIGHT_PUSHES):
        a.append(by(r1.push(hc.smooth(W, H, i))))
        b.append(by(r2.push(hc.smooth(W, H, 20 + i).astype(np.float64), out="flow")))
    with Dev(ctx) as d:                                           # one more field through the device form, on the caller's blocks
        o = d.out(16 * W * H)
        r1.push_enqueue(d.inp(hc.smooth(W, H, HIST_LIGHT_PUSHES)), o, 1)
        a.append(by(d.raw(o)))
    out.update(ring=tuple(a), second_ring=tuple(b), index=(r1.index, r1.pushes >= HIST_LIGHT_PUSHES + 1, r2.index))
    r2.close()
    r1.reset()                                                    # the family's ring is handed on empty
    return out


def history_restate(L0, W, H):
    import history_cases as hc
    import history_ref as R
    ref1, ref2 = R.HistoryRef(H, W, HIST_L, np.float32, "reference"), R.HistoryRef(H, W, HIST_L, np.float64, "xy")
    a = tuple(by(ref1.get_history(hc.smooth(W, H, i))) for i in range(HIST_LIGHT_PUSHES + 1))
    b = tuple(by(ref2.get_history(hc.smooth(W, H, 20 + i).astype(np.float64), "flow")) for i in range(HIST_LIGHT_PUSHES))
    assert L0["ring"] == a and L0["second_ring"] == b and L0["index before"] == 0


def history_leaves_more() -> bool:
    """history_ref through the heavy pushes: when they end every slot of the ring holds a NaN or an infinity, and the last output carries
    them on; the light fields are finite, and so is everything history_ref makes of them on a fresh ring"""
    import history_cases as hc
    import history_ref as R
    W, H = FRAME
    ref = R.HistoryRef(H, W, HIST_L, np.float32, "reference")
    for i in range(2 * HIST_L + 1):
        out = ref.get_history(hc.planted(W, H, "reference") if i % 2 == 0 else hc.sampled(W, H, 10 * i + W))
    dirty = [int((~np.isfinite(ref.flow_uv_history[k])).sum()) for k in range(HIST_L)]
    fresh = R.HistoryRef(H, W, HIST_L, np.float32, "reference")
    clean = all(np.isfinite(fresh.get_history(hc.smooth(W, H, i))).all() for i in range(HIST_LIGHT_PUSHES + 1))
    return min(dirty) > 0 and int((~np.isfinite(out)).sum()) > 0 and ref.history_index != 0 and clean


# ---- family: global_motion ------------------------------------------------------------------------------------------------------------------
GM_HEAVY_PAIRS, GM_LIGHT_PAIRS = 1000, 4


@functools.lru_cache(maxsize=None)
def gm_inputs(W, H):
    import global_motion_cases as gc
    rng = np.random.default_rng(901)
    cases = {n: (s, d) for n, s, d, _ in gc.fit_cases()}
    coords = np.stack([rng.integers(0, W, GM_HEAVY_PAIRS), rng.integers(0, H, GM_HEAVY_PAIRS)], 1).astype(np.int32)
    few = np.array([[3, 4], [W - 5, 6], [W - 7, H - 4], [5, H - 6]], np.int32)
    M = np.array(rc.inputs()["M"])
    return dict(flow=np.array(dc.noise_fields(W, H)), coords=coords, few=few, M=M, src=np.stack([cases["noisy1000"][0]] * B),
                dst=np.stack([cases["noisy1000"][1], cases["noisy1000"][1] + 0.5, cases["noisy1000"][1] - 0.25]), src4=cases["exact4"][0][None],
                dst4=cases["exact4"][1][None], prev=frames_u8(W, H)[:-1], next=frames_u8(W, H)[1:], l_prev=frames_u8(W, H, 2, first=11)[:1],
                l_next=frames_u8(W, H, 2, first=11)[1:])


def _gm(ctx, light):
    from mavflow import _lib
    x, W, H = gm_inputs(ctx.W, ctx.H), ctx.W, ctx.H
    n, opt = (1, False) if light else (B, True)
    sl = slice(1, 2) if light else slice(0, B)
    flow, M, coords = x["flow"][sl], x["M"][sl], x["few"] if light else x["coords"]
    src, dst = (x["src4"], x["dst4"]) if light else (x["src"], x["dst"])
    prev, nxt = (x["l_prev"], x["l_next"]) if light else (x["prev"], x["next"])
    out = {}
    Hm, ok = ctx.find_homography(src, dst)
    out["find_homography"] = (by(Hm), by(ok))
    Hm, ok = ctx.flow_homography(flow, coords)
    out["flow_homography"] = (by(Hm), by(ok))
    got = ctx.global_motion(flow, M, optimize=opt, outputs=() if light else ("warped", "mag", "gray"))
    out["global_motion"] = tuple(by(got[k]) for k in sorted(got))
    got = ctx.global_motion_batch(prev, nxt, coords, optimize=opt, outputs=() if light else ("flow", "gray"))
    out["global_motion_batch"] = tuple(by(got[k]) for k in sorted(got))
    out["render_last_global_motion"] = tuple(by(v) for v in ctx.render_last_global_motion(n).values())
    with Dev(ctx) as d:
        dflow, Hd, okd, res = d.inp(flow), d.out(72 * n), d.out(4 * n), d.out(88 * n)
        _lib.check(ctx.lib.mav_find_homography_dev(ctx.h, vp(d.inp(src)), vp(d.inp(dst)), src.shape[1], n, vp(Hd), vp(okd)))
        out["find_homography_dev"] = (by(d.raw(Hd)), by(d.raw(okd)))
        Hd, okd = d.out(72 * n), d.out(4 * n)
        _lib.check(ctx.lib.mav_flow_homography_dev(ctx.h, vp(dflow), p_(coords), len(coords), n, vp(Hd), vp(okd)))
        out["flow_homography_dev"] = (by(d.raw(Hd)), by(d.raw(okd)))
        _lib.check(ctx.lib.mav_global_motion_dev(ctx.h, vp(dflow), vp(d.inp(np.ascontiguousarray(M))), n, C.c_double(1.5), int(opt), None, None, None, vp(res)))
        out["global_motion_dev"] = by(d.raw(res))
        Hd, okd, res = d.out(72 * n), d.out(4 * n), d.out(88 * n)
        ctx.global_motion_step(dflow, coords, n, res, optimize=opt, H_ptr=Hd, ok_ptr=okd)
        out["global_motion_step_dev"] = (by(d.raw(Hd)), by(d.raw(okd)), by(d.raw(res)))
        Hd, okd, res, fl = d.out(72 * n), d.out(4 * n), d.out(88 * n), d.out(8 * W * H * n)
        ctx.global_motion_batch_dev(d.inp(prev), d.inp(nxt), coords, n, res, optimize=opt, flow_ptr=fl, H_ptr=Hd, ok_ptr=okd)
        out["global_motion_batch_dev"] = (by(d.raw(Hd)), by(d.raw(okd)), by(d.raw(res)), by(d.raw(fl)))
    return out


def global_motion_heavy(ctx, st):
    _gm(ctx, False)


def global_motion_light(ctx, st):
    out = _gm(ctx, True)
    assert out["find_homography_dev"] == out["find_homography"] and out["flow_homography_dev"] == out["flow_homography"]
    return out


def global_motion_restate(L0, W, H):
    import global_motion_ref as R
    x = gm_inputs(W, H)
    He, oke = R.find_homography(x["src4"][0], x["dst4"][0])
    assert L0["find_homography"] == (by(He[None]), by(np.array([oke], np.int32))) and oke == 1
    He, oke = R.find_homography(x["few"].astype(np.float64), R.coords_new(x["few"], x["flow"][1]))
    assert L0["flow_homography"] == (by(He[None]), by(np.array([oke], np.int32)))


@functools.lru_cache(maxsize=None)
def gm_left(W, H) -> dict:
    """global_motion_ref and the pyramid oracle on both calls: pairs gathered, iterations of the fit's refinement, non-zero pixels of the
    normalised images the window search reads, pyramid pixels it builds, the optimised window's score (0 where optimize is off)"""
    import global_motion_ref as R
    from oracle import pyramid_oracle as po
    x = gm_inputs(W, H)

    def left(idx, coords, src, dst, optimize):
        pairs = steps = gray = score = 0
        for i, b in enumerate(idx):
            pairs += len(R.coords_new(coords, x["flow"][b]))
            hist = []
            R.find_homography(src[i], dst[i], hist)
            steps += len(hist)
            g = R.subtract(x["flow"][b], x["M"][b])["gray"]
            gray += int((g != 0).sum())
            if optimize:
                best = po.analyze_pyramid(g)
                score += int(po.optimize_window(g, (int(best[1]), int(best[2]), po.WIN, po.WIN))[0])
        return dict(batch=len(idx), pairs=pairs, fit_pairs=sum(len(a) for a in src), steps=steps, gray=gray, score=score)
    return dict(heavy=left([0, 1, 2], x["coords"], x["src"], x["dst"], True), light=left([1], x["few"], x["src4"], x["dst4"], False))


def global_motion_leaves_more() -> bool:
    v = gm_left(*FRAME)
    h, l = v["heavy"], v["light"]
    return all(h[k] > l[k] for k in h if k != "steps") and h["steps"] >= l["steps"] and l["score"] == 0 and h["pairs"] == B * GM_HEAVY_PAIRS \
        and l["pairs"] == GM_LIGHT_PAIRS


def global_motion_refused(ctx, st):
    x = gm_inputs(ctx.W, ctx.H)
    outside = x["coords"].copy()
    outside[5] = (ctx.W, 3)
    assert rc.code(ctx.global_motion_batch, x["prev"], x["next"], outside) == rc.ERR_ARG
    assert rc.code(ctx.flow_homography, x["flow"], x["coords"][:3]) == rc.ERR_ARG
    assert rc.code(ctx.find_homography, x["src"][:, :3], x["dst"][:, :3]) == rc.ERR_ARG
    assert rc.code(ctx.global_motion, x["flow"], x["M"], scale=1.0) == rc.ERR_ARG


def global_motion_batched(ctx, items):
    x = gm_inputs(ctx.W, ctx.H)
    idx = [1 if it == "light" else 2 * (i % 2) for i, it in enumerate(items)]
    got = ctx.global_motion(x["flow"][idx], x["M"][idx], optimize=True, outputs=("warped", "mag", "gray"))
    Hm, ok = ctx.flow_homography(x["flow"][idx], x["few"])
    return [tuple(by(got[k][i]) for k in sorted(got)) + (by(Hm[i]), by(ok[i])) for i in range(len(items))]


# ---- family: pyramid ------------------------------------------------------------------------------------------------------------------------
PYR_HEAVY_SCALE, PYR_LIGHT_SCALE = 1.5, 3.0


@functools.lru_cache(maxsize=None)
def pyr_inputs(W, H):
    import window_cases as wc
    heavy = np.stack([wc.image(k, W, H) for k in ("noise", "uniform", "band")])
    win = np.array([wc.start_windows(W, H)[k] for k in ("inside", "clip-right-bottom", "middle")], np.int32)
    return dict(heavy=heavy, win=win, light=wc.image("right", W, H)[None], zero=wc.image("zero", W, H)[None],
                l_win=np.array([wc.start_windows(W, H)["inside"]], np.int32))


def pyramid_heavy(ctx, st):
    x = pyr_inputs(ctx.W, ctx.H)
    ctx.analyze_pyramid(x["heavy"], PYR_HEAVY_SCALE)
    ctx.window_max(x["heavy"])
    ctx.optimize_window(x["heavy"], x["win"])


def pyramid_light(ctx, st):
    x = pyr_inputs(ctx.W, ctx.H)
    out = {"analyze_pyramid": by(ctx.analyze_pyramid(x["light"], PYR_LIGHT_SCALE)), "analyze_pyramid zero": by(ctx.analyze_pyramid(x["zero"], PYR_LIGHT_SCALE)),
           "window_max zero": by(ctx.window_max(x["zero"])), "window_max": by(ctx.window_max(x["light"]))}
    for k in ("zero", "light"):
        s, w = ctx.optimize_window(x[k], x["l_win"])
        out["optimize_window " + k] = (by(s), by(w))
    return out


def pyramid_restate(L0, W, H):
    from oracle import pyramid_oracle as po
    x = pyr_inputs(W, H)
    assert L0["analyze_pyramid"] == by(np.array([po.analyze_pyramid(x["light"][0], PYR_LIGHT_SCALE)], np.int64))
    assert L0["analyze_pyramid zero"] == by(np.zeros((1, 6), np.int64))
    for k in ("zero", "light"):
        s, w = po.optimize_window(x[k][0], tuple(int(v) for v in x["l_win"][0]))
        assert L0["optimize_window " + k] == (by(np.array([s], np.int64)), by(np.array([w], np.int32))), k


def pyramid_leaves_more() -> bool:
    from oracle import pyramid_oracle as po
    W, H = FRAME
    dh, dl = po.pyramid_dims(W, H, PYR_HEAVY_SCALE), po.pyramid_dims(W, H, PYR_LIGHT_SCALE)
    px = lambda dims: sum(w * h for w, h in dims[1:])
    x = pyr_inputs(W, H)
    return len(dh) > len(dl) and B * px(dh) > px(dl) and int(x["heavy"].sum()) > 0 == int(x["zero"].sum())


def pyramid_refused(ctx, st):
    x = pyr_inputs(ctx.W, ctx.H)
    assert rc.code(ctx.analyze_pyramid, x["heavy"], 1.0) == rc.ERR_ARG


def pyramid_batched(ctx, items):
    x = pyr_inputs(ctx.W, ctx.H)
    imgs = np.stack([x["light"][0] if it == "light" else x["heavy"][i] for i, it in enumerate(items)])
    a = ctx.analyze_pyramid(imgs, PYR_HEAVY_SCALE)
    m = ctx.window_max(imgs)
    s, w = ctx.optimize_window(imgs, np.concatenate([x["l_win"]] * len(items)))
    return [(by(a[i]), by(m[i]), by(s[i]), by(w[i])) for i in range(len(items))]


# ---- FAMILIES ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Family:
    name: str
    entries: tuple               # the header's functions whose surviving memory this pair of calls holds (each in exactly one family)
    heavy: object                # heavy(ctx, st)
    light: object                # light(ctx, st) -> {name: comparable}
    leaves_more: object          # () -> bool, on the CPU, at FRAME
    restate: object = None       # restate(L0, W, H): the fresh context's bytes against the numpy restatement
    refused: object = None       # refused(ctx, st): the family's part-way refused forms (REFUSED_FORMS), each asserted refused
    batched: object = None       # batched(ctx, items) -> per batch position the comparable outputs of ONE call; items: "light" | "heavy"


FAMILIES = [
    Family("detect", ("mav_detect", "mav_detect_dev", "mav_process_batch", "mav_process_batch_dev", "mav_frame_step_dev", "mav_frame_step_post",
                      "mav_frame_step_wait", "mav_worker_drain", "mav_worker_wait_enqueued", "mav_last_render", "mav_last_overlay", "mav_last_masks_tpr_fpr",
                      "mav_last_flow_dev"),
           detect_heavy, detect_light, detect_leaves_more, detect_restate, detect_refused, detect_batched),
    # the refusal variant: the part-way refused forms stand in for the heavy call, the light call is the same
    Family("detect refused", (), detect_refused, detect_light, detect_leaves_more, detect_restate),
    Family("parts", ("mav_derotate", "mav_foe_dense", "mav_foe_dense_f32", "mav_ransac", "mav_bgr2gray", "mav_bgr2gray_dev", "mav_phi_mask", "mav_phi_mask_f32",
                     "mav_bbox", "mav_tpr_fpr_counts", "mav_tpr_fpr_counts_dev", "mav_render", "mav_render_dev", "mav_flow_to_color", "mav_colormap_jet",
                     "mav_overlay", "mav_overlay_dev"),
           parts_heavy, parts_light, parts_leaves_more, parts_restate, parts_refused, parts_batched),
    Family("components", ("mav_components", "mav_components_dev", "mav_last_masks_components"),
           components_heavy, components_light, components_leaves_more, components_restate, None, components_batched),
    Family("roc", ("mav_roc_sweep", "mav_roc_sweep_dev", "mav_last_roc_sweep", "mav_roc_arm"), roc_heavy, roc_light, roc_leaves_more, roc_restate, None,
           roc_batched),
    Family("png", ("mav_png_encode", "mav_png_encode_dev", "mav_last_render_png", "mav_last_overlay_png"), png_heavy, png_light, png_leaves_more, png_restate,
           None, png_batched),
    Family("good_features", ("mav_good_features", "mav_good_features_ex", "mav_good_features_score", "mav_good_features_dev", "mav_good_features_ex_dev",
                             "mav_good_features_score_dev", "mav_gftt_last_pick"),
           good_features_heavy, good_features_light, good_features_leaves_more, good_features_restate),
    Family("lk", ("mav_lk_track", "mav_lk_track_err", "mav_lk_track_dev", "mav_lk_track_ex_dev", "mav_lk_track_err_dev", "mav_lk_last_iterations"),
           lk_heavy, lk_light, lk_leaves_more, lk_restate),
    Family("gt_stats", ("mav_gt_stats", "mav_gt_stats_dev"), gt_stats_heavy, gt_stats_light, gt_stats_leaves_more, gt_stats_restate, None,
           gt_stats_batched),
    Family("radial", ("mav_radial_error_hist", "mav_radial_error_hist_dev"), radial_heavy, radial_light, radial_leaves_more, radial_restate),
    Family("history", ("mav_history_create", "mav_history_destroy", "mav_history_reset", "mav_history_info", "mav_history_push", "mav_history_push_dev"),
           history_heavy, history_light, history_leaves_more, history_restate),
    Family("global_motion", ("mav_find_homography", "mav_find_homography_dev", "mav_flow_homography", "mav_flow_homography_dev", "mav_global_motion",
                             "mav_global_motion_dev", "mav_global_motion_step_dev", "mav_global_motion_batch", "mav_global_motion_batch_dev",
                             "mav_last_global_motion_render"),
           global_motion_heavy, global_motion_light, global_motion_leaves_more, global_motion_restate, global_motion_refused, global_motion_batched),
    Family("pyramid", ("mav_analyze_pyramid", "mav_window_max", "mav_optimize_window"), pyramid_heavy, pyramid_light, pyramid_leaves_more, pyramid_restate,
           pyramid_refused, pyramid_batched),
]
BY_NAME = {f.name: f for f in FAMILIES}
NAMES = [f.name for f in FAMILIES]
WITH_REFUSAL = [f.name for f in FAMILIES if f.refused is not None]
WITH_BATCH = [f.name for f in FAMILIES if f.batched is not None]      # (the other families take one frame, one ring or one table per call)
THIRDS = {"a": lambda i: i % 3 == 0, "b": lambda i: i % 3 == 1, "c": lambda i: i % 3 == 2}      # the walk's light calls in three thirds, as resident_cases.GROUPS
# the part-way refused forms a family's `refused` runs, by resident_cases' form names: each must still be there
REFUSED_FORMS = {
    "detect": ("mav_frame_step_dev refused(compute flow, n_pairs=0)", "mav_detect refused(n_pairs=0)", "mav_process_batch refused(n_pairs=0)"),
    "parts": ("mav_foe_dense refused(n_pairs=0)", "mav_tpr_fpr_counts refused(mask_value=0)"),
    "global_motion": ("mav_global_motion_batch refused(sample outside)", "mav_flow_homography refused(n=3)", "mav_find_homography refused(n=3)",
                      "mav_global_motion refused(scale=1)"),
    "pyramid": ("mav_analyze_pyramid refused(scale=1)",),
}

# ---- DEFERRED ---------------------------------------------------------------------------------------------------------------------------------
# The Farneback entry points have no pair of calls here (DESIGN 5 says why).  Their workspace is held by schedule_cases.dirty, and the detect
# and global_motion families run Farneback inside their fused calls.
DEFERRED = {
    "farneback": ("mav_farneback", "mav_farneback_init", "mav_farneback_ex", "mav_farneback_dev", "mav_farneback_init_dev", "mav_farneback_ex_dev"),
}

# ---- EXEMPT -----------------------------------------------------------------------------------------------------------------------------------
EXEMPT = dict(rc.EXEMPT)
EXEMPT.update({
    "mav_gt_stats_defaults": "fills a struct",
    "mav_gt_flow": "every output pixel is a function of its own inputs: staging blocks and the caller's field, no scratch of the context's",
    "mav_gt_flow_dev": "caller-owned memory only",
    "mav_device_count": "a query, no context", "mav_set_option": "host state", "mav_get_option": "host state", "mav_set_window": "host state",
    "mav_get_window": "host state", "mav_schedule_info": "a query", "mav_schedule_info_ex": "a query", "mav_mem_info": "a query",
    "mav_num_layers": "a query", "mav_layer_dims": "a query", "mav_pyramid_levels": "a query", "mav_pyramid_dims": "a query", "mav_lk_level_dims": "a query",
    "mav_sync": "waits", "mav_stream": "a query", "mav_dev_alloc": "allocation: the block is the caller's", "mav_dev_free": "allocation",
    "mav_memcpy_h2d": "a copy between the caller's blocks", "mav_memcpy_d2h": "a copy between the caller's blocks", "mav_host_alloc": "host memory",
    "mav_host_free": "host memory", "mav_upload_async": "a copy into the caller's block", "mav_upload_async_unordered": "a copy into the caller's block",
    "mav_upload_fence": "stream order only", "mav_upload_gather": "a copy into the caller's block through a page-locked host ring",
    "mav_download_async": "a copy out of the caller's block", "mav_marker_create": "an event", "mav_marker_record": "an event", "mav_marker_wait": "an event",
    "mav_marker_query": "an event", "mav_marker_destroy": "an event", "mav_timer_start": "two events", "mav_timer_stop": "two events",
    "mav_profile_enable": "host records and events", "mav_profile_get": "host records", "mav_profile_busy": "host records", "mav_profile_intervals": "host records",
    "mav_membw_probe": "allocates, clears and frees buffers of its own",
    "mav_allgather_results": "the caller's blocks through a communicator",
    "mav_stage_remap_linear": "a stage hook: staging blocks in, staging blocks out",
    "mav_stage_blur_resize": "a stage hook on the Farneback workspace (schedule_cases.dirty)", "mav_stage_blur_resize_two_pass": "a stage hook (as above)",
    "mav_stage_blur_resize_ex": "a stage hook (as above)", "mav_stage_polyexp": "a stage hook (as above)", "mav_stage_update_matrices": "a stage hook (as above)",
    "mav_stage_update_matrices_from": "a stage hook (as above)", "mav_stage_initial_flow": "a stage hook (as above)", "mav_stage_blur_iter": "a stage hook (as above)",
    "mav_stage_coefficients": "a stage hook: host tables", "mav_stage_phi_mask": "a stage hook of the detection's phi kernel",
    "mav_stage_pyramid_level": "a stage hook of the pyramid", "mav_stage_lk_pyramid": "a stage hook of the sparse workspace",
    "mav_stage_lk_scharr": "a stage hook of the sparse workspace", "mav_stage_min_eigen": "a stage hook of the sparse workspace",
    "mav_stage_corner_response": "a stage hook of the sparse workspace", "mav_stage_corner_pick": "a stage hook of the sparse workspace",
})


def family_of() -> dict:
    """header function -> the names of the families that list it"""
    m = {}
    for f in FAMILIES:
        for e in f.entries:
            m.setdefault(e, []).append(f.name)
    for name, entries in DEFERRED.items():
        for e in entries:
            m.setdefault(e, []).append(name)
    return m

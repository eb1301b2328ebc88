"""The resident results of a context as a table: which calls leave something on the device for the mav_last_* readers (PRODUCERS),
which calls come back for it (READERS), and what every other entry point of include/mavflow.h does to it when it runs in between
(INTERVENERS): `keeps` -- every reader still returns the producer's bytes -- or `drops` -- every reader of that kind returns
MAV_ERR_STATE and writes nothing.  A third outcome, OK with other bytes, is the defect the table exists to catch.

The classes are not observations: each comes from a rule that cites the lines of csrc/mavflow.cpp it mirrors (RULES), and
tests/test_resident_cases_cpu.py reads those lines against the table.  tests/test_gpu_resident_state.py runs every sequence.

Kinds of resident state (what the context remembers, mav_ctx in csrc/mavflow.cpp):
  render  last_render: flow, derotation block, FoE, sky, thresholds, fixed mask   -> mav_last_render(_png), mav_last_overlay(_png)
  roc     last_roc: field (float32 or float64), derotation block, FoE, sky         -> mav_last_roc_sweep
  masks   last_mf / last_md: the two masks of a HOST detection call                -> mav_last_masks_tpr_fpr, mav_last_masks_components
  motion  gm.last: flow and matrix of a global-motion call                        -> mav_last_global_motion_render
  flow    last_flow: where the newest flow call wrote                              -> mav_last_flow_dev
mav_last_flow_dev has no error state: it reports the newest flow call's buffer, whatever ran since.  For that kind `drops` therefore
reads "replaced" (the reader answers for the intervener's flow, not the producer's), and HostCall::fresh, which does not touch
last_flow, keeps it.  "Replaced" is held like any other class: every form that computes flow says which field it computes and where
(Form.flow), and the reader must report that place and those bytes.

66x33 (no multiple of any tile, one Farneback layer), max_batch 3: the frames and inputs of tests/test_gpu_host_calls.py."""
import ctypes as C
import functools
import os
import re
from dataclasses import dataclass, field

import numpy as np

import detect_cases as dc

W, H, B = 66, 33, 3
N0 = W * H
N_PAIRS = dc.DETECT_PAIRS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow.h")
SOURCE = os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow.cpp")
OK, ERR_ARG, ERR_HIP, ERR_OOM, ERR_STATE = 0, -1, -2, -3, -4
KINDS = ("render", "roc", "masks", "motion", "flow")
ANGLES, MAGS = (5.0, 15.0, 40.0), (0.25, 1.0)
RADIUS = 10
N_COORDS = 40


def header_functions(text: str) -> list:
    """every function the header declares, in order"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\b(mav_[a-z0-9_]+)\s*\(", text)


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
# rule -> the kinds it drops; the comment is the place in csrc/mavflow.cpp the rule restates
RULES = {
    # HostCall::fresh: last_mf = last_md = nullptr, last_mask_batch = 0, last_render.batch = 0, last_roc.batch = 0, gm.last.batch = 0
    "fresh": {"render", "roc", "masks", "motion"},
    # ... and farneback_run's tail behind it (host calls that compute flow): c->last_flow = flow
    "fresh+flow": {"render", "roc", "masks", "motion", "flow"},
    # farneback_run's tail: last_flow = flow, last_render.batch = 0, last_roc.batch = 0, gm.last.batch = 0 (the masks of a host call
    # live in staging blocks that no _dev call takes)
    "flow": {"render", "roc", "motion", "flow"},
    # HostCall::after_last takes the NEXT free blocks and gives them back: a reader
    "after_last": set(),
    # a _dev call that writes caller-owned memory and workspaces no last_* record points at; mav_ransac (its own two doubles)
    "private": set(),
    # options, lifecycle, queries, copies, markers, timers: no kernel on anything resident
    "state": set(),
}
# Refused forms keep everything, except host-pointer calls whose fresh() has run when the refusal comes (the argument is judged behind
# `CHK(h.fresh(batch))`): those drop what fresh drops.  By form name.
FRESH_BEFORE_REFUSAL = {
    "mav_detect refused(n_pairs=0)", "mav_process_batch refused(n_pairs=0)", "mav_foe_dense refused(n_pairs=0)",
    "mav_foe_dense_f32 refused(n_pairs=4097)", "mav_overlay refused(NaN foe_gt)", "mav_global_motion_batch refused(sample outside)",
    "mav_flow_homography refused(n=3)", "mav_find_homography refused(n=3)", "mav_global_motion refused(scale=1)",
    "mav_tpr_fpr_counts refused(mask_value=0)", "mav_analyze_pyramid refused(scale=1)",
}


# A frame step judges its step arguments before anything is enqueued, but its detection's arguments only when it gets there: one that
# computes flow and is then refused inside mav_detect_dev (frame_step_body: `CHK(mav_farneback_dev(...))` runs, `CHK(mav_detect_dev(...))`
# answers MAV_ERR_ARG) has run its gathers and its Farneback.  It drops what farneback_run's tail drops, as an accepted flow call does
# ("Resident results"; tests/test_gpu_pipeline_ownership.py holds the step's markers to this part-way refusal).  By form name.
ENQUEUED_BEFORE_REFUSAL = {
    "mav_frame_step_dev refused(compute flow, n_pairs=0)",
}


@dataclass(frozen=True)
class Form:
    """One way to call an entry point between a producer and its readers.  run(env) -> the library's return code.  refused: the code
    the library must answer with (None: an accepted call).  leaves: kinds the call makes resident itself (a reader of such a kind
    answers for this call: only its return code is held -- and, for the flow kind, `flow`).  flow: for a call that computes flow,
    (which field of alt_flows() it computes, whether it lands in the interveners' own block env.out(3) -- else in a block of the
    context's); None for every other call."""
    name: str
    entry: str
    rule: str
    run: object
    refused: object = None
    leaves: frozenset = frozenset()
    flow: object = None

    def klass(self, kind: str) -> str:
        if kind in self.leaves:
            return "replaces"
        if self.refused is None or self.name in ENQUEUED_BEFORE_REFUSAL:
            dropped = RULES[self.rule]
        elif self.name in FRESH_BEFORE_REFUSAL:
            dropped = RULES["fresh"]
        else:
            return "keeps"
        return "drops" if kind in dropped else "keeps"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs() -> dict:
    """the inputs every producer reads (tests/test_gpu_host_calls.py's), and under "alt" what the interveners run on: other flow, other
    rates, other FoEs, other frames.  Nothing writes them."""
    from mavflow import _lib, synth
    rng = np.random.default_rng(66033)
    frames = np.stack([synth.make_pair(W, H, i)[0] for i in range(B + 1)])
    flow32 = np.array(dc.noise_fields(W, H))
    fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
    fp.n_pairs, fp.mag_threshold = N_PAIRS, dc.DETECT_GATE
    v = dict(prev=frames[:-1].copy(), next=frames[1:].copy(), flow32=flow32, flow64=flow32.astype(np.float64), foe=dc.foes(W, H),
             sky=dc.sky_masks(W, H).astype(np.uint8), samples=dc.detect_samples(W, H, B, N_PAIRS), omega=dc.OMEGA.copy(), dt=dc.DT.copy(),
             frame0=np.array([1, 0, 0], np.uint8), fp=fp, tp=tp, gt=np.where(rng.random((B, H, W)) < 0.3, 255, 0).astype(np.uint8),
             bgr=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), foe_gt=dc.foes(W, H)[::-1].copy())
    v["coords"] = np.stack([rng.integers(0, W, N_COORDS), rng.integers(0, H, N_COORDS)], 1).astype(np.int32)
    v["M"] = np.array([[[1.01, 0.02, 0.5], [-0.01, 0.99, -0.3]], [[0.98, -0.03, 1.25], [0.02, 1.02, 0.75]],
                       [[1.0, 0.01, -0.5], [0.015, 0.97, 0.25]]])
    aframes = np.stack([synth.make_pair(W, H, i + 7)[0] for i in range(B + 1)])
    v["alt"] = dict(prev=aframes[:-1].copy(), next=aframes[1:].copy(), flow32=np.ascontiguousarray(flow32[::-1] * np.float32(1.5) + np.float32(0.25)),
                    foe=np.ascontiguousarray(dc.foes(W, H)[::-1] * 0.5 + 3.0), sky=(1 - v["sky"]).astype(np.uint8),
                    samples=dc.detect_samples(W, H, B, N_PAIRS, seed=1), omega=np.ascontiguousarray(-2.0 * dc.OMEGA[::-1] + 0.1),
                    dt=np.ascontiguousarray(dc.DT[::-1] * 3.0), frame0=np.array([0, 1, 0], np.uint8),
                    gt=np.where(rng.random((B, H, W)) < 0.6, 255, 0).astype(np.uint8), bgr=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8),
                    coords=np.stack([rng.integers(0, W, 24), rng.integers(0, H, 24)], 1).astype(np.int32),
                    M=np.ascontiguousarray(v["M"][::-1] * 1.01),
                    # a vote whose winner is nowhere near a detection's FoE: seven estimates around (5.5, 7.25), two strays
                    estimates=np.array([[5.5, 7.25], [6.0, 7.0], [5.0, 8.0], [5.75, 6.5], [4.5, 7.5], [6.5, 8.25], [5.25, 7.75],
                                        [400.0, -90.0], [-300.0, 250.0]]))
    v["alt"]["flow64"] = v["alt"]["flow32"].astype(np.float64)
    for a in list(v.values()) + list(v["alt"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


def p_(a):
    """host array -> void*"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def vp(p):
    """device address -> void* (never a bare Python int: an entry point without argtypes would take it as a C int)"""
    return None if p is None else C.c_void_p(int(p))


class HipFailure(RuntimeError):
    """a call answered MAV_ERR_HIP / MAV_ERR_OOM: the context's sequences stop here"""


def hip_failure(e: BaseException):
    """the HipFailure an exception of the bindings stands for -- mavflow._lib.check raises MavflowError("[-2] ...") for MAV_ERR_HIP and
    MemoryError for MAV_ERR_OOM, which is how a producer, ctx.sync() or a copy reports a fault -- or None for any other exception (a
    refusal, MAV_ERR_STATE, a mistake of the test's)"""
    from mavflow import _lib
    if isinstance(e, HipFailure):
        return e
    if isinstance(e, MemoryError):
        return HipFailure(f"[{ERR_OOM}] {e}")
    if isinstance(e, _lib.MavflowError) and str(e).startswith((f"[{ERR_HIP}]", f"[{ERR_OOM}]")):
        return HipFailure(str(e))
    return None


def code(fn, *a, **kw) -> int:
    """the return code of a binding call that raises (mavflow._lib.check)"""
    from mavflow import _lib
    try:
        fn(*a, **kw)
        return OK
    except ValueError:
        return ERR_ARG
    except MemoryError:
        return ERR_OOM
    except _lib.MavflowError as e:
        s = str(e)
        return int(s[1:s.index("]")])


class Env:
    """One context with the producers' and the interveners' device buffers.  dev(name, array | bytes): a caller-owned block, made and
    filled once (mav_dev_alloc: not part of the context's ctx_bytes).  Producers' blocks are "p_*", interveners' "iv_*": no intervener
    is handed a producer's block."""

    def __init__(self, ctx):
        self.ctx, self.lib, self.x, self.d, self.hist = ctx, ctx.lib, inputs(), {}, None
        self.y = self.x["alt"]

    @property
    def h(self):
        return self.ctx.h

    def dev(self, name, src):
        if name not in self.d:
            self.d[name] = self.ctx.alloc(src) if isinstance(src, int) else self.ctx.alloc(src.nbytes).upload(src)
        return self.d[name].ptr

    def out(self, i=0):
        """the i-th of eight 256 KB output blocks of the interveners"""
        return self.dev("iv_out", 8 << 18) + (i << 18)

    def history(self):
        if self.hist is None:
            self.hist = self.ctx.flow_history(3)
        return self.hist

    def close(self):
        if self.hist is not None:
            self.hist.close()
        for b in self.d.values():
            b.free()
        self.d = {}


# ---- producers ------------------------------------------------------------------------------------------------------------------------
def _par_block(x):
    """samples | omega | dt | frame0 packed as a frame step reads them; -> (bytes, offsets)"""
    parts = [np.ascontiguousarray(x["samples"], np.uint32), x["omega"], x["dt"], x["frame0"]]
    off, blob = [], b""
    for a in parts:
        blob += b"\0" * (-len(blob) % 8)
        off.append(len(blob))
        blob += a.tobytes()
    return np.frombuffer(blob, np.uint8).copy(), off


def _pdev(env, own_flow=True):
    x = env.x
    n = N0 * B
    d = dict(flow=env.dev("p_flow", x["flow32"]), samples=env.dev("p_samples", np.ascontiguousarray(x["samples"], np.uint32)),
             omega=env.dev("p_omega", x["omega"]), dt=env.dev("p_dt", x["dt"]), frame0=env.dev("p_frame0", x["frame0"]),
             sky=env.dev("p_sky", x["sky"]), prev=env.dev("p_prev", x["prev"]), next=env.dev("p_next", x["next"]),
             mf=env.dev("p_mf", n), md=env.dev("p_md", n), res=env.dev("p_res", 32 * B), flow_out=env.dev("p_flow_out", 8 * n),
             mres=env.dev("p_mres", 128 * B), Hm=env.dev("p_H", 72 * B), ok=env.dev("p_ok", 4 * B))
    return d


def _dev_info(env, d, flow_ptr, computed):
    """what a device producer wrote, brought to the host (the stream is drained first)"""
    from mavflow import _lib
    env.ctx.sync()
    res = env.d["p_res"].download(_lib.RESULT_DTYPE, (B,))
    flow = np.empty((B, H, W, 2), np.float32)
    _lib.check(env.lib.mav_memcpy_d2h(env.h, p_(flow), vp(flow_ptr), flow.nbytes))
    return dict(flow=flow if computed else env.x["flow32"], foe=np.ascontiguousarray(res["foe"]), mf=env.d["p_mf"].download(np.uint8, (B, H, W)),
                md=env.d["p_md"].download(np.uint8, (B, H, W)), form="rates", flow_ptr=flow_ptr)


def _host_info(env, out, flow):
    return dict(flow=np.array(flow), foe=np.ascontiguousarray(out["results"]["foe"]), mf=np.array(out["mask_fixed"]).view(np.uint8),
                md=np.array(out["mask_dyn"]).view(np.uint8), form="rates")


def prod_detect(env):
    x = env.x
    out = env.ctx.detect(x["flow32"], x["samples"], omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"], foe_params=x["fp"],
                         thr_params=x["tp"])
    return _host_info(env, out, x["flow32"])


def prod_process_batch(env):
    x = env.x
    out = env.ctx.process_batch(x["prev"], x["next"], x["samples"], omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"],
                                foe_params=x["fp"], thr_params=x["tp"])
    return _host_info(env, out, out["flow"])


def _prod_phi(f32):
    def run(env):
        from mavflow import _lib
        x = env.x
        mf, md = np.empty((B, H, W), np.uint8), np.empty((B, H, W), np.uint8)
        fn = env.lib.mav_phi_mask_f32 if f32 else env.lib.mav_phi_mask
        _lib.check(fn(env.h, p_(x["flow32"] if f32 else x["flow64"]), p_(x["foe"]), p_(x["sky"]), B, C.byref(x["tp"]), None, p_(mf), p_(md), None))
        return dict(flow=x["flow32"], foe=x["foe"], mf=mf, md=md, form="frame0" if f32 else "plain")
    return run


def prod_detect_dev(env):
    from mavflow import _lib
    d, x = _pdev(env), env.x
    _lib.check(env.lib.mav_detect_dev(env.h, vp(d["flow"]), vp(d["samples"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]), vp(d["sky"]), B,
                                      C.byref(x["fp"]), C.byref(x["tp"]), None, vp(d["mf"]), vp(d["md"]), vp(d["res"])))
    return _dev_info(env, d, d["flow"], False)


def _prod_process_batch_dev(own_flow):
    def run(env):
        from mavflow import _lib
        d, x = _pdev(env), env.x
        _lib.check(env.lib.mav_process_batch_dev(env.h, vp(d["prev"]), vp(d["next"]), vp(d["samples"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]),
                                                 vp(d["sky"]), B, C.byref(x["fp"]), C.byref(x["tp"]), vp(d["flow_out"]) if own_flow else None, None,
                                                 vp(d["mf"]), vp(d["md"]), vp(d["res"])))
        fl = d["flow_out"] if own_flow else env.lib.mav_last_flow_dev(env.h)
        return _dev_info(env, d, fl, True)
    return run


def _step(env, d, detect_only=False, flow=None):
    """the frame step of the producers: Farneback of the frames into the caller's buffer, then the detection"""
    from mavflow import _lib
    x = env.x
    par, off = _par_block(x)
    s = _lib.FrameStep()
    s.n = B
    s.par_dev = env.dev("p_par", par)
    s.compute_flow = 0 if detect_only else 1
    s.prev_dev, s.next_dev, s.flow_dev = d["prev"], d["next"], (flow if flow is not None else d["flow_out"])
    s.detect = 1
    s.off_samples, s.off_omega, s.off_dt, s.off_frame0 = off
    s.has_omega = s.has_frame0 = 1
    s.sky_dev = d["sky"]
    s.foe, s.thr = x["fp"], x["tp"]
    s.mask_fixed_dev, s.mask_dyn_dev, s.out_dev = d["mf"], d["md"], d["res"]
    return s


def prod_frame_step_dev(env):
    from mavflow import _lib
    d = _pdev(env)
    s = _step(env, d)
    _lib.check(env.lib.mav_frame_step_dev(env.h, C.byref(s)))
    return _dev_info(env, d, d["flow_out"], True)


def prod_frame_step_post(env):
    """the same step through the worker; it is waited for, and the worker drained, before anything reads"""
    d = _pdev(env)
    s = _step(env, d)
    env.h                                        # (drains whatever was posted before)
    t = env.ctx.post_step(s)
    env.ctx.wait_step(t)
    env.ctx.drain()
    return _dev_info(env, d, d["flow_out"], True)


def prod_global_motion(env):
    x = env.x
    env.ctx.global_motion(x["flow32"], x["M"], outputs=())
    return dict(flow=x["flow32"], Hm=x["M"])


def _prod_motion_step(own_H):
    def run(env):
        d, x = _pdev(env), env.x
        env.ctx.global_motion_step(vp(d["flow"]), x["coords"], B, vp(d["mres"]), H_ptr=vp(d["Hm"]) if own_H else None, ok_ptr=vp(d["ok"]) if own_H else None)
        env.ctx.sync()
        return dict(flow=x["flow32"], Hm="fit")
    return run


def prod_global_motion_batch(env):
    x = env.x
    got = env.ctx.global_motion_batch(x["prev"], x["next"], x["coords"])
    return dict(flow="farneback", Hm=got["H"].copy(), flow_ptr=env.lib.mav_last_flow_dev(env.h))


@dataclass(frozen=True)
class Producer:
    entries: tuple               # the header's functions this producer stands for
    leaves: tuple                # the kinds it leaves resident
    run: object                  # run(env) -> what the direct calls need


PRODUCERS = {
    "detect": Producer(("mav_detect",), ("render", "roc", "masks"), prod_detect),
    "process_batch": Producer(("mav_process_batch",), ("render", "roc", "masks"), prod_process_batch),
    "phi_mask": Producer(("mav_phi_mask",), ("roc", "masks"), _prod_phi(False)),
    "phi_mask_f32": Producer(("mav_phi_mask_f32",), ("roc", "masks"), _prod_phi(True)),
    "detect_dev": Producer(("mav_detect_dev",), ("render", "roc"), prod_detect_dev),
    "process_batch_dev": Producer(("mav_process_batch_dev",), ("render", "roc", "flow"), _prod_process_batch_dev(True)),
    "process_batch_dev(flow=NULL)": Producer(("mav_process_batch_dev",), ("render", "roc", "flow"), _prod_process_batch_dev(False)),
    "frame_step_dev": Producer(("mav_frame_step_dev",), ("render", "roc", "flow"), prod_frame_step_dev),
    "frame_step_post+wait": Producer(("mav_frame_step_post", "mav_frame_step_wait"), ("render", "roc", "flow"), prod_frame_step_post),
    "global_motion": Producer(("mav_global_motion",), ("motion",), prod_global_motion),
    "global_motion_step_dev(H=NULL)": Producer(("mav_global_motion_step_dev",), ("motion",), _prod_motion_step(False)),
    "global_motion_step_dev": Producer(("mav_global_motion_step_dev",), ("motion",), _prod_motion_step(True)),
    "global_motion_batch": Producer(("mav_global_motion_batch",), ("motion", "flow"), prod_global_motion_batch),
}


# ---- readers --------------------------------------------------------------------------------------------------------------------------
def canary(shape, dt):
    """an output filled with a byte no result is made of all over (tests/test_gpu_host_calls.py's _outs)"""
    return np.full(shape, 0xA5 if np.dtype(dt).kind in "ui" else np.nan, dt)


def untouched(a) -> bool:
    return a.tobytes() == canary(a.shape, a.dtype).tobytes()


def _png_buf(env, count):
    need = env.lib.mav_png_bound(W, H, 3) * count
    return canary((need,), np.uint8), canary((count, 2), np.uint64)


def _png_files(out, index):
    from mavflow.frame_source import png_wrap
    return tuple(png_wrap(W, H, 3, out[int(o):int(o) + int(n)].tobytes()) for o, n in index)


def _roc_params():
    from mavflow import _lib
    return _lib.roc_params(ANGLES, MAGS)         # (struct, angles, mags): the arrays must outlive the call


def read_render(env):
    o = [canary((B, H, W, 3), np.uint8) for _ in range(3)]
    rc = env.lib.mav_last_render(env.h, B, p_(o[0]), p_(o[1]), p_(o[2]))
    return rc, o, tuple(a.tobytes() for a in o)


def read_render_png(env):
    out, idx = _png_buf(env, 3 * B)
    rc = env.lib.mav_last_render_png(env.h, B, 1, 1, 1, p_(out), C.c_size_t(out.size), p_(idx))
    return rc, [out, idx], (_png_files(out, idx) if rc == OK else None)


def read_overlay(env):
    o, wr = canary((B, H, W, 3), np.uint8), canary((B,), np.uint8)
    rc = env.lib.mav_last_overlay(env.h, p_(env.x["bgr"]), p_(env.x["foe_gt"]), B, RADIUS, p_(o), p_(wr))
    return rc, [o, wr], (o.tobytes(), wr.tobytes())


def read_overlay_png(env):
    out, idx = _png_buf(env, B)
    wr = canary((B,), np.uint8)
    rc = env.lib.mav_last_overlay_png(env.h, p_(env.x["bgr"]), p_(env.x["foe_gt"]), B, RADIUS, p_(out), C.c_size_t(out.size), p_(idx), p_(wr))
    return rc, [out, idx, wr], ((_png_files(out, idx), wr.tobytes()) if rc == OK else None)


def read_counts(env):
    cf, cd = canary((B, 4), np.int64), canary((B, 4), np.int64)
    rc = env.lib.mav_last_masks_tpr_fpr(env.h, p_(env.x["gt"]), 255, B, p_(cf), p_(cd))
    return rc, [cf, cd], (cf.tobytes(), cd.tobytes())


def _read_components(which):
    def read(env):
        from mavflow import _lib
        p = _lib.cc_defaults(connectivity=8, min_area=1, max_blobs=64)
        lab, cnt, tab = canary((B, H, W), np.int32), canary((B, 8), np.uint8), canary((B, 64 * 40), np.uint8)
        rc = env.lib.mav_last_masks_components(env.h, which, B, C.byref(p), p_(lab), p_(cnt), p_(tab))
        return rc, [lab, cnt, tab], (lab.tobytes(), cnt.tobytes(), tab.tobytes())
    return read


def read_roc(env):
    from mavflow import _lib
    rp, a, m = _roc_params()
    tab = canary((B, _lib.roc_table_words(len(ANGLES), len(MAGS))), np.int64)
    rc = env.lib.mav_last_roc_sweep(env.h, p_(env.x["gt"]), B, B, C.byref(rp), p_(tab))
    return rc, [tab], _lib.roc_expand(tab, len(ANGLES), len(MAGS)).tobytes()


def read_motion(env):
    o = [canary((B, H, W, 3), np.uint8) for _ in range(2)]
    rc = env.lib.mav_last_global_motion_render(env.h, B, p_(o[0]), p_(o[1]))
    return rc, o, tuple(a.tobytes() for a in o)


def read_flow(env):
    """the pointer mav_last_flow_dev reports and the B fields behind it (never an error: see the module's head)"""
    from mavflow import _lib
    ptr = env.lib.mav_last_flow_dev(env.h)
    flow = np.empty((B, H, W, 2), np.float32)
    env.ctx.sync()
    _lib.check(env.lib.mav_memcpy_d2h(env.h, p_(flow), vp(ptr), flow.nbytes))
    return OK, [], (ptr, flow.tobytes())


# reader -> (the header's function, the kind it needs, read(env) -> (return code, its outputs, the outputs as comparable values))
READERS = {
    "render_last": ("mav_last_render", "render", read_render),
    "render_last_png": ("mav_last_render_png", "render", read_render_png),
    "overlay_last": ("mav_last_overlay", "render", read_overlay),
    "overlay_last_png": ("mav_last_overlay_png", "render", read_overlay_png),
    "counts_last": ("mav_last_masks_tpr_fpr", "masks", read_counts),
    "components_last(fixed)": ("mav_last_masks_components", "masks", _read_components(0)),
    "components_last(dynamic)": ("mav_last_masks_components", "masks", _read_components(1)),
    "roc_sweep_last": ("mav_last_roc_sweep", "roc", read_roc),
    "motion_render_last": ("mav_last_global_motion_render", "motion", read_motion),
    "last_flow_dev": ("mav_last_flow_dev", "flow", read_flow),
}


def readers_of(producer: str) -> list:
    return [r for r, (_, kind, _) in READERS.items() if kind in PRODUCERS[producer].leaves]


# ---- the direct calls: the baseline from the entry points that take everything from the host ---------------------------------------------
def direct(ref, x, info, kinds) -> dict:
    """reader -> the same values from `ref`, a context of its own (ctx.render, ctx.overlay, ctx.png_encode, ctx.tpr_fpr_counts,
    ctx.components, ctx.roc_sweep, ctx.flow_to_color on tests/global_motion_ref.py's fields)"""
    from mavflow import _lib
    out = {}
    if "render" in kinds:
        rates = dict(omega=x["omega"], dt=x["dt"], sky=x["sky"], frame0=x["frame0"])
        imgs = ref.render(info["flow"], info["foe"], thr_params=x["tp"], **rates)
        order = [imgs["result"], imgs["flow"], imgs["phi"]]
        over, wr = ref.overlay(x["bgr"], info["mf"], info["foe"], x["foe_gt"], radius=RADIUS)
        over, wr = np.array(over), np.array(wr).view(np.uint8)
        out["render_last"] = tuple(a.tobytes() for a in order)
        out["render_last_png"] = tuple(f for a in order for f in ref.png_encode(a))
        out["overlay_last"] = (over.tobytes(), wr.tobytes())
        out["overlay_last_png"] = (tuple(ref.png_encode(over)), wr.tobytes())
    if "masks" in kinds:
        out["counts_last"] = (ref.tpr_fpr_counts(x["gt"], info["mf"]).tobytes(), ref.tpr_fpr_counts(x["gt"], info["md"]).tobytes())
        for name, m in (("components_last(fixed)", info["mf"]), ("components_last(dynamic)", info["md"])):
            p = _lib.cc_defaults(connectivity=8, min_area=1, max_blobs=64)
            lab, cnt, tab = np.empty((B, H, W), np.int32), np.empty((B, 8), np.uint8), np.empty((B, 64 * 40), np.uint8)
            _lib.check(ref.lib.mav_components(ref.h, p_(np.ascontiguousarray(m)), B, C.byref(p), p_(lab), p_(cnt), p_(tab)))
            out[name] = (lab.tobytes(), cnt.tobytes(), tab.tobytes())      # (unused records are zero bytes: whole tables compare)
    if "roc" in kinds:
        # "plain": mav_phi_mask's float64 field is the float32 one widened, which is what a pair without rates and flag computes on
        rates = dict(rates=dict(omega=x["omega"], dt=x["dt"], frame0=x["frame0"]), frame0=dict(frame0=np.ones(B, np.uint8)), plain={})[info["form"]]
        got = ref.roc_sweep(info["flow"], info["foe"], x["gt"], ANGLES, MAGS, sky=x["sky"], **rates)
        out["roc_sweep_last"] = got["counts"].tobytes()                     # (B, Ka, Km, 4): compare with _lib.roc_expand of the reader's table
    if "flow" in kinds:
        out["last_flow_dev"] = (info["flow_ptr"], info["flow"].tobytes())
    if "motion" in kinds:
        import global_motion_ref as R
        subs = [R.subtract(info["flow"][b], info["Hm"][b]) for b in range(B)]
        out["motion_render_last"] = (ref.flow_to_color(np.stack([s["warped"] for s in subs])).tobytes(),
                                     ref.flow_to_color(np.stack([s["global_motion"] for s in subs])).tobytes())
    return out


# ---- interveners ----------------------------------------------------------------------------------------------------------------------
def alt_flows(ref) -> dict:
    """the fields the interveners that compute flow compute, from `ref`, a context of its own: Form.flow[0] -> (B, H, W, 2) float32"""
    y = inputs()["alt"]
    return dict(plain=np.array(ref.farneback(y["prev"], y["next"])), init=np.array(ref.farneback(y["prev"], y["next"], initial_flow=y["flow32"])))


def _foe_params(n_pairs):
    from mavflow import _lib
    fp = _lib.foe_defaults()
    fp.n_pairs, fp.mag_threshold = n_pairs, dc.DETECT_GATE
    return fp


def _ydev(env):
    y = env.y
    return dict(flow=env.dev("iv_flow", y["flow32"]), samples=env.dev("iv_samples", np.ascontiguousarray(y["samples"], np.uint32)),
                omega=env.dev("iv_omega", y["omega"]), dt=env.dev("iv_dt", y["dt"]), frame0=env.dev("iv_frame0", y["frame0"]),
                sky=env.dev("iv_sky", y["sky"]), prev=env.dev("iv_prev", y["prev"]), next=env.dev("iv_next", y["next"]),
                foe=env.dev("iv_foe", y["foe"]), gt=env.dev("iv_gt", y["gt"]), bgr=env.dev("iv_bgr", y["bgr"]),
                flow64=env.dev("iv_flow64", y["flow64"]), M=env.dev("iv_M", np.ascontiguousarray(y["M"])),
                pts=env.dev("iv_pts", np.array([[10.5, 8.0], [33.0, 16.5], [50.25, 20.0], [5.0, 30.0]], np.float32)),
                n=env.dev("iv_n", np.array([4], np.int32)))


def iv_detect_dev(n_pairs):
    def run(env):
        d, fp, tp = _ydev(env), _foe_params(n_pairs), env.x["tp"]
        return env.lib.mav_detect_dev(env.h, vp(d["flow"]), vp(d["samples"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]), vp(d["sky"]), B,
                                      C.byref(fp), C.byref(tp), None, vp(env.out(0)), vp(env.out(1)), vp(env.out(2)))
    return run


def iv_process_batch_dev(n_pairs):
    def run(env):
        d, fp, tp = _ydev(env), _foe_params(n_pairs), env.x["tp"]
        return env.lib.mav_process_batch_dev(env.h, vp(d["prev"]), vp(d["next"]), vp(d["samples"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]),
                                             vp(d["sky"]), B, C.byref(fp), C.byref(tp), vp(env.out(3)), None, vp(env.out(0)), vp(env.out(1)),
                                             vp(env.out(2)))
    return run


def _iv_step(env, n=B, n_pairs=N_PAIRS, compute_flow=1):
    from mavflow import _lib
    d, y = _ydev(env), env.y
    par, off = _par_block(y)
    s = _lib.FrameStep()
    s.n = n
    s.par_dev = env.dev("iv_par", par)
    s.compute_flow = compute_flow
    s.prev_dev, s.next_dev, s.flow_dev = d["prev"], d["next"], (env.out(3) if compute_flow else d["flow"])
    s.detect = 1
    s.off_samples, s.off_omega, s.off_dt, s.off_frame0 = off
    s.has_omega = s.has_frame0 = 1
    s.sky_dev = d["sky"]
    s.foe, s.thr = _foe_params(n_pairs), env.x["tp"]
    s.mask_fixed_dev, s.mask_dyn_dev, s.out_dev = env.out(0), env.out(1), env.out(2)
    return s


def iv_frame_step_dev(**kw):
    def run(env):
        s = _iv_step(env, **kw)
        return env.lib.mav_frame_step_dev(env.h, C.byref(s))
    return run


def iv_frame_step_post(env):
    s = _iv_step(env)
    env.h
    rc = code(lambda: env.ctx.wait_step(env.ctx.post_step(s)))
    env.ctx.drain()
    return rc


def iv_frame_step_post_refused(env):
    s = _iv_step(env)
    s.n_gather = -1
    t = C.c_uint64()
    return env.lib.mav_frame_step_post(env.h, C.byref(s), C.byref(t))


def iv_frame_step_wait_refused(env):
    return env.lib.mav_frame_step_wait(env.h, C.c_uint64(1 << 40), None)


def iv_host_detect(n_pairs, batch=B):
    def run(env):
        from mavflow import _lib
        y, fp = env.y, _foe_params(n_pairs)
        res, mf, md = np.empty(B + 1, _lib.RESULT_DTYPE), np.empty((B + 1, H, W), np.uint8), np.empty((B + 1, H, W), np.uint8)
        return env.lib.mav_detect(env.h, p_(y["flow32"]), p_(y["samples"]), p_(y["omega"]), p_(y["dt"]), p_(y["frame0"]), p_(y["sky"]), batch,
                                  C.byref(fp), C.byref(env.x["tp"]), None, p_(mf), p_(md), p_(res))
    return run


def iv_host_process_batch(n_pairs):
    def run(env):
        from mavflow import _lib
        y, fp = env.y, _foe_params(n_pairs)
        res, mf, md = np.empty(B, _lib.RESULT_DTYPE), np.empty((B, H, W), np.uint8), np.empty((B, H, W), np.uint8)
        return env.lib.mav_process_batch(env.h, p_(y["prev"]), p_(y["next"]), p_(y["samples"]), p_(y["omega"]), p_(y["dt"]), p_(y["frame0"]),
                                         p_(y["sky"]), B, C.byref(fp), C.byref(env.x["tp"]), None, None, p_(mf), p_(md), p_(res))
    return run


def iv_foe_dense(f32, n_pairs):
    def run(env):
        y, fp = env.y, _foe_params(n_pairs)
        foe = np.empty((B, 2))
        fn = env.lib.mav_foe_dense_f32 if f32 else env.lib.mav_foe_dense
        return fn(env.h, p_(y["flow32"] if f32 else y["flow64"]), p_(y["samples"]), B, C.byref(fp), p_(foe))
    return run


def iv_phi_mask(f32, batch=B):
    def run(env):
        y = env.y
        mf, md = np.empty((B, H, W), np.uint8), np.empty((B, H, W), np.uint8)
        fn = env.lib.mav_phi_mask_f32 if f32 else env.lib.mav_phi_mask
        return fn(env.h, p_(y["flow32"] if f32 else y["flow64"]), p_(y["foe"]), p_(y["sky"]), batch, C.byref(env.x["tp"]), None, p_(mf), p_(md), None)
    return run


def iv_ransac(count=None):
    def run(env):
        est = env.y["estimates"]
        foe = np.empty(2)
        return env.lib.mav_ransac(env.h, p_(est), len(est) if count is None else count, C.c_double(2.0), p_(foe))
    return run


def iv_farneback_dev(batch=B):
    def run(env):
        d = _ydev(env)
        return env.lib.mav_farneback_dev(env.h, vp(d["prev"]), vp(d["next"]), batch, vp(env.out(3)))
    return run


def iv_farneback_init_dev(batch=B):
    def run(env):
        d = _ydev(env)
        return env.lib.mav_farneback_init_dev(env.h, vp(d["prev"]), vp(d["next"]), batch, vp(d["flow"]), vp(env.out(3)))
    return run


def iv_farneback_ex_dev(depth=0):
    def run(env):
        d = _ydev(env)
        return env.lib.mav_farneback_ex_dev(env.h, vp(d["prev"]), vp(d["next"]), depth, B, None, vp(env.out(3)))
    return run


def iv_farneback_ex(depth=0):
    def run(env):
        y = env.y
        flow = np.empty((B, H, W, 2), np.float32)
        return env.lib.mav_farneback_ex(env.h, p_(y["prev"]), p_(y["next"]), depth, B, None, p_(flow))
    return run


def iv_components(dev, connectivity=8):
    def run(env):
        from mavflow import _lib
        p = _lib.cc_defaults(connectivity=8, min_area=1, max_blobs=16)
        p.connectivity = connectivity
        if dev:
            return env.lib.mav_components_dev(env.h, vp(_ydev(env)["sky"]), B, C.byref(p), None, vp(env.out(0)), vp(env.out(1)))
        cnt, tab = np.empty((B, 8), np.uint8), np.empty((B, 16 * 40), np.uint8)
        return env.lib.mav_components(env.h, p_(env.y["sky"]), B, C.byref(p), None, p_(cnt), p_(tab))
    return run


def iv_overlay(dev, radius=RADIUS, nan=False):
    def run(env):
        y = env.y
        if dev:
            d = _ydev(env)
            return env.lib.mav_overlay_dev(env.h, vp(d["bgr"]), vp(d["sky"]), vp(d["foe"]), vp(d["foe"]), B, radius, vp(env.out(0)), vp(env.out(1)))
        gt = y["foe"].copy()
        if nan:
            gt[1, 0] = np.nan
        o, wr = np.empty((B, H, W, 3), np.uint8), np.empty(B, np.uint8)
        return env.lib.mav_overlay(env.h, p_(y["bgr"]), p_(y["sky"]), p_(y["foe"]), p_(gt), B, radius, p_(o), p_(wr))
    return run


def _coords(y, outside):
    c = y["coords"].copy()
    if outside:
        c[5] = (W, 3)
    return c


def iv_motion_batch(dev, outside=False):
    def run(env):
        from mavflow import _lib
        y, c = env.y, _coords(env.y, outside)
        if dev:
            d = _ydev(env)
            return env.lib.mav_global_motion_batch_dev(env.h, vp(d["prev"]), vp(d["next"]), p_(c), len(c), B, C.c_double(1.5), 0, vp(env.out(3)),
                                                       vp(env.out(0)), vp(env.out(1)), None, vp(env.out(2)))
        res = np.empty(B, _lib.MOTION_DTYPE)
        return env.lib.mav_global_motion_batch(env.h, p_(y["prev"]), p_(y["next"]), p_(c), len(c), B, C.c_double(1.5), 0, None, None, None, None, p_(res))
    return run


def iv_motion_step(outside=False, own_H=True):
    def run(env):
        d, c = _ydev(env), _coords(env.y, outside)
        return env.lib.mav_global_motion_step_dev(env.h, vp(d["flow"]), p_(c), len(c), B, C.c_double(1.5), 1, vp(env.out(0)) if own_H else None,
                                                  vp(env.out(1)) if own_H else None, None, vp(env.out(2)))
    return run


def iv_global_motion(dev, scale=1.5):
    def run(env):
        from mavflow import _lib
        y = env.y
        if dev:
            d = _ydev(env)
            return env.lib.mav_global_motion_dev(env.h, vp(d["flow"]), vp(d["M"]), B, C.c_double(scale), 0, None, None, None, vp(env.out(2)))
        res = np.empty(B, _lib.MOTION_DTYPE)
        return env.lib.mav_global_motion(env.h, p_(y["flow32"]), p_(np.ascontiguousarray(y["M"])), B, C.c_double(scale), 0, None, None, None, p_(res))
    return run


def iv_flow_homography(dev, n=None, outside=False):
    def run(env):
        y, c = env.y, _coords(env.y, outside)
        k = len(c) if n is None else n
        if dev:
            return env.lib.mav_flow_homography_dev(env.h, vp(_ydev(env)["flow"]), p_(c), k, B, vp(env.out(0)), vp(env.out(1)))
        Hm, ok = np.empty((B, 9)), np.empty(B, np.int32)
        return env.lib.mav_flow_homography(env.h, p_(y["flow32"]), p_(c), k, B, p_(Hm), p_(ok), None)
    return run


def iv_find_homography(dev, n=None):
    def run(env):
        rng = np.random.default_rng(5)
        src = rng.random((B, 12, 2)) * 60
        dst = np.ascontiguousarray(src * 1.02 + rng.random((B, 12, 2)))
        k = 12 if n is None else n
        if dev:
            return env.lib.mav_find_homography_dev(env.h, vp(env.dev("iv_src", src)), vp(env.dev("iv_dst", dst)), k, B, vp(env.out(0)), vp(env.out(1)))
        Hm, ok = np.empty((B, 9)), np.empty(B, np.int32)
        return env.lib.mav_find_homography(env.h, p_(src), p_(dst), k, B, p_(Hm), p_(ok))
    return run


def iv_history_push(dev, depth=5):
    def run(env):
        hist = env.history()
        if dev:
            return env.lib.mav_history_push_dev(env.h, hist._h, vp(_ydev(env)["flow"]), depth, 1, 0, vp(env.out(4)))
        out = np.empty((1, H, W, 2), np.float64)
        return env.lib.mav_history_push(env.h, hist._h, p_(env.y["flow32"]), depth, 1, 0, p_(out))
    return run


def iv_history_create(length=4):
    def run(env):
        from mavflow import _lib
        p, hh = _lib.HistoryParams(length, 5, 0), C.c_void_p()
        rc = env.lib.mav_history_create(env.h, C.byref(p), C.byref(hh))
        return rc if rc != OK else env.lib.mav_history_destroy(env.h, hh)
    return run


def iv_history_misc(env):
    hist = env.history()
    rc = env.lib.mav_history_reset(env.h, hist._h)
    i = C.c_int()
    return rc if rc != OK else env.lib.mav_history_info(env.h, hist._h, C.byref(i), None, None)


def iv_roc_sweep(dev, n_angles=None):
    def run(env):
        from mavflow import _lib
        y = env.y
        rp, a, m = _roc_params()
        if n_angles is not None:
            rp.n_angles = n_angles
        if dev:
            d = _ydev(env)
            return env.lib.mav_roc_sweep_dev(env.h, vp(d["flow"]), vp(d["foe"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]), vp(d["sky"]), vp(d["gt"]),
                                             B, B, None, C.byref(rp), vp(env.out(0)))
        tab = np.empty((B, _lib.roc_table_words(len(ANGLES), len(MAGS))), np.int64)
        return env.lib.mav_roc_sweep(env.h, p_(y["flow32"]), p_(y["foe"]), p_(y["omega"]), p_(y["dt"]), p_(y["frame0"]), p_(y["sky"]), p_(y["gt"]), B, B,
                                     None, C.byref(rp), p_(tab))
    return run


def iv_roc_arm(off=0):
    def run(env):
        rp, a, m = _roc_params()
        rc = env.lib.mav_roc_arm(env.h, C.byref(rp), C.c_size_t(off))
        return rc if rc != OK else env.lib.mav_roc_arm(env.h, None, C.c_size_t(0))      # (armed, then disarmed again)
    return run


def iv_render(dev, batch=B):
    def run(env):
        y = env.y
        if dev:
            d = _ydev(env)
            return env.lib.mav_render_dev(env.h, vp(d["flow"]), vp(d["foe"]), vp(d["omega"]), vp(d["dt"]), vp(d["frame0"]), vp(d["sky"]), batch,
                                          C.byref(env.x["tp"]), vp(env.out(0)), vp(env.out(1)), vp(env.out(2)))
        o = [np.empty((B + 1, H, W, 3), np.uint8) for _ in range(3)]
        return env.lib.mav_render(env.h, p_(y["flow32"]), p_(y["foe"]), p_(y["omega"]), p_(y["dt"]), p_(y["frame0"]), p_(y["sky"]), batch,
                                  C.byref(env.x["tp"]), p_(o[0]), p_(o[1]), p_(o[2]))
    return run


def iv_tpr_fpr(dev, mask_value=255):
    def run(env):
        y = env.y
        if dev:
            d = _ydev(env)
            return env.lib.mav_tpr_fpr_counts_dev(env.h, vp(d["gt"]), B, vp(d["sky"]), None, mask_value, B, vp(env.out(0)), None)
        cnt = np.empty((B, 4), np.int64)
        return env.lib.mav_tpr_fpr_counts(env.h, p_(y["gt"]), p_(y["sky"]), mask_value, B, p_(cnt))
    return run


def iv_png_encode(dev, channels=3):
    def run(env):
        bound = env.lib.mav_png_bound(W, H, 3) * B
        if dev:
            return env.lib.mav_png_encode_dev(env.h, vp(_ydev(env)["bgr"]), B, channels, vp(env.out(0)), C.c_size_t(bound), vp(env.out(1)))
        out, idx = np.empty(bound, np.uint8), np.empty((B, 2), np.uint64)
        return env.lib.mav_png_encode(env.h, p_(env.y["bgr"]), B, channels, p_(out), C.c_size_t(bound), p_(idx))
    return run


def iv_analyze_pyramid(scale=1.5):
    def run(env):
        out = np.empty((B, 6), np.int64)
        return env.lib.mav_analyze_pyramid(env.h, p_(env.y["sky"]), B, C.c_double(scale), p_(out))
    return run


def iv_lk_track(win=21):
    def run(env):
        from mavflow import _lib
        p = _lib.lk_defaults()
        p.win_w = win
        pts = np.array([[10.5, 8.0], [33.0, 16.5]], np.float32)
        out, st = np.empty((2, 2), np.float32), np.empty(2, np.uint8)
        return env.lib.mav_lk_track(env.h, p_(env.y["prev"][0]), p_(env.y["next"][0]), p_(pts), 2, C.byref(p), p_(out), p_(st))
    return run


def iv_lk_track_err(flags=0):
    def run(env):
        from mavflow import _lib
        p = _lib.lk_defaults()
        pts = np.array([[10.5, 8.0], [33.0, 16.5]], np.float32)
        out, st, err = np.empty((2, 2), np.float32), np.empty(2, np.uint8), np.empty(2, np.float32)
        return env.lib.mav_lk_track_err(env.h, p_(env.y["prev"][0]), p_(env.y["next"][0]), p_(pts), 2, C.byref(p), flags, p_(out), p_(st), p_(err))
    return run


def iv_lk_dev(which, win=21, flags=0):
    def run(env):
        from mavflow import _lib
        d, p = _ydev(env), _lib.lk_defaults()
        p.win_w = win
        a = (env.h, vp(d["prev"]), vp(d["next"]), vp(d["pts"]))
        if which == "dev":
            return env.lib.mav_lk_track_dev(*a, 4, C.byref(p), vp(env.out(0)), vp(env.out(1)))
        if which == "ex":
            return env.lib.mav_lk_track_ex_dev(*a, 4, vp(d["n"]), C.byref(p), vp(env.out(0)), vp(env.out(1)))
        return env.lib.mav_lk_track_err_dev(*a, 4, vp(d["n"]), C.byref(p), flags, vp(env.out(0)), vp(env.out(1)), vp(env.out(2)))
    return run


def iv_good_features(which, max_corners=50):
    def run(env):
        from mavflow import _lib
        d, p, sc = _ydev(env), _lib.gftt_defaults(), _lib.corner_score(True, 0.04)
        p.max_corners = max_corners
        gray, mask = env.y["prev"][1], env.y["sky"][0]
        out, n = np.empty((50, 2), np.float32), C.c_int()
        if which == "host":
            return env.lib.mav_good_features(env.h, p_(gray), C.byref(p), p_(out), C.byref(n))
        if which == "ex":
            return env.lib.mav_good_features_ex(env.h, p_(gray), p_(mask), C.byref(p), p_(out), C.byref(n))
        if which == "score":
            return env.lib.mav_good_features_score(env.h, p_(gray), p_(mask), C.byref(p), C.byref(sc), p_(out), C.byref(n))
        if which == "dev":
            return env.lib.mav_good_features_dev(env.h, vp(d["prev"]), C.byref(p), p_(out), C.byref(n))
        if which == "ex_dev":
            return env.lib.mav_good_features_ex_dev(env.h, vp(d["prev"]), vp(d["sky"]), C.byref(p), vp(env.out(0)), vp(env.out(1)))
        return env.lib.mav_good_features_score_dev(env.h, vp(d["prev"]), vp(d["sky"]), C.byref(p), C.byref(sc), vp(env.out(0)), vp(env.out(1)))
    return run


def iv_stage_polyexp(k=0):
    def run(env):
        I, R = np.ascontiguousarray(env.y["prev"][0], np.float32), np.empty((5, H, W), np.float32)
        return env.lib.mav_stage_polyexp(env.h, p_(I), k, p_(R))
    return run


def iv_upload_download(env):
    """every copy entry point once, between the interveners' own blocks and host arrays"""
    lib, src = env.lib, np.arange(4096, dtype=np.uint8)
    dst, back = env.out(5), np.empty(4096, np.uint8)
    pin = C.c_void_p()
    rcs = [lib.mav_host_alloc(env.h, C.c_size_t(4096), C.byref(pin))]
    C.memmove(pin, p_(src), 4096)
    rcs += [lib.mav_memcpy_h2d(env.h, vp(dst), p_(src), C.c_size_t(4096)), lib.mav_upload_async(env.h, vp(dst), pin, C.c_size_t(4096)),
            lib.mav_upload_async_unordered(env.h, vp(dst + 4096), pin, C.c_size_t(4096)), lib.mav_upload_fence(env.h)]
    srcs = (C.c_void_p * 2)(p_(src), p_(src))
    rcs += [lib.mav_upload_gather(env.h, vp(dst + 8192), srcs, 2, C.c_size_t(4096), 1), lib.mav_upload_fence(env.h),
            lib.mav_download_async(env.h, pin, vp(dst), C.c_size_t(4096)), lib.mav_sync(env.h),
            lib.mav_memcpy_d2h(env.h, p_(back), vp(dst), C.c_size_t(4096)), lib.mav_host_free(env.h, pin)]
    assert back.tobytes() == src.tobytes()
    return next((r for r in rcs if r != OK), OK)


def iv_markers(env):
    lib, m, done = env.lib, C.c_void_p(), C.c_int()
    rcs = [lib.mav_marker_create(env.h, C.byref(m)), lib.mav_marker_record(env.h, m), lib.mav_marker_wait(env.h, m),
           lib.mav_marker_query(env.h, m, C.byref(done)), lib.mav_marker_destroy(env.h, m)]
    return next((r for r in rcs if r != OK), OK)


def iv_dev_alloc(env):
    q = C.c_void_p()
    rc = env.lib.mav_dev_alloc(env.h, C.c_size_t(1 << 16), C.byref(q))
    return rc if rc != OK else env.lib.mav_dev_free(env.h, q)


def iv_timer(env):
    ms = C.c_float()
    rc = env.lib.mav_timer_start(env.h)
    return rc if rc != OK else env.lib.mav_timer_stop(env.h, C.byref(ms))


def iv_profile(env):
    lib, n, busy = env.lib, C.c_int(0), C.c_double()
    rcs = [lib.mav_profile_enable(env.h, 1), lib.mav_profile_enable(env.h, 0), lib.mav_profile_intervals(env.h, C.byref(n), None, None, None, None),
           lib.mav_profile_busy(env.h, b"phi", C.byref(busy))]
    names, tot, cnt, k = (C.c_char_p * 64)(), (C.c_double * 64)(), (C.c_long * 64)(), C.c_int(64)
    rcs.append(lib.mav_profile_get(env.h, C.byref(k), names, tot, cnt))
    return next((r for r in rcs if r != OK), OK)


def iv_queries(env):
    """the entry points that only report: nothing of them reaches the device"""
    lib, ctx = env.lib, env.ctx
    v, w, buf, a, b, ks, sg = C.c_long(), C.c_int(), C.create_string_buffer(8192), C.c_int(), C.c_int(), C.c_int(), C.c_double()
    st, hist = np.zeros(2, np.uint32), np.zeros(104, np.uint32)
    rcs = [lib.mav_get_option(env.h, b"group", C.byref(v)), lib.mav_get_window(env.h, C.byref(w)), lib.mav_schedule_info(env.h, B, buf, C.c_size_t(8192)),
           lib.mav_schedule_info_ex(env.h, B, 2, buf, C.c_size_t(8192)), lib.mav_mem_info(env.h, None, None, None, None),
           lib.mav_layer_dims(env.h, 0, C.byref(a), C.byref(b), C.byref(ks), C.byref(sg)), lib.mav_pyramid_dims(env.h, C.c_double(1.5), 0, C.byref(a), C.byref(b)),
           lib.mav_lk_level_dims(env.h, 1, C.byref(a), C.byref(b)), lib.mav_worker_drain(env.h), lib.mav_worker_wait_enqueued(env.h, C.c_uint64(0)),
           lib.mav_gftt_last_pick(env.h, p_(st)), lib.mav_lk_last_iterations(env.h, p_(hist))]
    assert lib.mav_num_layers(env.h) == 1 and lib.mav_pyramid_levels(env.h, C.c_double(1.5)) >= 1 and lib.mav_stream(env.h) and lib.mav_device_count() >= 1
    return next((r for r in rcs if r != OK), OK)


def iv_membw(env):
    g = C.c_double()
    return env.lib.mav_membw_probe(env.h, C.c_size_t(1 << 20), 1, C.byref(g))


def iv_batch_above(call):
    """a host-pointer call with batch = max_batch + 1, which HostCall::fresh refuses before it drops anything (check_dev_call is its first
    line).  call(lib, h, n, u8, f32, f64): the entry point on zero-filled arrays that are big enough for n pairs, though none is read"""
    def run(env):
        n = B + 1
        u8, f32, f64 = np.zeros((n, H, W, 3), np.uint8), np.zeros((n, H, W, 2), np.float32), np.zeros((n, H, W, 2), np.float64)
        return call(env.lib, env.h, n, p_(u8), p_(f32), p_(f64))
    return run


def iv_colormap_null(env):
    """mav_colormap_jet judges nothing but its pointers (any n is a length): the NULL it refuses in its first line, before fresh()"""
    bgr = np.zeros((B, H, W, 3), np.uint8)
    return env.lib.mav_colormap_jet(env.h, None, C.c_size_t(N0), p_(bgr))


def _b(fn):
    """a binding call on the alternative inputs as a form's run"""
    return lambda env: code(fn, env.ctx, env.y)


def _stage_flow_hooks(ctx, y):
    """the Farneback stage hooks on layer 0 (HostCall::fresh_layer each)"""
    a, b = y["prev"][0], y["next"][0]
    I0, I1 = ctx.stage_blur_resize(a, 0), ctx.stage_blur_resize(b, 0, two_pass=True)
    ctx.stage_blur_resize(a.astype(np.uint16), 0)
    R0, R1 = ctx.stage_polyexp(I0, 0), ctx.stage_polyexp(I1, 0)
    M = ctx.stage_update_matrices(R0, R1, y["flow32"][0], 0)
    ctx.stage_update_matrices_from(R0, R1, None, 0)
    ctx.stage_initial_flow(y["flow32"][0], 0)
    ctx.stage_blur_iter(R0, R1, M, 0)
    ctx.stage_coefficients(0)


def _stage_sparse_hooks(ctx, y):
    a = y["prev"][0]
    ctx.stage_lk_pyramid(a, 1), ctx.stage_lk_scharr(a, 0), ctx.stage_min_eigen(a), ctx.stage_corner_response(a, useHarrisDetector=True)
    ctx.stage_corner_pick(np.array([(0x3F800000 << 32) | 70, (0x40000000 << 32) | 900], np.uint64))


def _remap(ctx, y):
    mx, my = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) - 0.25)
    ctx.stage_remap_linear(y["flow32"][0], np.ascontiguousarray(mx), np.ascontiguousarray(my))


def F(name, entry, rule, run, refused=None, leaves=(), flow=None):
    return Form(name, entry, rule, run, refused, frozenset(leaves), flow)


OWN, CTX = True, False       # Form.flow[1]: the flow lands in env.out(3) / in a block of the context's (staging)


FORMS = [
    # -- the two sequences the code was read for, and what forwards to them
    F("mav_ransac", "mav_ransac", "private", iv_ransac()),
    F("mav_ransac refused(count=5000)", "mav_ransac", "private", iv_ransac(5000), ERR_ARG),
    F("mav_detect_dev", "mav_detect_dev", "private", iv_detect_dev(N_PAIRS), leaves=("render", "roc")),
    F("mav_detect_dev refused(n_pairs=0, other omega)", "mav_detect_dev", "private", iv_detect_dev(0), ERR_ARG),
    F("mav_process_batch_dev", "mav_process_batch_dev", "flow", iv_process_batch_dev(N_PAIRS), leaves=("render", "roc", "flow"), flow=("plain", OWN)),
    F("mav_process_batch_dev refused(n_pairs=5000)", "mav_process_batch_dev", "flow", iv_process_batch_dev(5000), ERR_ARG),
    F("mav_frame_step_dev", "mav_frame_step_dev", "flow", iv_frame_step_dev(), leaves=("render", "roc", "flow"), flow=("plain", OWN)),
    F("mav_frame_step_dev refused(n=0)", "mav_frame_step_dev", "flow", iv_frame_step_dev(n=0), ERR_ARG),
    F("mav_frame_step_dev refused(detection only, n_pairs=0, other omega)", "mav_frame_step_dev", "flow", iv_frame_step_dev(n_pairs=0, compute_flow=0), ERR_ARG),
    F("mav_frame_step_dev refused(compute flow, n_pairs=0)", "mav_frame_step_dev", "flow", iv_frame_step_dev(n_pairs=0), ERR_ARG, flow=("plain", OWN)),
    F("mav_frame_step_post+wait", "mav_frame_step_post", "flow", iv_frame_step_post, leaves=("render", "roc", "flow"), flow=("plain", OWN)),
    F("mav_frame_step_post refused(n_gather=-1)", "mav_frame_step_post", "flow", iv_frame_step_post_refused, ERR_ARG),
    F("mav_frame_step_wait refused(ticket never posted)", "mav_frame_step_wait", "state", iv_frame_step_wait_refused, ERR_ARG),
    # -- host-pointer calls: HostCall::fresh
    F("mav_detect", "mav_detect", "fresh", iv_host_detect(N_PAIRS), leaves=("render", "roc", "masks")),
    F("mav_detect refused(n_pairs=0)", "mav_detect", "fresh", iv_host_detect(0), ERR_ARG),
    F("mav_detect refused(batch above max_batch)", "mav_detect", "fresh", iv_host_detect(N_PAIRS, B + 1), ERR_ARG),
    F("mav_process_batch", "mav_process_batch", "fresh+flow", iv_host_process_batch(N_PAIRS), leaves=("render", "roc", "masks"), flow=("plain", CTX)),
    F("mav_process_batch refused(n_pairs=0)", "mav_process_batch", "fresh+flow", iv_host_process_batch(0), ERR_ARG),
    F("mav_foe_dense", "mav_foe_dense", "fresh", iv_foe_dense(False, N_PAIRS)),
    F("mav_foe_dense refused(n_pairs=0)", "mav_foe_dense", "fresh", iv_foe_dense(False, 0), ERR_ARG),
    F("mav_foe_dense_f32", "mav_foe_dense_f32", "fresh", iv_foe_dense(True, N_PAIRS)),
    F("mav_foe_dense_f32 refused(n_pairs=4097)", "mav_foe_dense_f32", "fresh", iv_foe_dense(True, 4097), ERR_ARG),
    F("mav_phi_mask", "mav_phi_mask", "fresh", iv_phi_mask(False), leaves=("roc", "masks")),
    F("mav_phi_mask refused(batch above max_batch)", "mav_phi_mask", "fresh", iv_phi_mask(False, B + 1), ERR_ARG),
    F("mav_phi_mask_f32", "mav_phi_mask_f32", "fresh", iv_phi_mask(True), leaves=("roc", "masks")),
    F("mav_phi_mask_f32 refused(batch=0)", "mav_phi_mask_f32", "fresh", iv_phi_mask(True, 0), ERR_ARG),
    F("mav_farneback", "mav_farneback", "fresh+flow", _b(lambda c, y: c.farneback(y["prev"], y["next"])), flow=("plain", CTX)),
    F("mav_farneback refused(batch above max_batch)", "mav_farneback", "fresh+flow",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_farneback(h, u8, u8, n, f32)), ERR_ARG),
    F("mav_farneback_init", "mav_farneback_init", "fresh+flow", _b(lambda c, y: c.farneback(y["prev"], y["next"], initial_flow=y["flow32"])), flow=("init", CTX)),
    F("mav_farneback_init refused(batch above max_batch)", "mav_farneback_init", "fresh+flow",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_farneback_init(h, u8, u8, n, f32, f32)), ERR_ARG),
    F("mav_farneback_ex", "mav_farneback_ex", "fresh+flow", iv_farneback_ex(), flow=("plain", CTX)),
    F("mav_farneback_ex refused(depth=1)", "mav_farneback_ex", "fresh+flow", iv_farneback_ex(1), ERR_ARG),
    F("mav_derotate", "mav_derotate", "fresh", _b(lambda c, y: c.derotate(y["flow32"], y["omega"], y["dt"]))),
    F("mav_derotate refused(batch above max_batch)", "mav_derotate", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_derotate(h, f32, f64, f64, n, f64)), ERR_ARG),
    F("mav_bgr2gray", "mav_bgr2gray", "fresh", _b(lambda c, y: c.bgr2gray(y["bgr"]))),
    F("mav_bgr2gray refused(batch above max_batch)", "mav_bgr2gray", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_bgr2gray(h, u8, n, u8)), ERR_ARG),
    F("mav_bbox", "mav_bbox", "fresh", _b(lambda c, y: c.bbox(y["sky"]))),
    F("mav_bbox refused(batch above max_batch)", "mav_bbox", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_bbox(h, u8, n, f64)), ERR_ARG),
    F("mav_window_max", "mav_window_max", "fresh", _b(lambda c, y: c.window_max(y["sky"]))),
    F("mav_window_max refused(batch above max_batch)", "mav_window_max", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_window_max(h, u8, n, f64)), ERR_ARG),
    F("mav_analyze_pyramid", "mav_analyze_pyramid", "fresh", iv_analyze_pyramid()),
    F("mav_analyze_pyramid refused(scale=1)", "mav_analyze_pyramid", "fresh", iv_analyze_pyramid(1.0), ERR_ARG),
    F("mav_optimize_window", "mav_optimize_window", "fresh", _b(lambda c, y: c.optimize_window(y["sky"], np.array([[4, 4, 16, 16]] * B, np.int32)))),
    F("mav_tpr_fpr_counts", "mav_tpr_fpr_counts", "fresh", iv_tpr_fpr(False)),
    F("mav_tpr_fpr_counts refused(mask_value=0)", "mav_tpr_fpr_counts", "fresh", iv_tpr_fpr(False, 0), ERR_ARG),
    F("mav_render", "mav_render", "fresh", iv_render(False)),
    F("mav_render refused(batch above max_batch)", "mav_render", "fresh", iv_render(False, B + 1), ERR_ARG),
    F("mav_flow_to_color", "mav_flow_to_color", "fresh", _b(lambda c, y: c.flow_to_color(y["flow32"]))),
    F("mav_flow_to_color refused(batch above max_batch)", "mav_flow_to_color", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_flow_to_color(h, f32, 0, n, u8)), ERR_ARG),
    F("mav_colormap_jet", "mav_colormap_jet", "fresh", _b(lambda c, y: c.colormap_jet(y["sky"]))),
    F("mav_colormap_jet refused(NULL gray)", "mav_colormap_jet", "fresh", iv_colormap_null, ERR_ARG),
    F("mav_overlay", "mav_overlay", "fresh", iv_overlay(False)),
    F("mav_overlay refused(NaN foe_gt)", "mav_overlay", "fresh", iv_overlay(False, nan=True), ERR_ARG),
    F("mav_components", "mav_components", "fresh", iv_components(False)),
    F("mav_components refused(connectivity=5)", "mav_components", "fresh", iv_components(False, 5), ERR_ARG),
    F("mav_roc_sweep", "mav_roc_sweep", "fresh", iv_roc_sweep(False)),
    F("mav_roc_sweep refused(n_angles=0)", "mav_roc_sweep", "fresh", iv_roc_sweep(False, 0), ERR_ARG),
    F("mav_history_push", "mav_history_push", "fresh", iv_history_push(False)),
    F("mav_history_push refused(depth=0)", "mav_history_push", "fresh", iv_history_push(False, 0), ERR_ARG),
    F("mav_stage_remap_linear", "mav_stage_remap_linear", "fresh", _b(_remap)),
    F("mav_png_encode", "mav_png_encode", "fresh", iv_png_encode(False)),
    F("mav_png_encode refused(channels=2)", "mav_png_encode", "fresh", iv_png_encode(False, 2), ERR_ARG),
    F("mav_find_homography", "mav_find_homography", "fresh", iv_find_homography(False)),
    F("mav_find_homography refused(n=3)", "mav_find_homography", "fresh", iv_find_homography(False, 3), ERR_ARG),
    F("mav_flow_homography", "mav_flow_homography", "fresh", iv_flow_homography(False)),
    F("mav_flow_homography refused(n=3)", "mav_flow_homography", "fresh", iv_flow_homography(False, 3), ERR_ARG),
    F("mav_global_motion", "mav_global_motion", "fresh", iv_global_motion(False), leaves=("motion",)),
    F("mav_global_motion refused(scale=1)", "mav_global_motion", "fresh", iv_global_motion(False, 1.0), ERR_ARG),
    F("mav_global_motion_batch", "mav_global_motion_batch", "fresh+flow", iv_motion_batch(False), leaves=("motion", "flow"), flow=("plain", CTX)),
    F("mav_global_motion_batch refused(sample outside)", "mav_global_motion_batch", "fresh+flow", iv_motion_batch(False, True), ERR_ARG),
    F("mav_stage_phi_mask", "mav_stage_phi_mask", "fresh", _b(lambda c, y: c.stage_phi_mask(y["flow32"], y["foe"], omega=y["omega"], dt=y["dt"], sky=y["sky"]))),
    F("mav_stage_phi_mask refused(batch above max_batch)", "mav_stage_phi_mask", "fresh",
      iv_batch_above(lambda lib, h, n, u8, f32, f64: lib.mav_stage_phi_mask(h, f32, f64, f64, f64, u8, n, None, None, u8, u8, None)), ERR_ARG),
    F("mav_stage_polyexp refused(layer 99)", "mav_stage_polyexp", "fresh", iv_stage_polyexp(99), ERR_ARG),
    F("Farneback stage hooks", "mav_stage_blur_resize", "fresh", _b(_stage_flow_hooks)),
    F("mav_stage_pyramid_level", "mav_stage_pyramid_level", "fresh", _b(lambda c, y: c.pyramid_level(y["sky"][0], 0))),
    # -- device-pointer calls that compute flow: farneback_run's tail
    F("mav_farneback_dev", "mav_farneback_dev", "flow", iv_farneback_dev(), leaves=("flow",), flow=("plain", OWN)),
    F("mav_farneback_dev refused(batch above max_batch)", "mav_farneback_dev", "flow", iv_farneback_dev(B + 1), ERR_ARG),
    F("mav_farneback_init_dev", "mav_farneback_init_dev", "flow", iv_farneback_init_dev(), leaves=("flow",), flow=("init", OWN)),
    F("mav_farneback_init_dev refused(batch=0)", "mav_farneback_init_dev", "flow", iv_farneback_init_dev(0), ERR_ARG),
    F("mav_farneback_ex_dev", "mav_farneback_ex_dev", "flow", iv_farneback_ex_dev(), leaves=("flow",), flow=("plain", OWN)),
    F("mav_farneback_ex_dev refused(depth=1)", "mav_farneback_ex_dev", "flow", iv_farneback_ex_dev(1), ERR_ARG),
    F("mav_global_motion_batch_dev", "mav_global_motion_batch_dev", "flow", iv_motion_batch(True), leaves=("motion", "flow"), flow=("plain", OWN)),
    F("mav_global_motion_batch_dev refused(sample outside)", "mav_global_motion_batch_dev", "flow", iv_motion_batch(True, True), ERR_ARG),
    # -- device-pointer calls on caller-owned memory and private workspaces
    F("mav_global_motion_dev", "mav_global_motion_dev", "private", iv_global_motion(True), leaves=("motion",)),
    F("mav_global_motion_dev refused(scale=1)", "mav_global_motion_dev", "private", iv_global_motion(True, 1.0), ERR_ARG),
    F("mav_global_motion_step_dev", "mav_global_motion_step_dev", "private", iv_motion_step(), leaves=("motion",)),
    F("mav_global_motion_step_dev(H=NULL)", "mav_global_motion_step_dev", "private", iv_motion_step(own_H=False), leaves=("motion",)),
    F("mav_global_motion_step_dev refused(sample outside)", "mav_global_motion_step_dev", "private", iv_motion_step(True), ERR_ARG),
    F("mav_find_homography_dev", "mav_find_homography_dev", "private", iv_find_homography(True)),
    F("mav_find_homography_dev refused(n=3)", "mav_find_homography_dev", "private", iv_find_homography(True, 3), ERR_ARG),
    F("mav_flow_homography_dev", "mav_flow_homography_dev", "private", iv_flow_homography(True)),
    F("mav_flow_homography_dev refused(sample outside)", "mav_flow_homography_dev", "private", iv_flow_homography(True, outside=True), ERR_ARG),
    F("mav_bgr2gray_dev", "mav_bgr2gray_dev", "private", lambda env: env.lib.mav_bgr2gray_dev(env.h, vp(_ydev(env)["bgr"]), B, vp(env.out(0)))),
    F("mav_bgr2gray_dev refused(batch=0)", "mav_bgr2gray_dev", "private", lambda env: env.lib.mav_bgr2gray_dev(env.h, vp(_ydev(env)["bgr"]), 0, vp(env.out(0))), ERR_ARG),
    F("mav_render_dev", "mav_render_dev", "private", iv_render(True)),
    F("mav_render_dev refused(batch=0)", "mav_render_dev", "private", iv_render(True, 0), ERR_ARG),
    F("mav_overlay_dev", "mav_overlay_dev", "private", iv_overlay(True)),
    F("mav_overlay_dev refused(radius=-1)", "mav_overlay_dev", "private", iv_overlay(True, -1), ERR_ARG),
    F("mav_tpr_fpr_counts_dev", "mav_tpr_fpr_counts_dev", "private", iv_tpr_fpr(True)),
    F("mav_tpr_fpr_counts_dev refused(mask_value=0)", "mav_tpr_fpr_counts_dev", "private", iv_tpr_fpr(True, 0), ERR_ARG),
    F("mav_components_dev", "mav_components_dev", "private", iv_components(True)),
    F("mav_components_dev refused(connectivity=5)", "mav_components_dev", "private", iv_components(True, 5), ERR_ARG),
    F("mav_roc_sweep_dev", "mav_roc_sweep_dev", "private", iv_roc_sweep(True)),
    F("mav_roc_sweep_dev refused(n_angles=0)", "mav_roc_sweep_dev", "private", iv_roc_sweep(True, 0), ERR_ARG),
    F("mav_png_encode_dev", "mav_png_encode_dev", "private", iv_png_encode(True)),
    F("mav_png_encode_dev refused(channels=2)", "mav_png_encode_dev", "private", iv_png_encode(True, 2), ERR_ARG),
    F("mav_history_push_dev", "mav_history_push_dev", "private", iv_history_push(True)),
    F("mav_history_push_dev refused(depth=0)", "mav_history_push_dev", "private", iv_history_push(True, 0), ERR_ARG),
    F("mav_allgather_results refused(no communicator)", "mav_allgather_results", "private",
      lambda env: env.lib.mav_allgather_results(env.h, None, vp(env.out(0)), C.c_size_t(32), vp(env.out(1))), ERR_ARG),
    # -- the sparse path: its own workspace (LkState)
    F("mav_lk_track", "mav_lk_track", "private", iv_lk_track()),
    F("mav_lk_track refused(win_w=4)", "mav_lk_track", "private", iv_lk_track(4), ERR_ARG),
    F("mav_lk_track_err", "mav_lk_track_err", "private", iv_lk_track_err()),
    F("mav_lk_track_err refused(flags=1)", "mav_lk_track_err", "private", iv_lk_track_err(1), ERR_ARG),
    F("mav_lk_track_dev", "mav_lk_track_dev", "private", iv_lk_dev("dev")),
    F("mav_lk_track_dev refused(win_w=4)", "mav_lk_track_dev", "private", iv_lk_dev("dev", win=4), ERR_ARG),
    F("mav_lk_track_ex_dev", "mav_lk_track_ex_dev", "private", iv_lk_dev("ex")),
    F("mav_lk_track_ex_dev refused(win_w=4)", "mav_lk_track_ex_dev", "private", iv_lk_dev("ex", win=4), ERR_ARG),
    F("mav_lk_track_err_dev", "mav_lk_track_err_dev", "private", iv_lk_dev("err")),
    F("mav_lk_track_err_dev refused(flags=1)", "mav_lk_track_err_dev", "private", iv_lk_dev("err", flags=1), ERR_ARG),
    F("mav_lk_track_err_dev refused(win_w=4)", "mav_lk_track_err_dev", "private", iv_lk_dev("err", win=4), ERR_ARG),
    F("mav_good_features", "mav_good_features", "private", iv_good_features("host")),
    F("mav_good_features refused(max_corners=0)", "mav_good_features", "private", iv_good_features("host", 0), ERR_ARG),
    F("mav_good_features_ex", "mav_good_features_ex", "private", iv_good_features("ex")),
    F("mav_good_features_ex refused(max_corners=0)", "mav_good_features_ex", "private", iv_good_features("ex", 0), ERR_ARG),
    F("mav_good_features_score", "mav_good_features_score", "private", iv_good_features("score")),
    F("mav_good_features_score refused(max_corners=0)", "mav_good_features_score", "private", iv_good_features("score", 0), ERR_ARG),
    F("mav_good_features_dev", "mav_good_features_dev", "private", iv_good_features("dev")),
    F("mav_good_features_dev refused(max_corners=0)", "mav_good_features_dev", "private", iv_good_features("dev", 0), ERR_ARG),
    F("mav_good_features_ex_dev", "mav_good_features_ex_dev", "private", iv_good_features("ex_dev")),
    F("mav_good_features_ex_dev refused(max_corners=0)", "mav_good_features_ex_dev", "private", iv_good_features("ex_dev", 0), ERR_ARG),
    F("mav_good_features_score_dev", "mav_good_features_score_dev", "private", iv_good_features("score_dev")),
    F("mav_good_features_score_dev refused(max_corners=0)", "mav_good_features_score_dev", "private", iv_good_features("score_dev", 0), ERR_ARG),
    F("sparse stage hooks", "mav_stage_lk_pyramid", "private", _b(_stage_sparse_hooks)),
    # -- options and lifecycle
    F("mav_set_option", "mav_set_option", "state", lambda env: env.lib.mav_set_option(env.h, b"phi_screen", C.c_long(1))),
    F("mav_set_option refused(unknown name)", "mav_set_option", "state", lambda env: env.lib.mav_set_option(env.h, b"no_such_option", C.c_long(1)), ERR_ARG),
    F("mav_set_window", "mav_set_window", "state", lambda env: env.lib.mav_set_window(env.h, 0)),
    F("mav_set_window refused(window=7)", "mav_set_window", "state", lambda env: env.lib.mav_set_window(env.h, 7), ERR_ARG),
    F("mav_roc_arm", "mav_roc_arm", "state", iv_roc_arm()),
    F("mav_roc_arm refused(off_table=4)", "mav_roc_arm", "state", iv_roc_arm(4), ERR_ARG),
    F("mav_profile_enable", "mav_profile_enable", "state", iv_profile),
    F("mav_timer_start+stop", "mav_timer_start", "state", iv_timer),
    F("mav_sync", "mav_sync", "state", lambda env: env.lib.mav_sync(env.h)),
    F("mav_dev_alloc+free", "mav_dev_alloc", "state", iv_dev_alloc),
    F("mav_history_create+destroy", "mav_history_create", "state", iv_history_create()),
    F("mav_history_create refused(length=2)", "mav_history_create", "state", iv_history_create(2), ERR_ARG),
    F("mav_history_reset+info", "mav_history_reset", "state", iv_history_misc),
    F("copies", "mav_upload_gather", "state", iv_upload_download),
    F("markers", "mav_marker_create", "state", iv_markers),
    F("queries", "mav_mem_info", "state", iv_queries),
    F("mav_membw_probe", "mav_membw_probe", "state", iv_membw),
]
# Entry points a form above calls besides the one it is named for (helpers that run several in one go)
ALSO = {
    "Farneback stage hooks": ("mav_stage_blur_resize_two_pass", "mav_stage_blur_resize_ex", "mav_stage_polyexp", "mav_stage_update_matrices",
                              "mav_stage_update_matrices_from", "mav_stage_initial_flow", "mav_stage_blur_iter", "mav_stage_coefficients"),
    "sparse stage hooks": ("mav_stage_lk_scharr", "mav_stage_min_eigen", "mav_stage_corner_response", "mav_stage_corner_pick"),
    "mav_timer_start+stop": ("mav_timer_stop",),
    "mav_dev_alloc+free": ("mav_dev_free",),
    "mav_history_create+destroy": ("mav_history_destroy",),
    "mav_history_reset+info": ("mav_history_info",),
    "mav_profile_enable": ("mav_profile_get", "mav_profile_busy", "mav_profile_intervals"),
    "copies": ("mav_host_alloc", "mav_host_free", "mav_memcpy_h2d", "mav_memcpy_d2h", "mav_upload_async", "mav_upload_async_unordered",
               "mav_upload_fence", "mav_download_async"),
    "markers": ("mav_marker_record", "mav_marker_wait", "mav_marker_query", "mav_marker_destroy"),
    "queries": ("mav_get_option", "mav_get_window", "mav_schedule_info", "mav_schedule_info_ex", "mav_num_layers", "mav_layer_dims", "mav_pyramid_levels",
                "mav_pyramid_dims", "mav_lk_level_dims", "mav_worker_drain", "mav_worker_wait_enqueued", "mav_gftt_last_pick", "mav_lk_last_iterations",
                "mav_stream", "mav_device_count"),
}
# Entry points that take no context or cannot touch the device
EXEMPT = {
    "mav_fb_defaults": "fills a struct", "mav_foe_defaults": "fills a struct", "mav_thr_defaults": "fills a struct", "mav_cc_defaults": "fills a struct",
    "mav_history_defaults": "fills a struct", "mav_gftt_defaults": "fills a struct", "mav_lk_defaults": "fills a struct",
    "mav_corner_score_defaults": "fills a struct", "mav_last_error": "thread-local string", "mav_png_unfilter": "host memory, no context",
    "mav_png_bound": "arithmetic, no context", "mav_history_schedule": "pure host, no context", "mav_runtime_info": "versions, no context",
    "mav_comm_unique_id": "RCCL bootstrap, no context", "mav_comm_init": "RCCL bootstrap: a second rank's business, nothing of the context's device state",
    "mav_comm_count": "a communicator, no context", "mav_comm_destroy": "a communicator, no context",
    "mav_create": "makes the context: nothing is resident yet", "mav_destroy": "ends the context: nothing can be read afterwards",
}
GROUPS = {"a": lambda i: i % 3 == 0, "b": lambda i: i % 3 == 1, "c": lambda i: i % 3 == 2}      # the forms in three thirds, to keep a test short


def intervener_entries() -> dict:
    """header function -> the forms that call it"""
    m = {}
    for f in FORMS:
        for e in (f.entry,) + tuple(ALSO.get(f.name, ())):
            m.setdefault(e, []).append(f.name)
    return m

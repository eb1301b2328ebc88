"""TEST INFRASTRUCTURE -- the frames, rings, policies, fields and pointers at which every form of the flow history
(csrc/kernels_history.hip and its entry points in csrc/mavflow.cpp) is held to the numpy restatement tests/history_ref.py by
tests/test_gpu_history.py, and the forms each case takes there.  The counterpart of tests/motion_cases.py for this feature.

Two kinds of forms.  What the kernels DISPATCH on -- template instances (ring element, input element, axes order, output form), the
grid-stride loops past the cap of 4096 workgroups (one pixel per thread: no pair, no tail form), the vector access a caller's
pointer allows -- is restated below as predicates that cite the lines they mirror.  Which way an ELEMENT of a
remap goes -- interior, one of the borders, a corner, wholly outside on each side, rounding ties, non-finite and far-away coordinates,
a NaN tap under a zero weight -- is read from history_ref's trace of the case's own inputs: tests/test_history_cases_cpu.py runs the
restatement on every case and fails when a form of FORMS is reached by no case, or when a case does not reach what it names."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import history_ref as R

WG = 256                      # HIST_WG: threads of a workgroup of every kernel
PX = 1                        # HIST_PX: pixels per thread of k_history_trace
CAP = 4096                    # HIST_CAP: most workgroups of a launch (history_blocks)
MAX_LENGTH = 64               # MAV_HISTORY_MAX_LENGTH
STAGED_ALIGN = 256            # a staging block is a hipMalloc allocation of its own: aligned to at least this

FORMS = {
    # template instances and entry-point policies
    "ring": {"f32", "f64"},
    "input": {"f32->f32", "f32->f64", "f64->f64"},
    "axes": {"reference", "xy"},
    "out": {"reference", "flow"},
    "count": {"1", ">1", ">1:short-last-call"},
    # the schedule (mav_history_schedule) over the case's pushes
    "schedule": {"h<L-2", "h=L-2", "h=L-1", "slot-overwritten"},
    # one remap element (history_ref's trace)
    "tap": {"interior", "sx=-1", "sx=W-1", "sy=-1", "sy=H-1", "corner", "outside:left", "outside:right", "outside:top", "outside:bottom"},
    "coord": {"tie-down", "tie-up", "negative-fraction", "nan", "+inf", "-inf", "past-int32", "beyond+32768", "beyond-32768",
              "nan-tap-zero-weight"},
    "frame": {"1x1", "1xN", "Nx1", "few-pixels", "ragged"},
    # the kernels' index walk
    "trace.stride": {"1", ">1", ">1:partial-last"},
    "put.stride": {"1", ">1"},
    "put.access": {"vec", "scalar"},
    "out.access": {"vec", "scalar"},
    "ptr": {"staged", "caller:aligned", "caller:flow+4B", "caller:flow+8B", "caller:out+8B", "caller:out+4B"},
}


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------
def history_blocks(items: int) -> int:
    """kernels_history.hip history_blocks(): `need = (items + 255) / 256; need < 4096 ? (need ? need : 1) : 4096`."""
    need = (items + WG - 1) // WG
    return need if 0 < need < CAP else (1 if need == 0 else CAP)


def stride_forms(items: int) -> set:
    """`for (q = blockIdx.x * 256 + threadIdx.x; q < items; q += gridDim.x * 256)`: the iterations thread 0 takes, and whether the
    last one leaves threads without an item."""
    T = history_blocks(items) * WG
    iters = (items + T - 1) // T
    if iters <= 1:
        return {"1"}
    return {">1"} | ({">1:partial-last"} if items % T else set())


def trace_items(n0: int) -> int:
    """launch_trace_t: `history_blocks((W * H + HIST_PX - 1) / HIST_PX)`: a workgroup takes HIST_WG * HIST_PX pixels per step."""
    return (n0 + PX - 1) // PX


def second_iteration_pixel() -> int:
    """The first pixel a capped trajectory grid reaches in its second iteration: thread 0 of workgroup 0 at base = 4096 * 256."""
    return CAP * WG * PX


def put_vec(elem: int, off: int) -> bool:
    """k_history_put: `vec = ((uintptr_t)src & (2 * sizeof(S) - 1)) == 0`; field t of a call starts t * W * H * 2 elements further:
    a multiple of the pair, so only the caller's offset decides."""
    return off % (2 * elem) == 0


def out_vec(elem: int, off: int) -> bool:
    """k_history_trace: `vec = ((uintptr_t)out & (sizeof(O) - 1)) == 0` with O the output pair."""
    return off % (2 * elem) == 0


ELEM = {"f32": 4, "f64": 8}
NP = {"f32": np.float32, "f64": np.float64}
OUT_ELEM = {"reference": 8, "flow": 4}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One history driven through `pushes` fields (default 2 L + 1: every slot is overwritten).  entry "host": mav_history_push on
    staged pointers; "dev": mav_history_push_dev on the caller's buffers at the given byte offsets.  count: fields per call (the last
    call takes what is left)."""
    name: str
    W: int
    H: int
    L: int = 4
    ring: str = "f32"
    inp: str = "f32"
    axes: str = "reference"
    out: str = "reference"
    kind: str = "planted"
    pushes: int = 0
    count: int = 1
    entry: str = "host"
    flow_off: int = 0
    out_off: int = 0
    expects: frozenset = frozenset()

    @property
    def n0(self):
        return self.W * self.H

    @property
    def n_pushes(self):
        return self.pushes or 2 * self.L + 1


def _frame_form(W, H):
    if W == 1 and H == 1:
        return "1x1"
    if H == 1:
        return "1xN"
    if W == 1:
        return "Nx1"
    return "few-pixels" if W * H <= 32 else "ragged"


def static_forms(c: Case) -> set:
    """{(group, form)} the case reaches by its shape and policies, from the predicates alone."""
    out = {("ring", c.ring), ("input", f"{c.inp}->{c.ring}"), ("axes", c.axes), ("out", c.out), ("frame", _frame_form(c.W, c.H))}
    out.add(("count", "1" if c.count == 1 else ">1"))
    if c.count > 1 and c.n_pushes % c.count:
        out.add(("count", ">1:short-last-call"))
    h = 0
    for i in range(c.n_pushes):
        out.add(("schedule", "h<L-2" if h < c.L - 2 else ("h=L-2" if h == c.L - 2 else "h=L-1")))
        if i >= c.L:
            out.add(("schedule", "slot-overwritten"))
        h = (h + 1) % c.L
    out |= {("trace.stride", f) for f in stride_forms(trace_items(c.n0))}
    out |= {("put.stride", f) for f in stride_forms(c.n0) - {">1:partial-last"}}
    out.add(("put.access", "vec" if put_vec(ELEM[c.inp], c.flow_off) else "scalar"))
    out.add(("out.access", "vec" if out_vec(OUT_ELEM[c.out], c.out_off) else "scalar"))
    if c.entry == "host":
        out.add(("ptr", "staged"))
    else:
        if not c.flow_off and not c.out_off:
            out.add(("ptr", "caller:aligned"))
        if c.flow_off:
            out.add(("ptr", f"caller:flow+{c.flow_off}B"))
        if c.out_off:
            out.add(("ptr", f"caller:out+{c.out_off}B"))
    return out


def element_forms(trace: list) -> set:
    """{(group, form)} of the remap elements of a run, from history_ref's trace."""
    out = set()
    for t in trace:
        W, H, fits, inside, sx, sy = t["W"], t["H"], t["fits"], t["inside"], t["sx"], t["sy"]
        ex, ey = (sx == -1) | (sx == W - 1), (sy == -1) | (sy == H - 1)
        found = {
            ("tap", "interior"): inside & ~ex & ~ey,
            ("tap", "corner"): inside & ex & ey,
            ("tap", "sx=-1"): inside & (sx == -1) & ~ey,
            ("tap", "sx=W-1"): inside & (sx == W - 1) & ~ey,
            ("tap", "sy=-1"): inside & (sy == -1) & ~ex,
            ("tap", "sy=H-1"): inside & (sy == H - 1) & ~ex,
            ("tap", "outside:left"): fits & (sx + 1 < 0),
            ("tap", "outside:right"): fits & (sx >= W),
            ("tap", "outside:top"): fits & (sy + 1 < 0),
            ("tap", "outside:bottom"): fits & (sy >= H),
            ("coord", "nan-tap-zero-weight"): t["nan_zero_w"],
        }
        for p, q, m in ((t["px"], t["qx"], t["mx"]), (t["py"], t["qy"], t["my"])):
            with np.errstate(all="ignore"):
                fin = np.isfinite(p)
                tie = fin & fits & (np.abs(p - np.floor(p)) == 0.5)
                found.setdefault(("coord", "tie-down"), np.zeros(p.shape, bool))
                found.setdefault(("coord", "tie-up"), np.zeros(p.shape, bool))
                found[("coord", "tie-down")] = found[("coord", "tie-down")] | (tie & (q < p))
                found[("coord", "tie-up")] = found[("coord", "tie-up")] | (tie & (q > p))
                for key, mask in ((("coord", "negative-fraction"), fits & (m > -1) & (m < 0) & ((q >> 5) == -1)),
                                  (("coord", "nan"), np.isnan(m)), (("coord", "+inf"), np.isposinf(m)), (("coord", "-inf"), np.isneginf(m)),
                                  (("coord", "past-int32"), fin & ~((p >= -2.0 ** 31) & (p < 2.0 ** 31))),
                                  (("coord", "beyond+32768"), fits & ((q >> 5) > 32767)), (("coord", "beyond-32768"), fits & ((q >> 5) < -32768))):
                    found[key] = found.get(key, np.zeros(p.shape, bool)) | mask
        out |= {k for k, m in found.items() if m.any()}
    return out


def _e(*forms):
    return frozenset(forms)


TAPS_ALL = tuple("tap=" + f for f in sorted(FORMS["tap"]))
COORDS_ALL = tuple("coord=" + f for f in sorted(FORMS["coord"]))
SCHEDULE_ALL = tuple("schedule=" + f for f in sorted(FORMS["schedule"]))
RAGGED = dict(W=37, H=23)          # 851 pixels: odd sizes, four workgroups of pixels with a partly filled last one
INSTANCES = [(ring, inp, axes, out) for ring, inps in (("f32", ("f32",)), ("f64", ("f32", "f64"))) for inp in inps
             for axes in ("reference", "xy") for out in ("reference", "flow")]
CASES = [
    # every instance of the trajectory kernel (ring x axes x out) and of the ring write (input -> ring), on the planted fields that
    # send an element every way a remap can go, over 2 L + 1 pushes
    Case(f"planted37x23_{inp}to{ring}_{axes}_{out}", **RAGGED, ring=ring, inp=inp, axes=axes, out=out,
         expects=_e(*TAPS_ALL, *COORDS_ALL, *SCHEDULE_ALL, f"ring={ring}", f"input={inp}->{ring}", f"axes={axes}", f"out={out}", "frame=ragged",    "trace.stride=1", "put.stride=1",
                    "put.access=vec", "out.access=vec", "ptr=staged", "count=1"))
    for ring, inp, axes, out in INSTANCES
] + [
    # the smallest frames: every tap of a 1 x 1 field is the one pixel or outside
    Case("tiny1x1_L3", 1, 1, L=3, expects=_e("frame=1x1",  "tap=corner", "coord=nan")),
    Case("tiny7x1", 7, 1, expects=_e("frame=1xN",   "tap=corner", "tap=sy=-1")),
    Case("tiny1x7_xy", 1, 7, axes="xy", expects=_e("frame=Nx1",  "tap=corner", "tap=sx=-1")),
    Case("tiny5x3_f64", 5, 3, ring="f64", inp="f64", expects=_e("frame=few-pixels",  
                                                                  "tap=interior", "tap=corner")),
    Case("tiny6x2_flow", 6, 2, out="flow", expects=_e("frame=few-pixels",  )),
    # a longer ring on a smooth field of a few pixels' magnitude, and several fields per call
    Case("smooth41x29_L5", 41, 29, L=5, kind="smooth", expects=_e(*SCHEDULE_ALL, "tap=interior", )),
    Case("count3_37x23", **RAGGED, count=3, expects=_e("count=>1", *SCHEDULE_ALL)),
    Case("count2_37x23_f64_flow", **RAGGED, ring="f64", inp="f32", out="flow", count=2, expects=_e("count=>1", "count=>1:short-last-call")),
    Case("count11_smooth16x16_L5", 16, 16, L=5, kind="smooth", count=11, expects=_e("count=>1",  *SCHEDULE_ALL)),
    # a caller's own pointers: aligned to the element only
    Case("dev37x23_aligned", **RAGGED, entry="dev", count=3, expects=_e("ptr=caller:aligned", "put.access=vec", "out.access=vec")),
    Case("dev37x23_flow+4B", **RAGGED, entry="dev", count=3, flow_off=4, expects=_e("ptr=caller:flow+4B", "put.access=scalar", "out.access=vec")),
    Case("dev37x23_out+8B", **RAGGED, entry="dev", count=3, out_off=8, expects=_e("ptr=caller:out+8B", "put.access=vec", "out.access=scalar")),
    Case("dev37x23_flowform_out+4B", **RAGGED, entry="dev", out="flow", axes="xy", out_off=4,
         expects=_e("ptr=caller:out+4B", "out.access=scalar", "out=flow")),
    Case("dev37x23_f64_flow+8B_out+8B", **RAGGED, entry="dev", ring="f64", inp="f64", flow_off=8, out_off=8, count=2,
         expects=_e("ptr=caller:flow+8B", "put.access=scalar", "out.access=scalar", "input=f64->f64")),
    Case("dev37x23_f32tof64_flow+4B", **RAGGED, entry="dev", ring="f64", inp="f32", flow_off=4,
         expects=_e("ptr=caller:flow+4B", "put.access=scalar", "input=f32->f64")),
    # past the cap (the only large case): 1 050 625 pixels against 4096 * 256 threads, a 3-slot ring, one push per slot
    Case("cap1025x1025_L3", 1025, 1025, L=3, kind="smooth", pushes=3,
         expects=_e("trace.stride=>1", "trace.stride=>1:partial-last", "put.stride=>1",  "schedule=h<L-2",
                    "schedule=h=L-2", "schedule=h=L-1", "tap=interior")),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LARGE = "cap1025x1025_L3"


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def targets(W: int, H: int):
    """(x, y) positions a planted field sends its pixels to, one per pixel in turn: every way a remap element can go."""
    cx, cy = (W - 1) // 2, (H - 1) // 2
    inf = np.inf
    return [(cx + 0.25, cy + 0.5), (-0.5, cy), (W - 0.5, cy), (cx, -0.5), (cx, H - 0.5), (-0.5, -0.5), (W - 0.5, H - 0.5), (-0.25, H - 0.75),
            (-1.5, cy), (W + 0.25, cy), (cx, -2.0), (cx, H + 1.0),
            (cx + 1 / 64, cy), (cx + 3 / 64, cy), (cx, cy + 1 / 64), (cx, cy + 3 / 64), (-1 / 64, cy), (-3 / 64, -1 / 64),
            (np.nan, cy), (cx, np.nan), (inf, cy), (cx, -inf), (-inf, inf), (1e30, cy), (cx, -1e30),
            (40000.5, cy), (cx, -40000.5), (-40000.5, 40000.5),
            (W - 2.0, H - 1.0), (W - 1.0, H - 2.0), (W - 2.0, H - 2.0)]           # next to the sampled field's NaN pixel, weight 0 on it


def planted(W: int, H: int, axes: str) -> np.ndarray:
    """(H, W, 2) float32: read at its own integer position (the first step of a push), the k-th pixel with even x and even y moves to
    targets[k % len].  The other pixels hold zero, so that no planted pixel has an infinity or a NaN as a (zero-weight) neighbour tap."""
    t = targets(W, H)
    f = np.zeros((H, W, 2), np.float32)
    k = 0
    with np.errstate(all="ignore"):
        for y in range(0, H, 2):
            for x in range(0, W, 2):
                tx, ty = t[k % len(t)]
                k += 1
                dr, dc = np.float32(ty - y), np.float32(tx - x)
                f[y, x] = (dr, dc) if axes == "reference" else (dc, dr)
    return f


def sampled(W: int, H: int, seed: int) -> np.ndarray:
    """(H, W, 2) float32 noise of a pixel or two, with a NaN at the last pixel and an infinity at the first."""
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 1.2, (H, W, 2)).astype(np.float32)
    f[H - 1, W - 1, 0] = np.nan
    if W * H > 1:
        f[0, 0, 1] = np.inf
    return f


def smooth(W: int, H: int, i: int) -> np.ndarray:
    """(H, W, 2) float32: a smooth field of about 2 px that changes from push to push, with a little noise."""
    rng = np.random.default_rng(1000 + i)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    u = 2.0 * np.sin(xx / 17.0 + 0.3 * i) + 0.5 * np.cos(yy / 11.0)
    v = 1.5 * np.cos(yy / 13.0 - 0.2 * i) - 0.7 * np.sin(xx / 23.0)
    return (np.stack([u, v], axis=-1) + rng.normal(0, 0.05, (H, W, 2))).astype(np.float32)


def fields_of(c: Case) -> np.ndarray:
    """(pushes, H, W, 2) of the case's input element: planted and sampled fields in turn, or the smooth sequence."""
    if c.kind == "smooth":
        f = np.stack([smooth(c.W, c.H, i) for i in range(c.n_pushes)])
    else:
        f = np.stack([planted(c.W, c.H, c.axes) if i % 2 == 0 else sampled(c.W, c.H, 10 * i + c.W) for i in range(c.n_pushes)])
    return f.astype(NP[c.inp])


@lru_cache(maxsize=None)
def reference(name: str):
    """(outputs (pushes, H, W, 2) in the case's out form, {(group, form)} of its remap elements): the restatement run once per case and
    shared by every test that needs it.  Callers must not write into the arrays."""
    c = BY_NAME[name]
    ref = R.HistoryRef(c.H, c.W, c.L, NP[c.ring], c.axes)
    trace, outs, forms = [], [], set()
    for f in fields_of(c):
        outs.append(ref.get_history(f, c.out, trace))
        forms |= element_forms(trace)
        trace.clear()
    res = np.stack(outs)
    res.setflags(write=False)
    return res, frozenset(forms)


def case_forms(c: Case) -> set:
    return static_forms(c) | set(reference(c.name)[1])

"""TEST INFRASTRUCTURE -- the frames, batches, pair counts and pointers at which every form of the global-motion branch
(csrc/kernels_motion.hip and its launches in csrc/mavflow.cpp) is held to the numpy restatement tests/global_motion_ref.py by
tests/test_gpu_motion_forms.py, and the forms each case takes there.  The counterpart of tests/detect_cases.py for this branch.

The two full-frame passes dispatch per batch item on the alignment of the item's bases, on the frame's pixel count (tails, the
grid-stride loop past the cap of 2048 workgroups) and on its width (a thread's pixels straddling a row end); the calls differ in the
outputs they request, the matrix stride and the fit's flags; the fit's sums run in chunks of 16.  Every predicate below restates one
such decision and cites the line it mirrors; tests/test_motion_cases_cpu.py derives the forms each case reaches from these predicates
alone and fails when a form of FORMS is reached by no case, or when a case's `expects` is not what the predicates say.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from global_motion_cases import H_TRUE, fit_cases, project

MAX_PAIRS = 65536             # MAV_HOMOGRAPHY_MAX_PAIRS (include/mavflow.h)
WG = 256                      # threads of a workgroup of both passes and of k_pair_gather
CAP = 2048                    # motion_blocks(): most workgroups of a pass per batch item
PX_A, PX_B = 2, 4             # pixels per thread of k_motion_pass_a / k_motion_pass_b
STAGED_ALIGN = 256            # a staging block is a hipMalloc allocation of its own: aligned to at least this

FORMS = {
    "passA.access": {"vec", "scalar"},
    "passA.tail": {"even", "odd-last-pixel"},
    "passA.pair": {"in-row", "straddles-row-end"},
    "passA.stride": {"1", ">1", ">1:partial-last"},
    "passA.outputs": {"none", "warped", "mag", "warped+mag", "gm:nokey", "warped:nokey"},
    "passA.key": {"key", "nokey"},
    "passB.access": {"vec", "scalar"},
    "passB.tail": {"cnt4", "cnt1", "cnt2", "cnt3"},
    "passB.quad": {"in-row", "one-row-end", "several-row-ends"},
    "passB.stride": {"1", ">1"},
    "passB.max": {"positive", "zero"},
    "m_stride": {"6", "9"},
    "ok": {"null", "all-good", "one-failed"},
    "gather.blocks": {"n<256", "n%256==0", "n%256!=0"},
    "fit.sum_tail": {"n%16==0", "n%16!=0", "n<16"},
    "fit.n": {"4", "bound"},
    "ptr": {"staged", "caller:flow+8B", "caller:gray+1B", "caller:warped+8B", "caller:mag+4B"},
}
# Not reached, with the reason.  Unlike the UNTESTED forms of detect_cases.py, a caller's 8-byte aligned flow pointer, 4-byte aligned
# mag pointer or odd gray pointer is an ordinary, valid argument of the _dev entry points (include/mavflow.h states no alignment), so
# those ARE cases; what is left is:
UNTESTED = {
    # `gm` is never a caller's pointer: only mav_last_global_motion_render passes one, and it is that call's own staging block
    "ptr": {"caller:gm+8B"},
}


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------
def motion_blocks(items: int) -> int:
    """kernels_motion.hip motion_blocks(): `need = (items + 255) / 256; need < 2048 ? (need ? need : 1) : 2048`."""
    need = (items + WG - 1) // WG
    return need if 0 < need < CAP else (1 if need == 0 else CAP)


def pass_items(n0: int, px: int) -> int:
    """k_motion_pass_a: `pairs = (n0 + 1) / 2`; k_motion_pass_b: `quads = (n0 + 3) / 4`; the launchers pass the same count."""
    return (n0 + px - 1) // px


def grid_threads(n0: int, px: int) -> int:
    """Threads of one grid pass over an item: `gridDim.x * 256`, the loops' stride."""
    return motion_blocks(pass_items(n0, px)) * WG


def second_iteration_pixel(px: int) -> int:
    """The first pixel a capped grid reaches in its second iteration: thread 0 of workgroup 0 at q = 2048 * 256."""
    return CAP * WG * px


def stride_forms(n0: int, px: int) -> set:
    """`for (q = blockIdx.x * 256 + threadIdx.x; q < items; q += gridDim.x * 256)`: the iterations thread 0 takes, and whether
    the last one leaves threads without an item."""
    items, T = pass_items(n0, px), grid_threads(n0, px)
    iters = (items + T - 1) // T
    if iters <= 1:
        return {"1"}
    return {">1"} | ({">1:partial-last"} if items % T else set())


def pass_a_vec(n0: int, b: int, flow_off=0, warped_off=0, mag_off=0, gm_off=0) -> bool:
    """k_motion_pass_a: `vec = (f & 15) == 0 && (!warped || ((warped + base * 2) & 15) == 0) && (!gm || ((gm + base * 2) & 15) == 0)
    && (!mag || ((mag + base) & 7) == 0)` with f = flow + base * 2, base = b * W * H.  The offsets are those of each buffer's start
    from a STAGED_ALIGN boundary in bytes; None = the output is not requested."""
    base = b * n0
    ok = (flow_off + base * 8) % 16 == 0
    ok = ok and (warped_off is None or (warped_off + base * 8) % 16 == 0)
    ok = ok and (gm_off is None or (gm_off + base * 8) % 16 == 0)
    return ok and (mag_off is None or (mag_off + base * 4) % 8 == 0)


def pass_b_vec(n0: int, b: int, flow_off=0, gray_off=0) -> bool:
    """k_motion_pass_b: `vec = (f & 15) == 0 && (g & 3) == 0` with f = flow + base * 2, g = gray + base."""
    base = b * n0
    return (flow_off + base * 8) % 16 == 0 and (gray_off + base) % 4 == 0


def _row_ends_per_group(W: int, H: int, px: int) -> np.ndarray:
    """For every group of `px` consecutive pixels of the flattened frame (a thread's pair or quad): how many row ends lie between
    two of its pixels.  A row end after pixel e (e = y W + W - 1, a next row exists) is inside group e // px unless e is the group's
    last pixel."""
    n0 = W * H
    groups = np.zeros(pass_items(n0, px), np.int64)
    e = np.arange(H - 1, dtype=np.int64) * W + (W - 1)
    e = e[e % px != px - 1]
    np.add.at(groups, e // px, 1)
    return groups


def pass_a_tail(n0: int) -> str:
    """k_motion_pass_a: `two = p0 + 1 < n0` is false for the last pair of an odd pixel count."""
    return "odd-last-pixel" if n0 % 2 else "even"


def pass_a_pair_forms(W: int, H: int) -> set:
    """k_motion_pass_a: `x1 = x0 + 1 < W ? x0 + 1 : 0, y1 = x0 + 1 < W ? y0 : y0 + 1` for pairs with two pixels."""
    g = _row_ends_per_group(W, H, PX_A)
    two = np.ones(len(g), bool)
    if (W * H) % 2:
        two[-1] = False
    return ({"in-row"} if (two & (g == 0)).any() else set()) | ({"straddles-row-end"} if (two & (g > 0)).any() else set())


def pass_b_tail_forms(n0: int) -> set:
    """k_motion_pass_b: `cnt = n0 - p0 >= 4 ? 4 : (int)(n0 - p0)`."""
    return ({"cnt4"} if n0 >= 4 else set()) | ({f"cnt{n0 % 4}"} if n0 % 4 else set())


def pass_b_quad_forms(W: int, H: int) -> set:
    """k_motion_pass_b: `if (++x == W) { x = 0; y++; }` between the pixels of one quad."""
    g = _row_ends_per_group(W, H, PX_B)
    return ({"in-row"} if (g == 0).any() else set()) | ({"one-row-end"} if (g == 1).any() else set()) | \
        ({"several-row-ends"} if (g > 1).any() else set())


def gather_form(n: int) -> str:
    """launch_pair_gather: grid ((n + 255) / 256, B); k_pair_gather: `if (i >= n) return`."""
    return "n<256" if n < WG else ("n%256==0" if n % WG == 0 else "n%256!=0")


def sum_tail_form(n: int) -> str:
    """seq_sum: `for (i0 = 0; i0 < n; i0 += 16)` with `i0 + u < n` guarding the last chunk."""
    return "n<16" if n < 16 else ("n%16==0" if n % 16 == 0 else "n%16!=0")


def fit_n_forms(n: int) -> set:
    """check_pairs (mavflow.cpp): `n < 4 || n > MAV_HOMOGRAPHY_MAX_PAIRS` is refused."""
    return ({"4"} if n == 4 else set()) | ({"bound"} if n == MAX_PAIRS else set())


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
OUTPUT_SETS = {"none": (), "warped": ("warped",), "mag": ("mag",), "warped+mag": ("warped", "mag")}      # Context.global_motion's
RENDER_SETS = {"gm:nokey": ("global",), "warped:nokey": ("warped",)}                                     # render_last_global_motion's


@dataclass(frozen=True)
class Case:
    """One call shape.  entry: "host" (mav_global_motion: staged pointers, M (B, 6), no flags), "dev" (mav_global_motion_dev on the
    caller's buffers), "step" (mav_global_motion_step_dev: gather + fit + passes, matrix stride 9, the fit's flags) or "fit"
    (mav_find_homography alone).  Offsets: bytes added to an aligned device buffer's pointer."""
    name: str
    entry: str
    W: int = 0
    H: int = 0
    B: int = 1
    fields: tuple = ()            # field kinds (fields_of) run through the call
    outputs: tuple = ("warped+mag",)      # keys of OUTPUT_SETS / RENDER_SETS requested, one call each
    n: int = 0                    # pairs per item (step, fit)
    failed: int | None = None     # step: the item whose pairs determine no homography
    flow_off: int = 0
    gray_off: int = 0
    warped_off: int = 0
    mag_off: int = 0
    expects: frozenset = frozenset()

    @property
    def n0(self):
        return self.W * self.H


def case_forms(c: Case) -> set:
    """{(group, form)} the case reaches, from the predicates alone."""
    out = set()
    if c.entry in ("step", "fit"):
        out.add(("fit.sum_tail", sum_tail_form(c.n)))
        out |= {("fit.n", f) for f in fit_n_forms(c.n)}
    if c.entry == "fit":
        return out
    n0 = c.n0
    if c.entry == "step":
        out |= {("gather.blocks", gather_form(c.n)), ("m_stride", "9"), ("ok", "all-good" if c.failed is None else "one-failed")}
        outputs = ("none",) + tuple(o for o in c.outputs if o in RENDER_SETS)        # the step requests neither warped nor mag
    else:
        out |= {("m_stride", "6"), ("ok", "null")}
        outputs = c.outputs
    for o in outputs:
        out.add(("passA.outputs", o))
        out.add(("passA.key", "nokey" if o in RENDER_SETS else "key"))
        w = c.warped_off if "warped" in o else None
        m = c.mag_off if "mag" in o else None
        g = 0 if o.startswith("gm") else None
        for b in range(c.B):
            out.add(("passA.access", "vec" if pass_a_vec(n0, b, c.flow_off, w, m, g) else "scalar"))
    for b in range(c.B):
        out.add(("passB.access", "vec" if pass_b_vec(n0, b, c.flow_off, c.gray_off) else "scalar"))
    out.add(("passA.tail", pass_a_tail(n0)))
    out |= {("passA.pair", f) for f in pass_a_pair_forms(c.W, c.H)}
    out |= {("passA.stride", f) for f in stride_forms(n0, PX_A)}
    out |= {("passB.tail", f) for f in pass_b_tail_forms(n0)}
    out |= {("passB.quad", f) for f in pass_b_quad_forms(c.W, c.H)}
    out |= {("passB.stride", f) for f in stride_forms(n0, PX_B) - {">1:partial-last"}}       # (FORMS names no partial form for pass B: every quad carries its own count)
    for f in c.fields:
        out.add(("passB.max", "zero" if f == "zero" else "positive"))
    offs = [("flow+8B", c.flow_off), ("gray+1B", c.gray_off), ("warped+8B", c.warped_off), ("mag+4B", c.mag_off)]
    out |= {("ptr", "caller:" + k) for k, v in offs if v}
    if c.entry == "host":
        out.add(("ptr", "staged"))
    return out


def _e(*forms):
    return frozenset(forms)


SMALL_FIELDS = ("random", "constant", "zero", "last_pixel")
LARGE_FIELDS = ("random", "constant", "zero", "ties_all", "ties_late", "ties_last")
TINY = [(1, 1), (2, 1), (3, 1), (1, 5), (3, 3), (5, 2)]
TINY_EXPECTS = {                                          # batch 3: an odd W * H gives item 1 an 8-byte base
    (1, 1): _e("passA.tail=odd-last-pixel", "passB.tail=cnt1", "passA.access=scalar", "passB.access=scalar"),
    (2, 1): _e("passA.tail=even", "passA.pair=in-row", "passB.tail=cnt2", "passA.access=vec", "passB.access=scalar"),
    (3, 1): _e("passA.tail=odd-last-pixel", "passB.tail=cnt3", "passA.access=scalar"),
    (1, 5): _e("passA.pair=straddles-row-end", "passB.quad=several-row-ends", "passB.tail=cnt1", "passB.tail=cnt4"),
    (3, 3): _e("passA.pair=straddles-row-end", "passB.quad=one-row-end", "passB.tail=cnt1", "passA.access=scalar"),
    (5, 2): _e("passA.tail=even", "passA.pair=straddles-row-end", "passB.quad=one-row-end", "passB.tail=cnt2", "passA.access=vec",
               "passB.access=scalar"),
}
CALLER = dict(W=64, H=64, B=2, fields=("random",))       # item bases all aligned (64 * 64 * 8 B per item): each offset alone selects scalar
CASES = [Case(f"tiny{W}x{H}b3", "host", W, H, 3, fields=("random", "constant", "zero"), expects=TINY_EXPECTS[(W, H)]) for W, H in TINY] + [
    # the two sizes kept from tests/test_gpu_global_motion.py SIZES, with what they are there for
    Case("64x64b1", "host", 64, 64, 1, fields=SMALL_FIELDS,
         expects=_e("passA.access=vec", "passB.access=vec", "passA.tail=even", "passA.pair=in-row", "passB.tail=cnt4", "passB.quad=in-row",
                    "passA.stride=1", "passB.stride=1", "m_stride=6", "ok=null", "ptr=staged", "passB.max=zero", "passB.max=positive")),
    Case("97x71b3", "host", 97, 71, 3, fields=SMALL_FIELDS,
         expects=_e("passA.access=vec", "passA.access=scalar", "passB.access=scalar", "passA.tail=odd-last-pixel",
                    "passA.pair=straddles-row-end", "passB.quad=one-row-end", "passB.tail=cnt3", "passA.stride=1")),
    # past pass A's cap: 1 050 625 px, a second iteration of 1025 pairs; at batch 2 item 1 is scalar with a stride
    Case("1025x1025b1", "host", 1025, 1025, 1, fields=LARGE_FIELDS,
         expects=_e("passA.stride=>1", "passA.stride=>1:partial-last", "passB.stride=1", "passA.tail=odd-last-pixel", "passB.tail=cnt1",
                    "passA.access=vec")),
    Case("1025x1025b2", "host", 1025, 1025, 2, fields=LARGE_FIELDS,
         expects=_e("passA.stride=>1:partial-last", "passA.access=scalar", "passA.access=vec", "passB.access=scalar")),
    # past pass B's cap too: 2 099 601 px
    Case("1449x1449b1", "host", 1449, 1449, 1, fields=LARGE_FIELDS + ("tiesB_all", "tiesB_late"),
         expects=_e("passB.stride=>1", "passA.stride=>1:partial-last", "passB.tail=cnt1", "passB.quad=one-row-end")),
    # every output set the entry points can produce, on an odd-base item and with a stride
    Case("outputs97x71b3", "host", 97, 71, 3, fields=("random",), outputs=tuple(OUTPUT_SETS) + tuple(RENDER_SETS),
         expects=_e(*["passA.outputs=" + o for o in tuple(OUTPUT_SETS) + tuple(RENDER_SETS)], "passA.key=key", "passA.key=nokey",
                    "passA.access=scalar")),
    Case("outputs1025x1025b2", "host", 1025, 1025, 2, fields=("random",), outputs=tuple(OUTPUT_SETS) + tuple(RENDER_SETS),
         expects=_e(*["passA.outputs=" + o for o in tuple(OUTPUT_SETS) + tuple(RENDER_SETS)], "passA.access=scalar",
                    "passA.stride=>1:partial-last")),
    # the step: matrix stride 9 behind the fit, the fit's flags, the gather's grid
    Case("step97x71b3_failed", "step", 97, 71, 3, fields=("step",), n=200, failed=1,
         expects=_e("m_stride=9", "ok=one-failed", "gather.blocks=n<256", "fit.sum_tail=n%16!=0", "passA.outputs=none")),
    # a caller's own pointers
    Case("caller64x64b2_aligned", "dev", **CALLER, expects=_e("passA.access=vec", "passB.access=vec", "m_stride=6", "ok=null")),
    Case("caller64x64b2_flow+8B", "dev", **CALLER, flow_off=8, expects=_e("passA.access=scalar", "passB.access=scalar", "ptr=caller:flow+8B")),
    Case("caller64x64b2_gray+1B", "dev", **CALLER, gray_off=1, expects=_e("passA.access=vec", "passB.access=scalar", "ptr=caller:gray+1B")),
    Case("caller64x64b2_warped+8B", "dev", **CALLER, warped_off=8, expects=_e("passA.access=scalar", "passB.access=vec", "ptr=caller:warped+8B")),
    Case("caller64x64b2_mag+4B", "dev", **CALLER, mag_off=4, expects=_e("passA.access=scalar", "passB.access=vec", "ptr=caller:mag+4B")),
    # an odd pixel count on the caller's buffers: the last pair's second pixel does not exist, and nothing may be written past an
    # output's end (the GPU test keeps guard bytes there)
    Case("caller97x71b3_aligned", "dev", 97, 71, 3, fields=("random",),
         expects=_e("passA.tail=odd-last-pixel", "passA.access=scalar", "passB.tail=cnt3", "passB.access=scalar")),
    Case("step64x64b2_aligned", "step", 64, 64, 2, fields=("step",), n=256,
         expects=_e("passA.access=vec", "m_stride=9", "ok=all-good", "gather.blocks=n%256==0", "fit.sum_tail=n%16==0")),
    Case("step64x64b2_flow+8B", "step", 64, 64, 2, fields=("step",), n=300, flow_off=8,
         expects=_e("passA.access=scalar", "passB.access=scalar", "ptr=caller:flow+8B", "gather.blocks=n%256!=0", "fit.sum_tail=n%16!=0")),
    Case("step64x64b2_gray+1B", "step", 64, 64, 2, fields=("step",), n=256, gray_off=1,
         expects=_e("passA.access=vec", "passB.access=scalar", "ptr=caller:gray+1B")),
    # the fit alone: the chunk of 16 of its sums, and the two ends of the accepted range of n
    Case("fit4", "fit", n=4, expects=_e("fit.n=4", "fit.sum_tail=n<16")),
    Case("fit15", "fit", n=15, expects=_e("fit.sum_tail=n<16")),
    Case("fit16", "fit", n=16, expects=_e("fit.sum_tail=n%16==0")),
    Case("fit256", "fit", n=256, expects=_e("fit.sum_tail=n%16==0")),
    Case("fit1000_frame_like", "fit", n=1000, expects=_e("fit.sum_tail=n%16!=0")),
    Case("fit_bound", "fit", n=MAX_PAIRS, expects=_e("fit.n=bound", "fit.sum_tail=n%16==0")),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def frame_cases(entry="host", large=None):
    """The cases of one entry point; large: None = all, True / False = frames past / below pass A's cap."""
    return [c for c in CASES if c.entry == entry and not c.name.startswith("outputs") and
            (large is None or (c.n0 > second_iteration_pixel(PX_A)) == large)]


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
HOMOGRAPHY = np.array([[1.013, -0.021, 2.75], [0.017, 0.991, -1.5], [3e-5, -2e-5, 1.0]])
TIE_VECTOR, TIE_MAG = (3.0, 4.0), 5.0


def tie_pixels(c: Case) -> dict:
    """kind -> the flattened pixels that carry TIE_VECTOR; the FIRST of them must be reported.  ties_*: around the first pixel of pass
    A's second iteration; tiesB_*: around the first pixel of pass B's (frames that reach it); each with the frame's last pixel."""
    n0 = c.n0
    out = {}
    for tag, px in (("ties", PX_A), ("tiesB", PX_B)):
        edge = second_iteration_pixel(px)
        if edge < n0 - 1:
            out.update({tag + "_all": (edge - 1, edge, n0 - 1), tag + "_late": (edge, n0 - 1)})
    out["ties_last"] = (n0 - 1,)
    return out


def fields_of(c: Case, kind: str):
    """(flows (B, H, W, 2) float32, matrices (B, 3, 3) float64) of one field kind."""
    W, H, B = c.W, c.H, c.B
    rng = np.random.default_rng(W * 7 + H + B)
    eye = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
    zero = np.zeros((B, H, W, 2), np.float32)
    if kind == "random":                                  # noise and, where it fits, a moving patch somewhere else in every item
        gen = np.stack([HOMOGRAPHY + rng.normal(0, 1e-3, (3, 3)) * np.array([[1], [1], [0]]) for _ in range(B)])
        f = rng.normal(0, 1.5, (B, H, W, 2)).astype(np.float32)
        if W > 20 and H > 20:
            for b in range(B):
                y0, x0 = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 20))
                f[b, y0:y0 + 18, x0:x0 + 18] += np.float32(9.0)
        return f, gen
    if kind == "zero":
        return zero, eye
    if kind == "constant":                                # every pixel ties: pixel (0, 0) must win
        shift = eye.copy()
        shift[:, 0, 2], shift[:, 1, 2] = 2.5, -1.25
        return zero, shift
    if kind == "last_pixel":
        f = zero.copy()
        f[:, H - 1, W - 1] = TIE_VECTOR
        return f, eye
    if kind in tie_pixels(c):
        f = zero.copy()
        for p in tie_pixels(c)[kind]:
            y, x = divmod(p, W)
            f[:, y, x] = TIE_VECTOR
        return f, eye
    raise ValueError(kind)


def step_inputs(c: Case):
    """(flows (B, H, W, 2) float32, coords (n, 2) of (x, y)) of a step case: a smooth field with noise and a moving patch per item; the
    pairs of item `failed` all land on one point, which determines no homography."""
    W, H, B = c.W, c.H, c.B
    rng = np.random.default_rng(5 + c.n + c.flow_off + c.gray_off)
    coords = np.c_[rng.integers(2, W - 2, c.n), rng.integers(2, H - 2, c.n)]
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.stack([np.stack([0.01 * xx - 0.3 + 0.002 * yy, -0.008 * yy + 0.2], axis=-1) for _ in range(B)]).astype(np.float32)
    f += rng.normal(0, 0.05, f.shape).astype(np.float32)
    for b in range(B):
        y0, x0 = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 20))
        f[b, y0:y0 + 16, x0:x0 + 16] += np.float32(6.0 - 10.0 * (b % 2))
    if c.failed is not None:
        f[c.failed, ..., 0], f[c.failed, ..., 1] = 7.0 - xx, 9.0 - yy
    return f, coords


FRAME_LIKE_SIZE = (1920, 1024)
FRAME_LIKE_H = np.array([[1.004, -0.006, 3.5], [0.005, 0.997, -2.25], [4e-6, -3e-6, 1.0]])


def frame_like_pairs():
    """(src, dst) (1000, 2) float64: samples of a 1920 x 1024 field -- the reference's capture size -- under a perspective motion with
    0.3 px of noise; the samples inside one 200 x 160 patch move by 6 px more.  dst = src + a float32 vector, what the gather gives."""
    rng = np.random.default_rng(41)
    W, H = FRAME_LIKE_SIZE
    coords = np.c_[rng.integers(0, W, 1000), rng.integers(0, H, 1000)]
    src = coords.astype(np.float64)
    flow = (project(FRAME_LIKE_H, src) - src + rng.normal(0, 0.3, (1000, 2))).astype(np.float32)
    patch = (coords[:, 0] >= 900) & (coords[:, 0] < 1100) & (coords[:, 1] >= 400) & (coords[:, 1] < 560)
    assert patch.sum() >= 5
    flow[patch] += np.float32(6.0)
    return src, src + flow


def fit_pairs(c: Case):
    """(src, dst) (n, 2) float64 of a fit case: the noisy H_TRUE recipe of global_motion_cases.fit_cases() at the case's n, the exact
    four corners at n = 4, the frame-like set at its own name."""
    if c.name == "fit1000_frame_like":
        return frame_like_pairs()
    if c.n == 4:
        _, src, dst, _ = fit_cases()[0]
        return src, dst
    rng = np.random.default_rng(1000 + c.n)
    src = rng.integers(20, 620, (c.n, 2)).astype(np.float64)
    return src, project(H_TRUE, src) + rng.normal(0, 0.7, (c.n, 2)).astype(np.float32)

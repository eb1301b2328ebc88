"""TEST INFRASTRUCTURE -- the host scheduler's ways of sweeping a layer (band-major or sweep-major, one stream or two, a partition
shifted by half a band, column strips of the tile order, M through its own, the first or alternating slots), restated, and the small
frames at which every one of them is run against the plain schedule (tests/test_gpu_schedule_forms.py) -- the sibling of
tests/stage_cases.py and tests/detect_cases.py.

What is restated, with the lines it mirrors (mavflow.cpp / kernels_flow.hip):
  * plan_sweeps (mavflow.cpp:1347-1407): name, pairs per launch, streams, J, shifted partition, where the initial M is built, M slot rule;
  * the calls it is made from: farneback_run's chunks and groups (mavflow.cpp:1734-1766), walk_layers (1629-1637), layer_sweeps' loop over
    the sub-groups (1481-1523), the deep layers (use_deep_batch 1705, the kd loop 721-723);
  * sweeps_band_major (mavflow.cpp:1440-1473): bound() with and without phase and with band_skew; per band the initial-M pixel rows and
    the (sweep, ty0, ty1) launches, the empty ones left out;
  * make_tile_map / tile_grid / tile_of_block (kernels_flow.hip:28-63): strip width, tiles per image, grid size, the tile of every
    workgroup.
tests/test_schedule_cases_cpu.py checks the restatement's own properties (every sweep covers every tile row once, a band's initial M
holds what its first sweep reads, no sweep reads a row of M another launch has overwritten, the tile map is a bijection) and that every
form of FORMS is reached; tests/test_gpu_schedule_forms.py ties the restatement to the library (mav_schedule_info, the launches per
class and stream of the profile) and compares every variant with the reference schedule bit for bit, every buffer dirty."""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass

import numpy as np

from stage_cases import pyramid

FT_X, FT_Y, HALO = 64, 16, 6              # kernels_flow.hip:1548-1549: the fast sweep's tile; winsize 12 / 13: a 6-pixel halo

FORMS = {
    "bands": {"J1:fallback", "J2", "J3..7", "J8", "J==Jmax", "T==Jmax*(I+2)"},
    "stream": {"one", "two", "two:ragged-last-group", "group-of-one"},
    "bound": {"plain", "clamp-hi", "clamp-lo", "skew-default", "skew0", "phase"},
    "sweep-range": {"ty0-clamped-to-0", "band-empty-at-late-sweep", "ragged-last-tile-row"},
    "iterations": {"1", "even", "odd>1", "10"},
    "initial_m": {"group", "sub", "band:zero", "band:coarser", "band:field"},
    "m_slot": {"own", "first", "alternate", "alternate:per_launch>1"},
    "window": {"box", "gauss"},
    "strip": {"auto:one", "auto:split", "1", "ragged-last", ">=tiles_x"},
    "grid": {"pad", "G>1"},
    "sweep-form": {"fast<6>", "fast<6,false>"},
}
# Not reached, on purpose:
#   bound / clamp-lo -- bound() raises a boundary to `lo = j` when T j / J + skew < j.  plan_sweeps grants J bands only when
#   T >= (iterations + 2) J, so T j / J >= 3 j, and the skew is never negative ("band_skew" = -1 stands for (iterations - 1) / 2 >= 0):
#   no frame and no option set reaches the clamp.  It stays in the restatement as it stays in the library.
UNTESTED = {"bound": {"clamp-lo"}}

# every option a variant may set, with the library's default (mav_ctx's initialisers, mavflow.cpp:357-427; "group": mav_create gives
# min(16, max_batch) below 4 Mpx, and no case here holds more than 16 pairs; "bands" 0 = automatic, 1 at these sizes: mavflow.cpp:734-738)
DEFAULTS = {"group": None, "group_fine": 1, "bands": 0, "pairs_in_flight": 2, "band_mb": 96, "coarse_cache_mb": 220, "coarse_half": 0,
            "share_m": 1, "strip": 0, "small_batch": 1, "deep_batch": 1, "coarse_bands": 0, "band_phase": 0, "band_skew": -1}
DEEP_FRAC = 6                             # mav_ctx::deep_frac (fixed once flow has been computed: not a variant's to set)


def reference_options(batch: int) -> dict:
    """The plain schedule every variant is compared with: one stream, sweep-major, the whole group per launch, M in its own slots."""
    return {"pairs_in_flight": 1, "bands": 1, "small_batch": 0, "deep_batch": 0, "group": batch, "group_fine": 0, "share_m": 0, "strip": 1 << 20}


def options(batch: int, variant: dict) -> dict:
    o = dict(DEFAULTS, **variant)
    if o["group"] is None or o["group"] > batch:                      # set_group clamps to max_batch (mavflow.cpp:757)
        o["group"] = batch
    return o


# ---- plan_sweeps ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    name: str
    per_launch: int
    streams: int
    J: int
    shift_second: bool
    m_build: str          # "group" / "sub" / "band"  (MBuild)
    m_slot: str           # "own" / "first" / "alternate"  (MSlot)


def tile_rows(h: int) -> int:
    return (h + FT_Y - 1) // FT_Y                                     # blur_iter_tile_rows, kernels_flow.hip:1712


def sweep_form(w: int) -> str:
    return "fast<6>" if w % 4 == 0 else "fast<6,false>"               # launch_sweep, kernels_flow.hip:1736-1742 (winsize 12 / 13)


def plan_sweeps(layers, k: int, g: int, I: int, winsize: int, o: dict) -> Plan:
    """mavflow.cpp:1347-1407.  layers: [(w, h, ...)]; g: pairs of the group; o: options()."""
    w, h = layers[k][:2]
    T = tile_rows(h)
    bands_ok = w % 4 == 0 and winsize // 2 == 6                       # :1833 (blur_iter_bands_ok on the library's own aligned buffers)
    bands_set = o["bands"] > 0                                        # set_bands, :765-770
    n0 = layers[0][0] * layers[0][1]                                  # mav_create's automatic count, :734-738
    bands = o["bands"] if bands_set else (min((n0 * 80 + (230 << 20) - 1) // (230 << 20), 8) if n0 * 80 > 200 << 20 else 1)
    sub = g
    if k == 0 and 0 < o["group_fine"] < g:                            # :1356
        sub = o["group_fine"]
    ws_pair = w * h * 80
    if k > 0 and o["coarse_cache_mb"] > 0:                            # :1357-1361
        fit = (o["coarse_cache_mb"] << 20) // max(ws_pair, 1)
        if fit < sub:
            sub = max(fit, 1)
    m_per_sub = sub < g                                               # :1365
    band_bytes = o["band_mb"] << 20
    big_coarse = bool(k > 0 and o["coarse_bands"] and bands_ok and ws_pair > band_bytes and T // (I + 2) >= 2)    # :1370
    if big_coarse:
        sub, m_per_sub = 1, True
    if k > 0 and not big_coarse and o["pairs_in_flight"] == 2 and g >= 2:                                         # :1372-1381
        half = max(sub // 2, 1)
        if o["coarse_half"] > 0:
            half = o["coarse_half"]
        if 2 * half > g:
            half = (g + 1) // 2
        return Plan("two sub-groups in flight", half, 2, 1, False, "sub", "alternate")
    if (k == 0 or big_coarse) and o["pairs_in_flight"] == 2 and m_per_sub and sub == 1 and g >= 2:                # :1382-1399
        J = bands if (bands_set and k == 0) else (ws_pair + band_bytes - 1) // band_bytes
        J = max(min(J, T // (I + 2)), 1)
        if J == 1 or bands_ok:
            return Plan("two pairs in flight, band-major", 1, 2, J, bool(J > 1 and o["band_phase"] and J >= o["band_phase"]),
                        "band" if J > 1 else "sub", "alternate")
    J = bands if (k == 0 and (m_per_sub or g == 1) and sub == 1 and T >= (I + 2) * bands and bands_ok) else 1     # :1405
    return Plan("one stream", sub, 1, J, False, "sub" if m_per_sub else "group", "first" if (m_per_sub and o["share_m"]) else "own")


# ---- sweeps_band_major ----------------------------------------------------------------------------------------------------------
def band_bounds(T: int, I: int, J: int, phase: bool, band_skew: int):
    """bound(0) .. bound(NBands), mavflow.cpp:1443-1454 -> (bounds, which interior bounds were clamped: {"plain", "clamp-lo", "clamp-hi"})"""
    nb = J + 1 if phase else J
    out, how = [], set()
    for j in range(nb + 1):
        if j <= 0:
            out.append(0)
        elif j >= nb:
            out.append(T)
        elif phase:
            out.append(T * (2 * j - 1) // (2 * J))                    # :1447
        else:
            b = T * j // J + ((I - 1) // 2 if band_skew < 0 else band_skew)      # :1451
            lo, hi = j, T - (nb - j)                                  # :1452
            how.add("clamp-lo" if b < lo else "clamp-hi" if b > hi else "plain")
            out.append(lo if b < lo else hi if b > hi else b)
    return out, how


@dataclass
class Band:
    j: int
    a0: int
    a1: int
    m_rows: tuple | None              # pixel rows [y0, y1) of the band's own initial M (M_BAND), clipped as launch_initial_m clips them
    launches: list                    # (sweep, ty0, ty1), non-empty ones only
    skipped: list                     # the sweeps at which the band is empty


def band_walk(h: int, I: int, J: int, phase: bool, band_skew: int, per_band_m: bool):
    """mavflow.cpp:1455-1472: the bands of one sub-group in launch order."""
    T = tile_rows(h)
    bounds, _ = band_bounds(T, I, J, phase, band_skew)
    nb = len(bounds) - 1
    out = []
    for j in range(nb):
        a0, a1 = bounds[j], bounds[j + 1]
        if a1 <= a0:                                                  # :1457
            continue
        m_rows = None
        if per_band_m:                                                # :1460, clipped by launch_initial_m (kernels_flow.hip:1349)
            y0, y1 = (0 if a0 == 0 else a0 * 16 - 8), (h if j == nb - 1 else a1 * 16 + 8)
            m_rows = (max(y0, 0), h if (y1 < 0 or y1 > h) else y1)
        b = Band(j, a0, a1, m_rows, [], [])
        for it in range(I):
            ty0, ty1 = max(a0 - it, 0), (T if j == nb - 1 else a1 - it)      # :1464-1465
            if ty1 <= ty0:                                            # :1466
                b.skipped.append(it)
                continue
            b.launches.append((it, ty0, ty1))
        out.append(b)
    return out


# ---- make_tile_map / tile_grid / tile_of_block ----------------------------------------------------------------------------------
@dataclass(frozen=True)
class TileMap:
    tiles_x: int
    tiles_y: int
    per_img: int
    n_tiles: int
    strip_w: int
    ty0: int


def make_tile_map(w: int, h: int, G: int, ty0: int = 0, ty1: int = -1, strip: int = 0) -> TileMap:
    """kernels_flow.hip:46-62 with the fast sweep's 64 x 16 tile"""
    tiles_x, tiles_y = (w + FT_X - 1) // FT_X, (h + FT_Y - 1) // FT_Y
    t0 = (ty0 if ty0 < tiles_y else tiles_y) if ty0 > 0 else 0
    if 0 <= ty1 < tiles_y:
        tiles_y = ty1
    tiles_y = tiles_y - t0 if tiles_y > t0 else 0
    sw = tiles_x
    if strip > 0:
        sw = strip if strip < tiles_x else tiles_x
    elif tiles_x > 40:
        ns = (tiles_x + 29) // 30
        sw = (tiles_x + ns - 1) // ns
    return TileMap(tiles_x, tiles_y, tiles_x * tiles_y, tiles_x * tiles_y * G, sw, t0)


def tile_grid(tm: TileMap) -> int:
    return (tm.n_tiles + 7) // 8 * 8                                  # kernels_flow.hip:63


def tile_of_block(tm: TileMap, b: int, grid: int):
    """kernels_flow.hip:29-44: (image, tx, ty) of workgroup b of a grid of `grid`, or None for a workgroup that leaves"""
    per = (grid + 7) >> 3
    tile = (b & 7) * per + (b >> 3)
    if tile >= tm.n_tiles:
        return None
    img = tile // tm.per_img
    tr = tile - img * tm.per_img
    strip_tiles = tm.strip_w * tm.tiles_y
    st = tr // strip_tiles
    tr -= st * strip_tiles
    x_base = st * tm.strip_w
    sw = min(tm.strip_w, tm.tiles_x - x_base)
    row = tr // sw
    return img, x_base + tr - row * sw, row + tm.ty0


def strip_form(tiles_x: int, strip: int) -> str:
    if strip == 0:
        return "auto:split" if tiles_x > 40 else "auto:one"
    if strip >= tiles_x:
        return ">=tiles_x"
    if strip == 1:
        return "1"
    return "ragged-last" if tiles_x % strip else "even"


# ---- one call -------------------------------------------------------------------------------------------------------------------
@dataclass
class SubGroup:
    """One sub-group of layer_sweeps' loop (mavflow.cpp:1502-1516)."""
    k: int
    plan: Plan
    g: int                # pairs of the group it belongs to
    s0: int               # its first pair
    gs: int               # its pairs = images per launch
    stream: int
    slot: int             # first M slot (m_off / ms, :1506)
    phase: bool
    source: str           # "zero" / "coarser" / "field": the layer's FlowSource kind
    bands: list           # band_walk


def deep_layers(case: "Case", o: dict):
    """(kd, does the call run layers kd .. top once for all its pairs?): mavflow.cpp:721-722 and use_deep_batch, :1705"""
    layers, kd = case.layers(), 0
    for k in range(len(layers) - 1, 0, -1):
        if layers[k][0] * layers[k][1] * DEEP_FRAC <= case.W * case.H:
            kd = k
        else:
            break
    return kd, bool(o["deep_batch"] and kd > 0 and case.batch > o["group"])


def call_walk(case: "Case", variant: dict):
    """Every sub-group of one farneback call of the case under the variant's options, in host order (farneback_run)."""
    o = options(case.batch, variant)
    layers, I, batch, group = case.layers(), case.iterations, case.batch, o["group"]
    L = len(layers)
    kd, deep = deep_layers(case, o)
    chunk = min(batch, 64) if deep else batch                         # deep_cap, :723 and :1744
    out = []

    def layer(k, g):                                                  # layer_sweeps
        p = plan_sweeps(layers, k, g, I, case.winsize, o)
        source = ("field" if case.init else "zero") if k == L - 1 else "coarser"
        for i, s0 in enumerate(range(0, g, p.per_launch)):
            second = p.streams == 2 and bool(i & 1)
            slot = s0 if p.m_slot == "own" else 0 if p.m_slot == "first" else (i & 1) * p.per_launch
            phase = p.shift_second and second
            out.append(SubGroup(k, p, g, s0, min(g - s0, p.per_launch), int(second), slot, phase, source,
                                band_walk(layers[k][1], I, p.J, phase, o["band_skew"], p.m_build == "band")))

    for d0 in range(0, batch, chunk):
        D = min(batch - d0, chunk)
        if deep:
            for k in range(L - 1, kd - 1, -1):                        # deep_layers, :1656
                layer(k, D)
        for g0 in range(d0, d0 + D, group):                           # :1758-1765
            for k in range((kd - 1) if deep else (L - 1), -1, -1):    # flow_group, :1700-1701
                layer(k, min(d0 + D - g0, group))
    return out


def schedule_layers(case: "Case", variant: dict):
    """What mav_schedule_info reports per layer (mavflow.cpp:1825-1837): (sweeps, pairs_per_launch, bands)."""
    o = options(case.batch, variant)
    layers, batch = case.layers(), case.batch
    L = len(layers)
    g = min(batch, o["group"])
    kd, deep = deep_layers(case, o)
    D = min(batch, 64) if deep else 0
    plans = [plan_sweeps(layers, k, D if (deep and k >= kd) else g, case.iterations, case.winsize, o) for k in range(L)]
    return [(p.name, p.per_launch, p.J) for p in plans]


def expected_launches(case: "Case", variant: dict) -> Counter:
    """(profile class, stream) -> launches of one call: the initial-M and the sweep launches (layer_sweeps and sweeps_band_major open one
    ProfScope per launch: mavflow.cpp:1459, 1467, 1497, 1511)."""
    n = Counter()
    for sg in call_walk(case, variant):
        sweeps = "blur_iter" if sg.k == 0 else "blur_iter_coarse"
        if sg.plan.m_build == "group" and sg.s0 == 0:
            n[("update_matrices", 0)] += 1                            # the group's, on the compute stream (:1496-1499)
        if sg.plan.m_build == "sub":
            n[("update_matrices", sg.stream)] += 1
        for b in sg.bands:
            if b.m_rows is not None and b.m_rows[1] > b.m_rows[0]:
                n[("update_matrices", sg.stream)] += 1
            n[(sweeps, sg.stream)] += len(b.launches)
    return n


def sweep_launches(case: "Case", variant: dict):
    """The distinct tile maps the call's sweep launches use: (w, h, G, ty0, ty1, strip).  The relaxed form takes the whole layer
    whatever the band says (kernels_flow.hip:1742); bands exist for fast<6> only."""
    o = options(case.batch, variant)
    layers = case.layers()
    out = set()
    for sg in call_walk(case, variant):
        w, h = layers[sg.k][:2]
        for b in sg.bands:
            for _, ty0, ty1 in b.launches:
                out.add((w, h, sg.gs, ty0, ty1, o["strip"]) if sweep_form(w) == "fast<6>" else (w, h, sg.gs, 0, -1, o["strip"]))
    return sorted(out)


# ---- the forms a variant reaches, from the predicates alone -----------------------------------------------------------------------
def forms_reached(case: "Case", variant: dict) -> set:
    o = options(case.batch, variant)
    layers, I = case.layers(), case.iterations
    walk = call_walk(case, variant)
    r = {f"window:{'gauss' if case.window == 'gaussian' else 'box'}"}
    group_sizes = {sg.g for sg in walk if sg.k == 0}
    if 1 in group_sizes:
        r.add("stream:group-of-one")
    for sg in walk:
        w, h = layers[sg.k][:2]
        T, p = tile_rows(h), sg.plan
        form = sweep_form(w)
        r.add(f"sweep-form:{form}")
        r.add("stream:one" if p.streams == 1 else "stream:two")
        if p.streams == 2 and sg.k == 0 and len(group_sizes) > 1:
            r.add("stream:two:ragged-last-group")
        r.add(f"initial_m:{p.m_build}" if p.m_build != "band" else f"initial_m:band:{sg.source}")
        if sg.g > 1:                                                  # with one pair every slot rule names slot 0
            r.add(f"m_slot:{p.m_slot}")
            if p.m_slot == "alternate" and p.per_launch > 1:
                r.add("m_slot:alternate:per_launch>1")
        if sg.k == 0 and o["bands"] > 1 and p.J == 1:
            r.add("bands:J1:fallback")
        tiles_x = (w + FT_X - 1) // FT_X
        r.add(f"strip:{strip_form(tiles_x, o['strip'])}")
        if sg.gs > 1:
            r.add("grid:G>1")
        for b in sg.bands:
            for _, ty0, ty1 in b.launches:
                tm = make_tile_map(w, h, sg.gs, ty0, ty1, o["strip"]) if form == "fast<6>" else make_tile_map(w, h, sg.gs, 0, -1, o["strip"])
                if tm.n_tiles % 8:
                    r.add("grid:pad")
        if p.J > 1:
            Jmax = T // (I + 2)
            r.add("bands:J2" if p.J == 2 else "bands:J8" if p.J == 8 else "bands:J3..7")
            if p.J == Jmax:
                r.add("bands:J==Jmax")
                if T == Jmax * (I + 2):
                    r.add("bands:T==Jmax*(I+2)")
            r.add("iterations:1" if I == 1 else "iterations:10" if I == 10 else "iterations:even" if I % 2 == 0 else "iterations:odd>1")
            if h % FT_Y:
                r.add("sweep-range:ragged-last-tile-row")
            if sg.phase:
                r.add("bound:phase")
            else:
                r |= {f"bound:{x}" for x in band_bounds(T, I, p.J, False, o["band_skew"])[1]}
                if o["band_skew"] <= 0:
                    r.add("bound:skew-default" if o["band_skew"] < 0 else "bound:skew0")
            for b in sg.bands:
                if b.skipped:
                    r.add("sweep-range:band-empty-at-late-sweep")
                if b.a0 > 0 and any(b.a0 - it < 0 for it, _, _ in b.launches):
                    r.add("sweep-range:ty0-clamped-to-0")
    return r


ALL_FORMS = {f"{family}:{form}" for family, forms in FORMS.items() for form in forms}
ALL_UNTESTED = {f"{family}:{form}" for family, forms in UNTESTED.items() for form in forms}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    W: int
    H: int
    batch: int
    iterations: int
    variants: list                        # option sets (name -> value; the rest at the library's defaults)
    expects: set                          # the forms the case is there to reach
    levels: int = 0
    winsize: int = 12
    window: str = "box"
    init: bool = False                    # the call carries an initial flow (OPTFLOW_USE_INITIAL_FLOW)

    def layers(self):
        return pyramid(self.W, self.H, 0.4, self.levels)

    def fb(self):
        from mavflow import _lib
        fb = _lib.fb_defaults(levels=self.levels)
        fb.winsize, fb.iterations = self.winsize, self.iterations
        return fb

    def params(self):
        from oracle import fb_oracle as fbo
        fb = self.fb()
        return fbo.Params(fb.pyr_scale, fb.levels, fb.winsize, fb.iterations, fb.poly_n, fb.poly_sigma, 0)

    def frames(self):
        from mavflow import synth
        return synth.make_batch(self.W, self.H, self.batch, distinct=self.batch)

    def initial_flow(self, poison: bool = False):
        if not self.init:
            return None
        import initial_flow_ref as ref
        return np.stack([ref.smooth_initial_flow(self.W, self.H, (40 if poison else 3) + b, gain=-0.5 if poison else 0.8) for b in range(self.batch)])


def expected_flow(case: Case, orc, prev, nxt, init=None) -> np.ndarray:
    """The oracle's flow of one pair of the case: fb_oracle.calc, through tests/gauss_window_ref.py for the Gaussian window and
    tests/initial_flow_ref.py for a call with an initial flow."""
    if case.window == "gaussian":
        import gauss_window_ref as gw
        return gw.calc(orc, prev, nxt, case.params())
    if init is not None:
        import initial_flow_ref as ref
        return ref.calc_init(orc, prev, nxt, init, case.params())
    return orc.calc(prev, nxt, case.params())


def variant_id(v: dict) -> str:
    return ",".join(f"{k}={v[k]}" for k in v) or "defaults"


def _pif(*sets):
    return [dict(s, pairs_in_flight=p) for s in sets for p in (1, 2)]


CASES = [
    # ---- bands ----
    Case("68x100-I1", 68, 100, 2, 1, _pif({"bands": 2}, {"bands": 3}), winsize=13,      # T = 7: bands 3 -> J 1 on one stream, 2 on two
         expects={"bands:J2", "bands:J1:fallback", "bands:J==Jmax", "sweep-range:ragged-last-tile-row", "iterations:1", "stream:one",
                  "stream:two", "initial_m:band:zero", "initial_m:sub", "m_slot:first", "m_slot:alternate", "grid:pad", "strip:auto:one",
                  "window:box"}),
    Case("132x200-I2", 132, 200, 2, 2,                                                   # T = 13: bounds 0, 4, 8, 13
         [{"pairs_in_flight": 1, "bands": 3}, {"pairs_in_flight": 2, "bands": 3},
          {"pairs_in_flight": 1, "bands": 3, "band_skew": 64},                          # 0, 11, 12, 13: one-row bands
          {"pairs_in_flight": 2, "bands": 3, "band_skew": 64},
          {"pairs_in_flight": 2, "bands": 3, "band_phase": 1}],                         # second stream: 0, 2, 6, 10, 13
         expects={"bands:J3..7", "bands:J==Jmax", "bound:plain", "bound:clamp-hi", "bound:phase", "iterations:even"}),
    Case("132x370-I1-J8", 132, 370, 2, 1, _pif({"bands": 8}),                           # T = 24 = 8 x 3
         expects={"bands:J8", "bands:J==Jmax", "bands:T==Jmax*(I+2)", "iterations:1"}),
    Case("132x384-I10", 132, 384, 2, 10,                                                # T = 24 = 2 x 12: bounds 0, 16, 24
         _pif({"bands": 2}) + [{"pairs_in_flight": 2, "bands": 2, "band_phase": 1}],    # 0, 6, 18, 24: band 0 empty from sweep 6 on
         expects={"bands:J2", "bands:T==Jmax*(I+2)", "iterations:10", "bound:phase", "bound:skew-default",
                  "sweep-range:ty0-clamped-to-0", "sweep-range:band-empty-at-late-sweep"}),
    Case("132x368-I10", 132, 368, 2, 10, _pif({"bands": 2}), expects={"bands:J1:fallback"}),      # T = 23: one row short of two bands
    Case("132x192-I4", 132, 192, 2, 4, [{"pairs_in_flight": 2, "bands": 2, "band_phase": 1}],    # 0, 3, 9, 12: band 0 empty at sweep 3
         expects={"iterations:even", "bound:phase", "sweep-range:band-empty-at-late-sweep"}),
    Case("132x290-I3", 132, 290, 2, 3, _pif({"bands": 3, "band_skew": 0}, {"bands": 3}),          # T = 19
         expects={"iterations:odd>1", "bound:skew0", "bound:skew-default", "sweep-range:ragged-last-tile-row", "bands:J3..7"}),
    Case("132x384-L1-I10", 132, 384, 2, 10, _pif({"bands": 2}), levels=1,               # layer 1 is 53 x 154: the relaxed form, never banded
         expects={"initial_m:band:coarser", "sweep-form:fast<6,false>", "sweep-form:fast<6>", "bands:J2"}),
    Case("132x192-I4-field", 132, 192, 2, 4, _pif({"bands": 2}), init=True, expects={"initial_m:band:field", "iterations:even"}),
    Case("132x200-I2-gauss", 132, 200, 2, 2, _pif({"bands": 3}), window="gaussian", winsize=13,
         expects={"window:gauss", "bands:J3..7", "initial_m:band:zero"}),
    # ---- batches, groups, slots ----
    Case("132x100-b3", 132, 100, 3, 1,
         _pif({"group": 3, "bands": 2}, {"group": 2, "bands": 2}) +                      # group 2: a last group of one pair
         [{"pairs_in_flight": 1, "share_m": s, "group_fine": gf} for s in (0, 1) for gf in (0, 1, 2)],
         expects={"stream:two:ragged-last-group", "stream:group-of-one", "m_slot:own", "m_slot:first", "m_slot:alternate",
                  "initial_m:group", "initial_m:sub", "grid:G>1"}),
    Case("132x384-L1-b5", 132, 384, 5, 3, [{"group": 5, "coarse_half": 2, "bands": 2}, {"group": 5, "coarse_half": 2, "bands": 2, "small_batch": 0},
                                           {"group": 2, "coarse_half": 1, "bands": 2}], levels=1,       # sub-groups 2, 2, 1; deep layer
         expects={"m_slot:alternate:per_launch>1", "iterations:odd>1", "initial_m:band:coarser"}),
    # ---- strips ----
    Case("2624x52-b3", 2624, 52, 3, 2,                                                  # 41 x 4 x 3 = 492 tiles in a grid of 496
         [{"pairs_in_flight": 1, "group": 3, "group_fine": 0, "strip": s} for s in (0, 1, 7, 41, 1 << 20)],
         expects={"strip:auto:split", "strip:1", "strip:ragged-last", "strip:>=tiles_x", "grid:pad", "grid:G>1"}),
    Case("2622x52-b3", 2622, 52, 3, 2, [{"pairs_in_flight": 1, "group": 3, "group_fine": 0, "strip": s} for s in (0, 7)],
         expects={"sweep-form:fast<6,false>", "strip:auto:split", "strip:ragged-last"}),
    Case("2624x100-I1-strip7", 2624, 100, 2, 1, _pif({"bands": 2, "strip": 7}),         # a band launch (ty0 > 0) through ragged strips
         expects={"strip:ragged-last", "bands:J2", "sweep-range:ragged-last-tile-row"}),
]
NAMES = [c.name for c in CASES]


# ---- poison: another picture's data in every buffer --------------------------------------------------------------------------------
_poison = {}


def poison_frames(W: int, H: int, batch: int):
    """An unrelated pair per slot: noise (nothing of the case's frames in it), pair b a cyclic shift of pair 0."""
    if (W, H) not in _poison:
        rng = np.random.default_rng(W * 10007 + H)
        _poison[(W, H)] = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    a, b = _poison[(W, H)]
    return (np.stack([np.roll(a, (3 * i, 5 * i), (0, 1)) for i in range(batch)]),
            np.stack([np.roll(b, (3 * i, 5 * i), (0, 1)) for i in range(batch)]))


_poison_flow = {}


def poison_flow(W: int, H: int, batch: int) -> np.ndarray:
    """A noise field per pair (sigma 2 px) for the dirtying call to start from; the fields of one shape are kept, no other shape's."""
    if (W, H, batch) not in _poison_flow:
        for key in [k for k in _poison_flow if k[:2] != (W, H)]:
            del _poison_flow[key]
        f = np.random.default_rng(W * 7919 + H).normal(0, 2, (H, W, 2)).astype(np.float32)
        _poison_flow[(W, H, batch)] = np.stack([np.roll(f, (3 * i, 5 * i), (0, 1)) for i in range(batch)])
    return _poison_flow[(W, H, batch)]


def dirty(ctx, W: int, H: int, batch: int, call=None):
    """Run another picture through the context with the options in effect, so that every workspace slot, M buffer and staging slot a
    compared call is about to use holds wrong data: a launch that skips a tile or reads the wrong slot then shows.  call(prev, nxt)
    makes the call; returns what it returned.  The default call is ctx.farneback WITH an initial flow of noise: the host entry points
    upload an initial flow into the very staging block the flow is computed in, so the whole block is overwritten -- a dirtying call
    without one runs the same faulty schedule as the call it precedes, skips the same tile, and leaves there what the call before it
    wrote: the correct flow of the same frames."""
    prev, nxt = poison_frames(W, H, batch)
    if call is None:
        return ctx.farneback(prev, nxt, initial_flow=poison_flow(W, H, batch))
    return call(prev, nxt)

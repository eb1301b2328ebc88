"""Every way the host scheduler can sweep a layer -- band-major or sweep-major, one stream or two, a partition shifted by half a band,
column strips of the tile order, M through its own, the first or alternating slots -- on the small frames of tests/schedule_cases.py,
where the band edges, the clamps of bound(), empty bands, ragged strips and padded grids are reached with launches of microseconds.

Per case the REFERENCE is the plain schedule (one stream, sweep-major, the whole group per launch, M in its own slots) in a fresh
context, held to the oracle through the strict gate of oracle/tolerances.py.  Per VARIANT (an option set of the case):
  1. the plan is the intended one: mav_schedule_info's per-layer sweeps / pairs_per_launch / bands equal the restated plan_sweeps, and
     the profile of one call holds, per stream, the number of initial-M and sweep launches the restated band walk gives -- a variant
     that silently falls back to J = 1, or skips a band, fails here;
  2. dirty first: another picture goes through the same context with the same options, batch and entry point, so that every workspace
     slot, M buffer and staging slot holds wrong data (through host pointers it starts from a noise field, which the entry point
     uploads into the block the flow is computed in: a tile the schedule skips in both calls then holds noise, not the flow an
     earlier variant left there);
  3. the case's frames then give the reference's flow bit for bit -- through host pointers, and through device pointers into a
     caller's buffer filled with 0xFF bytes, of which none may be left;
  4. and once more, call after call.
A tile a launch leaves out, a row a band does not reach or an M read from the wrong slot shows as the other picture's data (or as the
0xFF pattern); tests/test_gpu_schedule_pin.py sees neither, and the bit-identity tests on clean buffers saw only some of it.

Measured on an MI355X: every reference within mean 1.3e-6 / p99.9 2.9e-5 / max 5.5e-5 px of the oracle (the gate: 1e-4 / 1e-2 / 0.15);
the fifteen cases take about two seconds together."""
from collections import Counter

import numpy as np
import pytest

import schedule_cases as sc
from oracle import tolerances

pytestmark = pytest.mark.gpu

SWEEP_CLASSES = ("update_matrices", "blur_iter", "blur_iter_coarse")


def _set(c, opts):
    for k, v in opts.items():
        c.set_option(k, v)


def _same(got, ref, tag):
    if np.array_equal(got, ref):
        return
    bad = (got != ref).any(-1)
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    pytest.fail(f"{tag}: {int(bad.sum())} of {bad.size} pixels differ from the reference schedule, first at (pair, y, x) = {first}: "
                f"{got[first].tolist()} vs {ref[first].tolist()}")


def _launch_counts(c):
    kid, stream, _, _ = c.profile_intervals()
    names = list(c.profile_get())
    return Counter((names[k], int(s)) for k, s in zip(kid, stream) if names[k] in SWEEP_CLASSES)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.NAMES)
def test_every_variant_gives_the_reference_flow_on_dirty_buffers(mav, fb_oracle, case):
    from mavflow import _lib
    W, H, B = case.W, case.H, case.batch
    prev, nxt = case.frames()
    pprev, pnxt = sc.poison_frames(W, H, B)
    # the dirtying call starts from a field of its own even where the case starts from zero: see schedule_cases.dirty
    init, pinit = case.initial_flow(), case.initial_flow(poison=True) if case.init else sc.poison_flow(W, H, B)

    with _lib.Context(W, H, B, case.fb(), window=case.window) as c:            # the reference: a fresh context, the plain schedule
        _set(c, sc.reference_options(B))
        info = c.schedule_info(B)
        assert all(l["sweeps"] == "one stream" and l["bands"] == 1 and l["pairs_per_launch"] == B for l in info["layers"]), info["layers"]
        ref = c.farneback(prev, nxt, initial_flow=init).copy()
    for b in range(B):
        exp = sc.expected_flow(case, fb_oracle, prev[b], nxt[b], None if init is None else init[b])
        e = tolerances.epe(ref[b], exp)
        print(f"\n[schedule forms] {case.name} pair {b} reference vs oracle: mean {e.mean():.3g} p99.9 {np.percentile(e, 99.9):.3g} max {e.max():.3g} px")
        tolerances.check_flow(ref[b], exp, tag=f"{case.name} pair {b}")        # strict gate: no twins, no pixel excused

    with _lib.Context(W, H, B, case.fb(), window=case.window) as c:
        dev = {"case": (c.alloc(prev.nbytes).upload(prev), c.alloc(nxt.nbytes).upload(nxt), None if init is None else c.alloc(init.nbytes).upload(init)),
               "poison": (c.alloc(prev.nbytes).upload(pprev), c.alloc(nxt.nbytes).upload(pnxt), None if init is None else c.alloc(pinit.nbytes).upload(pinit))}
        host = {"case": (prev, nxt, init), "poison": (pprev, pnxt, pinit)}
        out = c.alloc(ref.nbytes)
        unwritten = np.full(ref.nbytes, 0xFF, np.uint8)

        def run(entry, which):
            if entry == "host":
                p, n, i = host[which]
                return c.farneback(p, n, initial_flow=i)
            p, n, i = dev[which]
            out.upload(unwritten)
            c.farneback_dev(p.ptr, n.ptr, B, out.ptr, flow_init_ptr=None if i is None else i.ptr)
            c.sync()
            return out.download(np.float32, ref.shape)

        for v in case.variants:
            tag = f"{case.name} [{sc.variant_id(v)}]"
            _set(c, sc.options(B, {}))                                         # every option back to the library's default, then the variant's
            _set(c, v)
            # 1. the plan is the intended one
            info = c.schedule_info(B)
            assert {k: info[k] for k in v} == v, tag
            got_plan = [(l["sweeps"], l["pairs_per_launch"], l["bands"]) for l in info["layers"]]
            assert got_plan == sc.schedule_layers(case, v), tag
            assert [(l["w"], l["h"]) for l in info["layers"]] == [l[:2] for l in case.layers()], tag
            for rep in range(2):
                for entry in ("host", "dev"):
                    profiled = rep == 0 and entry == "host"
                    if profiled:
                        c.profile_enable(1)
                    run(entry, "poison")                                       # 2. dirty first
                    if profiled:
                        counts = _launch_counts(c)
                        c.profile_enable(0)
                        assert counts == sc.expected_launches(case, v), (tag, dict(counts), dict(sc.expected_launches(case, v)))
                    got = run(entry, "case")                                   # 3. compare
                    if entry == "dev":
                        left = (got.view(np.uint32) == 0xFFFFFFFF).any(-1)
                        assert not left.any(), (f"{tag}: {int(left.sum())} pixels were never written, first at (pair, y, x) = "
                                                f"{tuple(int(i) for i in np.argwhere(left)[0])}")
                    _same(got, ref, f"{tag} {entry} pointers, call {rep}")

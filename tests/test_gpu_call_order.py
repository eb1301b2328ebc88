"""A call's result does not depend on what its context ran before it: the families of tests/order_cases.py, light after heavy.

Context A runs a family's `light` call alone: the reference bytes L0, held to the family's numpy restatement where it has one (so A and
B cannot be wrong together).  Context B runs `heavy` -- which, by the table's CPU predicate, leaves strictly more behind than light
touches -- and then `light`: every output must be L0's, byte for byte; again after heavy twice, after light itself, after the
family's part-way refused forms, with the light input at every batch position of a max_batch call, and after every family's heavy call
on one context (the walk).  What is meant to persist -- the resident LK pyramid, a history ring, an accumulator -- must persist through
the other families' heavy calls.  Device forms run on the caller's own blocks, canary-filled and longer than promised
(order_cases.Dev).  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import order_cases as oc

pytestmark = pytest.mark.gpu


class Run:
    """one context and the state a family keeps on it between its calls"""

    def __init__(self, frame=oc.FRAME):
        from mavflow import _lib, _truth, _validation      # noqa: F401  (the last two attach their methods to Context)
        self.W, self.H = frame
        self.ctx, self.st = _lib.Context(self.W, self.H, oc.B), {}

    def heavy(self, fam):
        fam.heavy(self.ctx, self.st)

    def light(self, fam):
        return fam.light(self.ctx, self.st)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for v in self.st.values():
            if hasattr(v, "close"):
                v.close()
        self.ctx.close()


@functools.lru_cache(maxsize=None)
def reference(name, frame=oc.FRAME):
    """L0: the family's light call alone on a fresh context, computed once per frame size and shared; at order_cases.FRAME it is
    compared with the family's restatement (the walk's smaller frame has the same code under it and no restatement of its own)"""
    fam = oc.BY_NAME[name]
    with Run(frame) as a:
        L0 = a.light(fam)
    if fam.restate is not None and frame == oc.FRAME:
        fam.restate(L0, *frame)
    return L0


def _where(a, b):
    """where two comparable values part: the path through the tuples, then lengths and the first differing byte"""
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        if len(a) != len(b):
            return f"{len(a)} parts against {len(b)}"
        return "; ".join(f"[{i}] {_where(x, y)}" for i, (x, y) in enumerate(zip(a, b)) if x != y)
    if isinstance(a, bytes) and isinstance(b, bytes):
        if len(a) != len(b):
            return f"{len(a)} bytes against {len(b)}"
        d = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
        return f"{d.size} of {len(a)} bytes differ, the first at {int(d[0])}: {a[int(d[0]):int(d[0]) + 8].hex()} against {b[int(d[0]):int(d[0]) + 8].hex()}"
    return f"{a!r} against {b!r}"


def differing(got, want):
    return [f"{k}: only in one" for k in sorted(set(got) ^ set(want))] + [f"{k}: {_where(got[k], want[k])}" for k in want if k in got and got[k] != want[k]]


def same(got, want, what):
    bad = differing(got, want)
    assert not bad, f"{what}: {bad} differ from the fresh context's bytes"


@pytest.mark.parametrize("name", oc.NAMES)
def test_light_after_heavy(name):
    fam, L0 = oc.BY_NAME[name], reference(name)
    with Run() as b:
        b.heavy(fam)
        same(b.light(fam), L0, f"{name}: light after heavy")
        b.heavy(fam)
        b.heavy(fam)
        same(b.light(fam), L0, f"{name}: light after heavy, heavy")
        same(b.light(fam), L0, f"{name}: light after light")


@pytest.mark.parametrize("name", oc.WITH_REFUSAL)
def test_light_after_refused(name):
    """the part-way refused forms of resident_cases (order_cases.REFUSED_FORMS): on a fresh context, and between heavy and light"""
    fam, L0 = oc.BY_NAME[name], reference(name)
    with Run() as c:
        fam.refused(c.ctx, c.st)
        same(c.light(fam), L0, f"{name}: light after its refused forms")
        c.heavy(fam)
        fam.refused(c.ctx, c.st)
        same(c.light(fam), L0, f"{name}: light after heavy and its refused forms")


@pytest.mark.parametrize("name", oc.WITH_BATCH)
def test_batch_position(name):
    """a clear sized by the call's batch where the scratch is max_batch long: batch 1 after heavy at max_batch, then the light input at
    each position of a max_batch call among heavy inputs"""
    fam = oc.BY_NAME[name]
    with Run() as a:
        item = fam.batched(a.ctx, ["light"])[0]
    with Run() as b:
        b.heavy(fam)
        assert fam.batched(b.ctx, ["light"])[0] == item, f"{name}: batch 1 after heavy at max_batch"
        for pos in range(oc.B):
            items = ["heavy"] * oc.B
            items[pos] = "light"
            assert fam.batched(b.ctx, items)[pos] == item, f"{name}: the light input at batch position {pos}"
        assert fam.batched(b.ctx, ["light"] * oc.B) == [item] * oc.B, f"{name}: the light input at every position"


@pytest.mark.parametrize("third", list(oc.THIRDS))
def test_walk(third):
    """one context at 66 x 33: every family's heavy call in table order, then the light calls of this third, each against its
    fresh-context L0; then the heavy calls in reversed order and the light calls again, reversed"""
    mine = [f for i, f in enumerate(oc.FAMILIES) if oc.THIRDS[third](i)]
    L0 = {f.name: reference(f.name, oc.WALK_FRAME) for f in mine}
    with Run(oc.WALK_FRAME) as r:
        for heavy, light, what in ((oc.FAMILIES, mine, "in table order"), (oc.FAMILIES[::-1], mine[::-1], "in reversed order")):
            for f in heavy:
                r.heavy(f)
            for f in light:
                same(r.light(f), L0[f.name], f"{f.name}: light after every family's heavy call {what}")


def test_persistent_state_survives_every_other_family():
    """what is meant to persist -- the resident LK pyramid behind prev=None, a history ring between pushes, an accumulator between adds --
    still answers by its contract after the other families' heavy calls ran in between"""
    import history_cases as hc
    import history_ref
    W, H = oc.FRAME
    lk, rad = oc.lk_inputs(W, H), oc.radial_inputs(W, H)
    fields = [hc.smooth(W, H, 40 + i) for i in range(5)]
    with Run() as a:                                             # the uninterrupted sequences
        o, s = a.ctx.lk_track(lk["b"], lk["c"], lk["one"])
        want_lk = (o.tobytes(), s.tobytes(), a.ctx.lk_last_iterations().tobytes())
        ring = a.st["r"] = a.ctx.flow_history(oc.HIST_L)
        want_ring = [ring.push(f).tobytes() for f in fields]
        acc = a.st["acc"] = a.ctx.radial_error_accumulator(rad["lm"], rad["le"])
        acc.add(rad["one_f"], rad["one_g"], rad["one_s"])
        acc.add(rad["one_f"], rad["one_g"], None)
        want_acc = oc._hist(acc.counts())
    ref = history_ref.HistoryRef(H, W, oc.HIST_L, np.float32, "reference")
    assert want_ring == [ref.get_history(f).tobytes() for f in fields]
    with Run() as b:
        b.ctx.lk_track(lk["a"], lk["b"], lk["one"])             # b's pyramid becomes resident
        ring = b.st["r"] = b.ctx.flow_history(oc.HIST_L)
        got_ring = [ring.push(f).tobytes() for f in fields[:2]]
        acc = b.st["acc"] = b.ctx.radial_error_accumulator(rad["lm"], rad["le"])
        acc.add(rad["one_f"], rad["one_g"], rad["one_s"])
        for f in oc.FAMILIES:
            if f.name not in ("lk", "good_features"):            # (these two replace the resident frame: that is their contract)
                b.heavy(f)
        o, s = b.ctx.lk_track(None, lk["c"], lk["one"])
        assert (o.tobytes(), s.tobytes(), b.ctx.lk_last_iterations().tobytes()) == want_lk, "prev=None after the other families' heavy calls"
        b.heavy(oc.BY_NAME["lk"])
        b.heavy(oc.BY_NAME["good_features"])
        got_ring += [ring.push(f).tobytes() for f in fields[2:]]
        assert got_ring == want_ring, "a history ring between pushes"
        acc.add(rad["one_f"], rad["one_g"], None)
        assert oc._hist(acc.counts()) == want_acc, "an accumulator between adds"

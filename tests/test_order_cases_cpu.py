"""tests/order_cases.py against the three headers and the source as text, without a GPU: every entry point has exactly one place in
the table -- a family's pair of calls, EXEMPT with a reason, or (the six Farneback calls) DEFERRED --, every SCRATCH member exists in the struct it is attributed to and
the cited line says what its rule claims, every device pointer of those structs is listed, and every family's heavy call leaves
strictly more behind than its light call touches (leaves_more: a condition of the table's inputs, computed from the numpy
restatements -- a pair that misses it is a table bug)."""
import os
import re

import pytest

import order_cases as oc
import resident_cases as rc


def _placed(names, families=None, exempt=None):
    """(functions with no place or more than one, names of the table that no header declares)"""
    families = oc.FAMILIES if families is None else families
    exempt = oc.EXEMPT if exempt is None else exempt
    count = {n: int(n in exempt) for n in names}
    unknown = [e for e in exempt if e not in count]
    for entries in [f.entries for f in families] + list(oc.DEFERRED.values()):
        for e in entries:
            if e in count:
                count[e] += 1
            else:
                unknown.append(e)
    return sorted(n for n, k in count.items() if k != 1), sorted(unknown)


def test_every_entry_point_of_the_three_headers_has_exactly_one_place():
    names = oc.header_names()
    assert len(names) == len(set(names)) and len(names) > 155
    with open(rc.HEADER) as f:
        assert set(rc.header_functions(f.read())) < set(names)            # the other two headers add to mavflow.h's
    wrong, unknown = _placed(names)
    assert not wrong, f"in no family and not exempt, or in more than one place: {wrong}"
    assert not unknown, f"in the table but in no header: {unknown}"
    for e, why in oc.EXEMPT.items():
        assert isinstance(why, str) and why.strip(), e


def test_a_new_prototype_or_a_removed_family_is_noticed():
    names = oc.header_names()
    wrong, _ = _placed(names + ["mav_something_new_dev"])
    assert wrong == ["mav_something_new_dev"]
    for f in oc.FAMILIES:
        if f.entries:
            wrong, _ = _placed(names, [g for g in oc.FAMILIES if g is not f])
            assert wrong == sorted(f.entries), f.name
    wrong, _ = _placed(names, exempt={k: v for k, v in oc.EXEMPT.items() if k != "mav_sync"})
    assert wrong == ["mav_sync"]


def test_the_table_is_the_issue_s():
    assert len(oc.NAMES) == len(set(oc.NAMES))
    for want in ("detect", "detect refused", "components", "roc", "png", "good_features", "lk", "gt_stats", "radial", "history", "global_motion",
                 "pyramid"):
        assert want in oc.BY_NAME, want
    # nothing but the six Farneback entry points is deferred, and nothing hides there
    assert list(oc.DEFERRED) == ["farneback"] and all(re.fullmatch(r"mav_farneback(_init|_ex)?(_dev)?", e) for e in oc.DEFERRED["farneback"])
    assert len(oc.DEFERRED["farneback"]) == 6 and not set(oc.DEFERRED) & set(oc.BY_NAME)
    assert oc.FRAME == (131, 67) and oc.WALK_FRAME == (66, 33) and oc.B == 3
    thirds = [sum(1 for i in range(len(oc.FAMILIES)) if sel(i)) for sel in oc.THIRDS.values()]
    assert sum(thirds) == len(oc.FAMILIES) and min(thirds) >= 4
    # the refused forms are resident_cases' part-way refused ones, by name; the refusal variant is the detect family's, where heavy stands
    forms = {f.name for f in rc.FORMS}
    part_way = rc.FRESH_BEFORE_REFUSAL | rc.ENQUEUED_BEFORE_REFUSAL
    assert set(oc.REFUSED_FORMS) == set(oc.WITH_REFUSAL) and len(oc.WITH_REFUSAL) >= 4
    for fam, names in oc.REFUSED_FORMS.items():
        for n in names:
            assert n in forms and n in part_way, (fam, n)
    assert rc.ENQUEUED_BEFORE_REFUSAL <= set(oc.REFUSED_FORMS["detect"])
    assert oc.BY_NAME["detect refused"].heavy is oc.BY_NAME["detect"].refused and oc.BY_NAME["detect refused"].light is oc.BY_NAME["detect"].light
    # every family whose calls take a batch has a batched form (the others take one frame, one ring or one table per call)
    assert set(oc.NAMES) - set(oc.WITH_BATCH) == {"detect refused", "good_features", "lk", "radial", "history"}


@pytest.mark.parametrize("frame", [oc.FRAME, oc.WALK_FRAME], ids=lambda f: f"{f[0]}x{f[1]}")
def test_the_inputs_exist_at_both_frames(frame):
    """every family's inputs are functions of the frame: the walk's 66 x 33 builds them all, with the shapes the calls take"""
    W, H = frame
    x = oc.detect_inputs(W, H)
    assert x["flow"].shape == (oc.B, H, W, 2) and x["l_flow"].shape == (1, H, W, 2) and x["prev"].shape == x["next"].shape == (oc.B, H, W)
    g = oc.gts_inputs(W, H)
    assert g["seg"].shape == (oc.B, H, W) and int((g["one"] > 127).sum()) == 1 and int((g["empty"] > 127).sum()) == 0
    r = oc.radial_inputs(W, H)
    assert r["flow"].shape == r["gt"].shape == (oc.B, H, W, 2) and r["one_f"].shape == (1, H, W, 2)
    m = oc.gm_inputs(W, H)
    assert m["coords"].shape == (oc.GM_HEAVY_PAIRS, 2) and (m["coords"] >= 0).all() and (m["coords"] < (W, H)).all()
    assert (m["few"] >= 0).all() and (m["few"] < (W, H)).all() and len({tuple(c) for c in m["few"]}) == oc.GM_LIGHT_PAIRS
    p = oc.pyr_inputs(W, H)
    assert p["heavy"].shape == (oc.B, H, W) and p["win"].shape == (oc.B, 4) and p["l_win"].shape == (1, 4)
    k = oc.lk_inputs(W, H)
    assert k["pts"].shape == (oc.LK_HEAVY_POINTS, 2) and k["a"].shape == k["b"].shape == k["c"].shape == (H, W)
    noise, flat = oc.png_images(W, H)
    assert noise.shape == (oc.B, H, W, 4) and flat.shape == (1, H, W)
    assert oc.cc_case(oc.CC_HEAVY, 8, W, H).masks.shape == (oc.B, H, W)


@pytest.mark.parametrize("s", oc.SCRATCH, ids=lambda s: s.key)
def test_scratch_member_exists_and_its_line_says_what_the_rule_claims(s):
    assert s.rule in oc.RULES, s.rule
    assert re.search(rf"\b{re.escape(s.member)}\b", oc.struct_body(s.struct)), f"struct {s.struct} has no member {s.member}"
    with open(os.path.join(oc.CSRC, s.file)) as f:
        lines = f.read().split("\n")
    assert 1 <= s.line <= len(lines) and re.search(s.pattern, lines[s.line - 1]), f"{s.file}:{s.line} reads {lines[s.line - 1].strip()!r}"
    for w in s.writers:
        assert w in oc.BY_NAME or w in oc.DEFERRED, f"{s.key}: no family {w!r}"
    # what the rule claims, in the words of the line
    line = lines[s.line - 1]
    if s.rule == "memset per call":
        assert "hipMemsetAsync" in line, s.key
    elif s.rule == "init kernel":
        assert re.search(r"k_gts_init|= 0ull|= INT_MAX", line), s.key
    elif s.rule == "self-resetting":
        assert re.search(r"atomic_store\(.*, 0u", line), s.key
    if s.guard:
        mod, fn = s.guard.split(".")
        assert callable(getattr(__import__(mod), fn))


def test_every_device_pointer_of_the_structs_is_listed():
    keys = [s.key for s in oc.SCRATCH]
    assert len(keys) == len(set(keys))
    listed = {}
    for s in oc.SCRATCH:
        listed.setdefault(s.struct, set()).add(s.member)
    assert set(listed) == set(oc.STRUCTS)
    for struct in oc.STRUCTS:
        ptrs = oc.device_pointers(struct)
        assert len(ptrs) >= 1, struct
        missing = ptrs - listed[struct] - set(oc.NOT_SCRATCH[struct])
        assert not missing, f"struct {struct}: device pointers {sorted(missing)} are in neither SCRATCH nor NOT_SCRATCH"
        extra = (listed[struct] | set(oc.NOT_SCRATCH[struct])) - ptrs - {"scratch"}          # (scratch: a vector of blocks, no bare pointer)
        assert not extra, f"struct {struct}: {sorted(extra)} are no pointer members"
    # removing an entry is noticed
    assert "gts_scratch" in oc.device_pointers("mav_ctx") and "done" in oc.device_pointers("FoeScratch") and "ring" in oc.device_pointers("mav_history")
    used = {w for s in oc.SCRATCH for w in s.writers}
    assert used >= set(oc.NAMES) - {"detect refused"}, sorted(set(oc.NAMES) - used)


def test_the_cited_clears_are_the_ones_the_source_has():
    """every hipMemsetAsync of mavflow.cpp on a member of the context is cited by a SCRATCH entry or is a lifecycle clear"""
    with open(os.path.join(oc.CSRC, oc.CPP)) as f:
        lines = f.read().split("\n")
    cited = {s.line for s in oc.SCRATCH if s.file == oc.CPP}
    lifecycle = {"buf[i]": "mav_membw_probe's own buffers", "h->ring, 0, h->ring_bytes, c->stream) != hipSuccess": "mav_history_create",
                 "blobs, 0, sizeof(mav_blob)": "the caller's table", "k.counters, 0, 2 * sizeof(unsigned)": "the corner counters: LkState.counters' other clear"}
    for i, line in enumerate(lines, 1):
        if "hipMemsetAsync(" in line and i not in cited:
            assert any(k in line for k in lifecycle), f"{oc.CPP}:{i} clears something no SCRATCH entry cites: {line.strip()}"


@pytest.mark.parametrize("name", oc.NAMES)
def test_heavy_leaves_more_than_light_touches(name):
    assert oc.BY_NAME[name].leaves_more() is True, f"{name}: the heavy call does not leave more behind than the light call touches"

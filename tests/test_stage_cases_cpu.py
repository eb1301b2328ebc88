"""The layer-image part of the stage table (tests/stage_cases.py: blur_form, BLUR_FORMS, BLUR_CASES) is what it claims to be --
checked from the restated predicates alone, without a GPU.  tests/test_gpu_blur_forms.py ties the restatement to the library through
mav_schedule_info's names and runs every form."""
import stage_cases as sc


def test_every_blur_form_is_reached_by_a_case():
    reached = set()
    for c in sc.BLUR_CASES:
        got = {f for f, _, _ in sc.blur_case_forms(c)}
        assert c.expects <= got, (c.name, sorted(c.expects - got))
        reached |= got
    untested = sc.UNTESTED["blur_form"]
    assert sc.BLUR_FORMS == reached, sorted(sc.BLUR_FORMS ^ reached)
    assert not (untested & reached)
    assert any(c.W % 64 and c.W % 4 and c.H % 16 for c in sc.BLUR_CASES)          # a ragged frame stays in the table


def test_predicates_at_the_shapes_they_were_chosen_for():
    """the launchers' arithmetic at the table's shapes, spelled out: a changed constant in kernels_flow.hip must change these too"""
    assert sc.pyramid(80, 80, 0.4, 1) == [(80, 80, 3), (32, 32, 5)] and sc.pyramid(79, 80, 0.4, 1) == [(79, 80, 3)]
    assert sc.pyramid(200, 200, 0.4, 2) == [(200, 200, 3), (80, 80, 5), (32, 32, 13)]
    assert sc.pyramid(200, 200, 0.178, 1)[1] == (36, 36, 13) and sc.pyramid(1600, 1600, 0.02, 1)[1] == (32, 32, 123)
    assert sc.pyramid(3840, 2160, 0.4, 5)[1:] == [(1536, 864, 5), (614, 346, 13), (246, 138, 37), (98, 55, 95)]
    # 13 taps: the thin margin of the 64 x 16 tile, and the 64 x 8 tile where that is past 64 KB
    th, rows, pitch, lds, fast = sc.fused_plan(200, 200, 36, 36, 13, True, 1)
    assert (th, fast, lds) == (16, True, 64740) and lds <= sc.LDS_DEFAULT
    th, rows, pitch, lds, fast = sc.fused_plan(200, 200, 32, 32, 13, True, 1)
    assert (th, fast) == (8, True) and sc.fused_lds_bytes(sc.fused_blur_rows(200, 32, 13), pitch, 1) > sc.LDS_DEFAULT >= lds
    assert sc.fused_plan(202, 200, 32, 32, 13, False, 1)[2] == 0                   # no fast tile: unstaged
    assert not sc.blur_is_fused(200, 200, 32, 32, 13, 2) and sc.blur_is_fused(200, 200, 32, 32, 13, 1)
    assert sc.blur_is_fused(80, 80, 32, 32, 5, 4) and not sc.blur_is_fused(3840, 2160, 246, 138, 37, 1)
    # the two-pass row block: 16, 8 or 4 rows in 48 KB, else the direct kernel
    assert [sc.two_pass_rows_blk(1600, 32, 123, e) for e in (1, 2, 4)] == [8, 4, 0]
    assert sc.two_pass_rows_blk(3840, 98, 95, 1) == 16


def test_blur_form_meets_nothing_outside_the_table():
    """blur_form over pyr_scale 0.01 .. 0.95, up to five levels, widths with W % 4 == 0 and == 2 up to 8192 at two aspect ratios, the
    three depths, dispatched and forced two-pass: every form it meets is in BLUR_FORMS.  In particular nothing selects
      * the 5-tap fast tile at 64 x 8 (a 5-tap layer's staged 64 x 16 region fits 64 KB at every depth),
      * the 13-tap fast tile, or any 13-tap fused tile, for 2- and 4-byte pixels (blur_resize_is_fused refuses them),
      * blur_h4's 5-tap branch (the unstaged tile and the direct kernel run only behind 13 and more taps)."""
    widths = sorted(set(range(32, 256, 2)) | set(range(256, 8193, 38)) | {8190, 8192})
    assert {w % 4 for w in widths} == {0, 2}
    met = set()
    for W in widths:
        for H in {W, max(32, W * 9 // 16)}:
            for s in range(1, 96):
                for layer in sc.pyramid(W, H, s / 100.0, 5):          # (the pyramids of fewer levels are its prefixes)
                    for d in sc.DEPTHS:
                        met.add(f"{d}:{sc.blur_form(W, H, layer, d)}")
                        met.add(f"{d}:{sc.blur_form(W, H, layer, d, True)}")
    assert met <= sc.BLUR_FORMS | sc.UNTESTED["blur_form"], sorted(met - sc.BLUR_FORMS)
    assert sc.UNTESTED["blur_form"] <= met                              # reachable, from frames too large for a test
    for f in met:
        depth, form = f.split(":")
        assert form not in ("fused/fast5/th8", "fused/generic/unstaged/ks5", "two-pass/direct/ks5"), f
        assert depth == "u8" or "13" not in form and "unstaged" not in form, f

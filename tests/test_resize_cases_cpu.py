"""The case table of the image resize (tests/resize_cases.py) held to the sources and to a pure-Python mirror of the host's dispatch:
every kernel form csrc/kernels_resize.hip can be instantiated as is reached by a run of the table, the forms and formats the table
names are the ones the sources name, and the shapes the issue lists are in the table with what they are there to reach.  Fails when a
form is no longer reached.  Runs without a GPU."""
import numpy as np

import resize_cases as T
import resize_ref as R


def test_the_table_names_what_the_sources_name(mav):
    from mavflow import resize as K
    s = T.source_forms()
    assert s["enum"] == list(T.FORMS)                                     # RS_* of mavflow_internal.h, in its order
    assert s["formats"] == set(T.FORMATS)
    assert s["dispatched"] == {f.upper() for f in T.FORMS}
    assert "atomic" not in s["text"] and "printf" not in s["text"] and "assert(" not in s["text"]
    assert "__shared__" not in s["text"]                                   # no LDS staging
    assert sorted(K.EXPORTS) == ["mav_resize", "mav_resize_dev", "mav_sky_mask", "mav_sky_mask_dev"]


def test_every_kernel_form_is_reached(mav):
    from mavflow import resize as K
    assert K.INTER_AREA == R.AREA
    reached = {}
    for shape in T.SHAPES:
        for run in T.runs(shape):
            reached.setdefault(T.form_reached(run), run)
    for run in T.sky_runs():
        reached.setdefault(T.form_reached(run, sky=True), run)
    missing = T.kernel_forms() - set(reached)
    assert not missing, sorted(missing)
    assert set(reached) == T.kernel_forms()                               # and the mirror names no form the kernel file lacks


def test_the_listed_shapes_reach_what_they_are_listed_for(mav):
    from mavflow import resize as K
    assert K.INTER_LINEAR == R.LINEAR
    shapes = {(s.src, s.dst) for s in T.SHAPES}
    listed = [((1, 1), (5, 3)), ((2, 2), (7, 5)), ((1, 9), (3, 30)), ((13, 1), (40, 6)), ((5, 3), (67, 4)), ((33, 17), (65, 70)), ((64, 48), (37, 29)),
              ((64, 48), (32, 24)), ((63, 48), (21, 16)), ((60, 45), (40, 30)), ((20, 12), (20, 12))]
    assert set(listed) <= shapes
    form = lambda fmt, s, d, i: R.form_of(fmt, s[0], s[1], d[0], d[1], i)
    assert R.linear_table(5, 1, 1 / 5)[2].all() and R.linear_table(3, 1, 1 / 3)[2].all()            # one tap everywhere
    assert not R.linear_table(7, 2, 2 / 7)[2].all()                                                   # two taps
    assert R.linear_table(3, 1, 1 / 3)[2].all() and not R.linear_table(30, 9, 9 / 30)[2].all()        # one source column: one tap horizontally only
    # a lane owns PX pixels, so a row of 64 lanes is 256 (128 for F32C2) pixels: 263 crosses it with a ragged tail in every format
    assert ((9, 2), (263, 3)) in shapes and all(263 > 64 * px and 263 % px for px in R.PX.values())
    assert 70 > 4 and 29 > 4                                                                          # more than one workgroup of 4 rows
    for fmt in R.FORMATS:
        u8 = R.FORMATS[fmt][0] == np.uint8
        assert form(fmt, (64, 48), (37, 29), R.LINEAR) == "linear" and form(fmt, (64, 48), (37, 29), R.AREA) == "area_general"
        assert form(fmt, (64, 48), (32, 24), R.LINEAR) == form(fmt, (64, 48), (32, 24), R.AREA) == ("area_2x2" if u8 else "area_fast")
        assert form(fmt, (64, 48), (32, 24), R.NEAREST) == "nearest"
        assert form(fmt, (63, 48), (21, 16), R.AREA) == "area_fast" and form(fmt, (48, 20), (12, 10), R.AREA) == "area_fast"
        assert form(fmt, (60, 45), (40, 30), R.AREA) == "area_general"
        for i in (R.NEAREST, R.LINEAR, R.AREA):
            assert form(fmt, (20, 12), (20, 12), i) == "copy"
    widths = {s.dst[0] for s in T.SHAPES}
    assert any(w % 4 == 0 for w in widths) and any(w % 4 for w in widths) and any(w % 2 for w in widths)
    assert T.B == 3


def test_the_store_path_mirror(mav):
    from mavflow import resize as K
    assert K.MAX_SIDE == R.MAX_SIDE
    for fmt in (R.U8C1, R.U8C3):
        assert R.vector_stores(fmt, 40, 0) and R.vector_stores(fmt, 40, 4) and not R.vector_stores(fmt, 40, 1) and not R.vector_stores(fmt, 37, 0)
    assert R.vector_stores(R.F32C1, 40, 0) and not R.vector_stores(R.F32C1, 40, 4) and not R.vector_stores(R.F32C1, 42, 0)
    assert R.vector_stores(R.F32C2, 42, 16) and not R.vector_stores(R.F32C2, 42, 8) and not R.vector_stores(R.F32C2, 21, 0)
    assert R.vector_stores(R.U8C3, 20, 8, sky=True) and not R.vector_stores(R.U8C3, 20, 1, sky=True)


def test_the_inputs_carry_what_they_are_noted_for(mav):
    from mavflow import resize as K
    assert K.SKY_KEY == T.SKY
    for fmt in (R.F32C1, R.F32C2):
        a = T.images(fmt, 33, 17)
        assert np.isnan(a[0]).sum() == 1 and np.isinf(a[0]).sum() == 1 and np.isfinite(a[1:]).all()
    for fmt in (R.U8C1, R.U8C3):
        a = T.images(fmt, 33, 17)
        assert set(np.unique(a[0])) == {0, 255} and a[1].min() < 8 and a[1].max() > 247
    # the prediction: the key occurs in flat regions, and the interpolated picture has the key where no source pixel has it
    p = T.prediction(60, 32)
    src_key = (p[..., 0] == 180) & (p[..., 1] == 130)
    assert src_key[0].any() and not src_key[0].all()
    big = R.resize(p[0], 120, 64, R.LINEAR)
    mask = R.sky_mask(p[0], 120, 64)
    assert mask.any() and not mask.all()
    one_channel = ((big[..., 0] == 180) ^ (big[..., 1] == 130))
    assert one_channel.any()                                              # a blend that passes through the key in one channel alone: not sky
    assert not mask[one_channel].any()

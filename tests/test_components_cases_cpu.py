"""The case table of the connected-components tests reaches every form of csrc/kernels_components.hip: the predicates of
tests/components_cases.py restate each dispatch decision, and this test fails when a form is no longer reached."""
import numpy as np

import components_cases as CC


def test_the_frames_and_patterns_the_table_promises():
    T_W, T_H = CC.T_W, CC.T_H
    assert CC.FRAMES == [(1, 1), (1, 37), (37, 1), (2, 2), (T_W, T_H), (T_W + 1, T_H + 1), (2 * T_W - 1, 3 * T_H + 1), (131, 67)]
    for (W, H) in CC.FRAMES:
        pats = CC.patterns(W, H)
        assert {"empty", "full", "corners", "checker", "serpentine", "serpentine_t", "spiral", "comb", "tile_checker", "corner_pairs",
                "rings", "values", "noise_05", "noise_41", "noise_59", "noise_90"} == set(pats)
        for name, m in pats.items():
            assert m.shape == (H, W) and m.dtype == np.uint8 and m.flags.c_contiguous, name
        assert not pats["empty"].any() and pats["full"].all()
        for conn in (4, 8):
            assert f"{W}x{H}-all-c{conn}" in CC.BY_ID
    big = CC.patterns(131, 67)
    assert set(np.unique(big["values"])) == {0, 7, 128, 255}
    for d, name in zip(CC.DENSITIES, ("noise_05", "noise_41", "noise_59", "noise_90")):
        assert abs(big[name].mean() - d) < 0.02
    # the checkerboard: ceil(W H / 2) components under 4-connectivity, one under 8
    c4, c8 = CC.BY_ID["131x67-all-c4"], CC.BY_ID["131x67-all-c8"]
    k = c4.names.index("checker")
    assert c4.expected[1]["n_components"][k] == -(-131 * 67 // 2) and c8.expected[1]["n_components"][k] == 1
    # serpentine, spiral and comb are single long components; the tile checkerboard and the corner pairs tell 4 from 8
    for name in ("serpentine", "serpentine_t", "spiral", "comb"):
        assert c4.expected[1]["n_components"][c4.names.index(name)] == 1, name
    for name in ("tile_checker", "corner_pairs"):
        k = c4.names.index(name)
        assert c8.expected[1]["n_components"][k] < c4.expected[1]["n_components"][k], name
    k = c8.names.index("rings")
    assert c8.expected[1]["n_components"][k] > 1                       # nested rings stay distinct
    assert {c.masks.shape[0] for c in CC.CASES} >= {1, 3}


def test_every_dispatch_form_is_reached():
    tiles, merges, stats, subs, trunc, filt = set(), {4: set(), 8: set()}, set(), set(), set(), set()
    for c in CC.CASES:
        tiles |= CC.tile_kinds(c.W, c.H)
        labels, counts, tables = c.expected
        for b, m in enumerate(c.masks):
            merges[c.connectivity] |= CC.merge_kinds(m, c.connectivity)
            if c.W * c.H >= 4096:
                stats |= CC.stats_kinds(labels[b], tables[b])
            trunc.add(bool(counts[b]["n_blobs"] > c.max_blobs))
            filt.add("all" if counts[b]["n_blobs"] == counts[b]["n_components"] else "none" if counts[b]["n_blobs"] == 0 else "some")
        subs.add(min(c.sub_batches(CC.workspace_per_image(c.W, c.H)), 2))
    assert tiles == {"interior", "edge"}
    assert merges[4] == {"horizontal", "vertical"} and merges[8] == {"horizontal", "vertical", "corner"}
    assert stats == {"uniform", "mixed"}
    assert subs == {1, 2}                                              # one sub-batch, several
    assert trunc == {False, True} and filt == {"all", "some", "none"}
    # labels requested vs NULL: tests/test_gpu_components.py runs every case both ways (host and device pointers)
    assert (CC.T_W, CC.T_H) in CC.FRAMES and CC.tile_kinds(CC.T_W, CC.T_H) == {"interior"}
    assert CC.workspace_per_image(1920, 1080) == 16653824              # 8 B per pixel + 8 B per chunk, rounded up to 256: 8.03 B per pixel


def test_the_references_are_computed_once_and_read_only():
    c = CC.BY_ID["131x67-b1-c8"]
    assert c.expected is c.expected
    assert not any(a.flags.writeable for a in c.expected)

"""The schedule table (tests/schedule_cases.py) is what it claims to be -- checked on the restated scheduler alone, without a GPU:
every case reaches the forms it names and every form of FORMS is reached; the restated band walk sweeps every tile row once per sweep,
builds a band's initial M where its first sweep reads, and never lets a sweep read a row of M that is not the previous sweep's; the
restated tile map sends the workgroups of a grid onto the tiles of the launch one to one.  tests/test_gpu_schedule_forms.py ties the
restatement to the library."""
import numpy as np
import pytest

import schedule_cases as sc

PAIRS = [(c, v) for c in sc.CASES for v in c.variants]
PAIR_IDS = [f"{c.name}[{sc.variant_id(v)}]" for c, v in PAIRS]


def test_every_form_is_reached_by_a_case_that_names_it():
    reached, named = set(), set()
    for c in sc.CASES:
        got = set().union(*(sc.forms_reached(c, v) for v in c.variants))
        assert c.expects <= got, (c.name, sorted(c.expects - got))
        assert got <= sc.ALL_FORMS, (c.name, sorted(got - sc.ALL_FORMS))
        reached |= got
        named |= c.expects
    assert sc.ALL_FORMS - sc.ALL_UNTESTED == reached, sorted(sc.ALL_FORMS - sc.ALL_UNTESTED - reached)
    assert sc.ALL_FORMS - sc.ALL_UNTESTED == named, sorted(sc.ALL_FORMS - sc.ALL_UNTESTED - named)
    assert not (sc.ALL_UNTESTED & reached) and sc.ALL_UNTESTED <= sc.ALL_FORMS
    assert len(set(sc.NAMES)) == len(sc.NAMES)
    assert all(c.W * c.H <= 300_000 and c.winsize // 2 == 6 for c in sc.CASES)       # small frames, the sweep forms that have bands
    # a sweep form without bands reports J = 1 whatever is asked for
    for c, v in PAIRS:
        for sg in sc.call_walk(c, v):
            assert sg.plan.J == 1 or sc.sweep_form(c.layers()[sg.k][0]) == "fast<6>", (c.name, v)


def test_restatement_at_the_shapes_it_was_chosen_for():
    """plan_sweeps and bound() at the table's shapes, spelled out: a changed constant in the scheduler must change these too"""
    by = {c.name: c for c in sc.CASES}
    J = lambda name, **v: [b for _, _, b in sc.schedule_layers(by[name], v)]
    assert J("68x100-I1", bands=2, pairs_in_flight=1) == [2] and J("68x100-I1", bands=3, pairs_in_flight=1) == [1]
    assert J("68x100-I1", bands=3, pairs_in_flight=2) == [2]                          # T = 7: Jmax = 2 clips, where one stream falls back
    assert J("132x370-I1-J8", bands=8, pairs_in_flight=1) == [8] == J("132x370-I1-J8", bands=8, pairs_in_flight=2)
    assert J("132x384-I10", bands=2, pairs_in_flight=1) == [2] and J("132x368-I10", bands=2, pairs_in_flight=1) == [1]
    assert J("132x368-I10", bands=2, pairs_in_flight=2) == [1]
    assert J("132x384-L1-I10", bands=2) == [2, 1] and J("2622x52-b3", bands=2, group_fine=1) == [1]
    assert sc.band_bounds(13, 2, 3, False, -1) == ([0, 4, 8, 13], {"plain"})
    assert sc.band_bounds(13, 2, 3, False, 64) == ([0, 11, 12, 13], {"clamp-hi"})
    assert sc.band_bounds(13, 2, 3, True, -1)[0] == [0, 2, 6, 10, 13]
    assert sc.band_bounds(24, 10, 2, False, -1)[0] == [0, 16, 24] and sc.band_bounds(24, 10, 2, True, -1)[0] == [0, 6, 18, 24]
    assert sc.band_bounds(12, 4, 2, True, -1)[0] == [0, 3, 9, 12]
    assert sc.band_bounds(19, 3, 3, False, 0)[0] == [0, 6, 12, 19] and sc.band_bounds(19, 3, 3, False, -1)[0] == [0, 7, 13, 19]
    assert sc.band_bounds(2, 1, 3, False, 0) == ([0, 1, 2, 2], {"clamp-lo"})      # what plan_sweeps never grants
    shifted = sc.band_walk(384, 10, 2, True, -1, True)
    assert shifted[0].skipped == [6, 7, 8, 9] and shifted[1].launches[7][:2] == (7, 0) and shifted[0].m_rows == (0, 104)
    assert shifted[1].m_rows == (88, 296) and shifted[2].m_rows == (280, 384)
    assert sc.band_walk(192, 4, 2, True, -1, True)[0].skipped == [3]
    # strips: 41 tiles across split 21 + 20; 3 images of 41 x 4 tiles pad to a grid of 496
    tm = sc.make_tile_map(2624, 52, 3)
    assert (tm.tiles_x, tm.tiles_y, tm.n_tiles, tm.strip_w, sc.tile_grid(tm)) == (41, 4, 492, 21, 496)
    assert [sc.make_tile_map(2624, 52, 3, strip=s).strip_w for s in (1, 7, 41, 1 << 20)] == [1, 7, 41, 41]
    assert sc.make_tile_map(2624, 100, 1, 3, 7, 7) == sc.TileMap(41, 4, 164, 164, 7, 3)
    assert sc.make_tile_map(132, 100, 1, 5, 9).tiles_y == 2 and sc.make_tile_map(132, 100, 1, 9, 12).n_tiles == 0


@pytest.mark.parametrize("case,variant", PAIRS, ids=PAIR_IDS)
def test_band_walk_covers_every_tile_row_once_and_reads_what_was_written(case, variant):
    layers, I = case.layers(), case.iterations
    walk = sc.call_walk(case, variant)
    # every pair of the call is swept on every layer, once: the sub-groups of a group follow each other and cut [0, g)
    for k in range(len(layers)):
        assert sum(sg.gs for sg in walk if sg.k == k) == case.batch, k
    for a, b in zip(walk, walk[1:] + [None]):
        assert a.gs >= 1 and a.s0 + a.gs <= a.g
        if b is not None and b.k == a.k and b.s0 > 0:
            assert b.s0 == a.s0 + a.gs and b.g == a.g
        else:
            assert a.s0 + a.gs == a.g and (b is None or b.s0 == 0)
    for i, sg in enumerate(walk):
        h, T = layers[sg.k][1], sc.tile_rows(layers[sg.k][1])
        # the M slots of the sub-group lie inside the group's, and two sub-groups in flight at once do not share one
        assert 0 <= sg.slot and sg.slot + sg.gs <= max(sg.g, 1), (sg.slot, sg.gs, sg.g)
        if sg.plan.streams == 2 and i + 1 < len(walk) and walk[i + 1].k == sg.k and walk[i + 1].s0 == sg.s0 + sg.gs:
            nxt = walk[i + 1]
            assert nxt.stream != sg.stream and (nxt.slot >= sg.slot + sg.gs or sg.slot >= nxt.slot + nxt.gs)
        # every sweep: the bands' launches cut [0, T) into consecutive pieces
        for it in range(I):
            pieces = sorted((ty0, ty1) for b in sg.bands for s, ty0, ty1 in b.launches if s == it)
            assert pieces[0][0] == 0 and pieces[-1][1] == T and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])), (it, pieces)
            assert all(ty1 > ty0 for ty0, ty1 in pieces)
        # a band's own initial M holds what its first sweep reads: its rows and the 6-pixel halo, clipped to the image
        for b in sg.bands:
            assert b.launches and b.launches[0][0] == 0, b
            if b.m_rows is not None:
                _, ty0, ty1 = b.launches[0]
                assert b.m_rows[0] <= max(16 * ty0 - sc.HALO, 0) and min(16 * ty1 + sc.HALO, h) <= b.m_rows[1], b
        assert all((b.m_rows is not None) == (sg.plan.m_build == "band") for b in sg.bands)
        # the ping-pong, row by row: Ma / Mb hold the number of the sweep whose input a row is (-1: another call's data).  In launch order
        # every sweep must find its rows and halo at its own number, and the last sweep must store every row of the flow once.
        M = [np.full(h, -1), np.full(h, -1)]
        flow = np.zeros(h, int)
        if sg.plan.m_build != "band":
            M[0][:] = 0
        for b in sg.bands:
            if b.m_rows is not None:
                M[0][b.m_rows[0]:b.m_rows[1]] = 0
            for it, ty0, ty1 in b.launches:
                src, dst = M[it & 1], M[1 - (it & 1)]
                read = src[max(16 * ty0 - sc.HALO, 0):min(16 * ty1 + sc.HALO, h)]
                assert (read == it).all(), (case.name, variant, sg.k, b.j, it, ty0, ty1, read.tolist())
                if it < I - 1:
                    dst[16 * ty0:min(16 * ty1, h)] = it + 1
                else:
                    flow[16 * ty0:min(16 * ty1, h)] += 1
        assert (flow == 1).all()


@pytest.mark.parametrize("case,variant", PAIRS, ids=PAIR_IDS)
def test_tile_map_is_a_bijection_for_every_launch(case, variant):
    """every strip value and band launch of the table: the workgroups of the grid hit each (image, ty, tx) of the launch once, nothing
    outside it, and the grid is the tile count rounded up to the 8 XCDs"""
    launches = sc.sweep_launches(case, variant)
    assert launches
    for w, h, G, ty0, ty1, strip in launches:
        tm = sc.make_tile_map(w, h, G, ty0, ty1, strip)
        grid = sc.tile_grid(tm)
        assert grid % 8 == 0 and tm.n_tiles <= grid < tm.n_tiles + 8 and tm.n_tiles > 0
        hit = [sc.tile_of_block(tm, b, grid) for b in range(grid)]
        tiles = [t for t in hit if t is not None]
        hi = sc.tile_rows(h) if ty1 < 0 else ty1
        want = {(s, tx, ty) for s in range(G) for ty in range(ty0, hi) for tx in range((w + 63) // 64)}
        assert len(tiles) == len(set(tiles)) == tm.n_tiles and set(tiles) == want, (w, h, G, ty0, ty1, strip)
        assert hit.count(None) == grid - tm.n_tiles


def test_expected_launches_count_what_the_walk_holds():
    by = {c.name: c for c in sc.CASES}
    n = sc.expected_launches(by["132x384-I10"], {"pairs_in_flight": 2, "bands": 2, "band_phase": 1})
    # stream 0: bands [0, 16), [16, 24) of ten sweeps; stream 1: [0, 6) six sweeps, [6, 18) and [18, 24) ten each
    assert n == {("update_matrices", 0): 2, ("blur_iter", 0): 20, ("update_matrices", 1): 3, ("blur_iter", 1): 26}
    n = sc.expected_launches(by["132x384-L1-b5"], {"group": 5, "coarse_half": 2, "bands": 2})
    assert n[("blur_iter_coarse", 0)] == 6 and n[("blur_iter_coarse", 1)] == 3                 # sub-groups 2, 2, 1 of three sweeps
    n = sc.expected_launches(by["132x100-b3"], {"pairs_in_flight": 1, "group_fine": 0})
    assert n == {("update_matrices", 0): 1, ("blur_iter", 0): 1}


@pytest.mark.parametrize("case", sc.CASES, ids=sc.NAMES)
def test_poison_is_another_picture_everywhere(case):
    """The frames that dirty the buffers: their flow differs from the case's at every pixel of every slot (the oracle's flows; where
    the oracle cannot be built, the frames differ), so that a pixel left over from the dirtying call cannot pass for the case's."""
    prev, nxt = case.frames()
    pprev, pnxt = sc.poison_frames(case.W, case.H, case.batch)
    assert prev.shape == pprev.shape == (case.batch, case.H, case.W) and prev.dtype == pprev.dtype
    assert (prev != pprev).mean() > 0.9 and (nxt != pnxt).mean() > 0.9
    for b in range(1, case.batch):                                     # distinct pairs: a neighbour's M is a wrong M
        assert (prev[b] != prev[0]).mean() > 0.5 and (pprev[b] != pprev[0]).mean() > 0.5
    try:
        from oracle import fb_oracle
        orc = fb_oracle.load()
    except OSError:
        return
    init, pinit = case.initial_flow(), case.initial_flow(poison=True)
    for b in range(case.batch):
        a = sc.expected_flow(case, orc, prev[b], nxt[b], None if init is None else init[b])
        p = sc.expected_flow(case, orc, pprev[b], pnxt[b], None if pinit is None else pinit[b])
        same = (a == p).all(-1)
        assert not same.any(), (case.name, b, int(same.sum()))
        if init is None and case.window == "box":                      # ... and started from the noise field of schedule_cases.dirty
            p = sc.expected_flow(case, orc, pprev[b], pnxt[b], sc.poison_flow(case.W, case.H, case.batch)[b])
            assert not (a == p).all(-1).any(), (case.name, b)

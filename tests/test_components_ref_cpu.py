"""tests/components_ref.py (the contract of mav_components restated) against scipy.ndimage.label on every case of the table, a few
hand-written expectations, and the hull property that ties the blob boxes to get_simple_bounding_box."""
import numpy as np
import pytest

import components_cases as CC
import components_ref as R
from oracle import foe_oracle as fo


def _scipy_tables(mask, connectivity, min_area, max_blobs):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    labels, n = ndi.label(np.asarray(mask) != 0, structure=structure)
    labels = labels.astype(np.int32)
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    yy, xx = np.mgrid[0:labels.shape[0], 0:labels.shape[1]]
    sx = np.bincount(labels.ravel(), weights=xx.ravel(), minlength=n + 1).astype(np.int64)
    sy = np.bincount(labels.ravel(), weights=yy.ravel(), minlength=n + 1).astype(np.int64)
    table = np.zeros(max_blobs, R.BLOB_DTYPE)
    n_blobs = 0
    for k, sl in enumerate(ndi.find_objects(labels), start=1):
        if areas[k] < min_area:
            continue
        if n_blobs < max_blobs:
            table[n_blobs] = (k, sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start, areas[k], sx[k], sy[k])
        n_blobs += 1
    return labels, (n, n_blobs), table


@pytest.mark.parametrize("cid", [c.id for c in CC.CASES])
def test_restatement_equals_scipy_on_every_case(cid):
    case = CC.BY_ID[cid]
    labels, counts, tables = case.expected
    for b, mask in enumerate(case.masks):
        sl, sc, st = _scipy_tables(mask, case.connectivity, case.min_area, case.max_blobs)
        assert np.array_equal(labels[b], sl), (cid, case.names[b])
        assert (int(counts[b]["n_components"]), int(counts[b]["n_blobs"])) == sc, (cid, case.names[b])
        assert tables[b].tobytes() == st.tobytes(), (cid, case.names[b])
        # the one-call form agrees with the cached two-step form
    one = R.components(case.masks[0], case.connectivity, case.min_area, case.max_blobs)
    assert np.array_equal(one[0], labels[0]) and one[2].tobytes() == tables[0].tobytes()


def test_hand_written_expectations():
    u = np.array([[1, 0, 1, 0, 1], [1, 0, 1, 0, 0], [1, 1, 1, 0, 1]], np.uint8)
    labels, counts, table = R.components(u, 4, 1, 4)
    assert labels.tolist() == [[1, 0, 1, 0, 2], [1, 0, 1, 0, 0], [1, 1, 1, 0, 3]] and counts == (3, 3)
    assert [tuple(int(v) for v in r) for r in table] == [(1, 0, 0, 3, 3, 7, 7, 8), (2, 4, 0, 1, 1, 1, 4, 0), (3, 4, 2, 1, 1, 1, 4, 2), (0,) * 8]
    # a diagonal pair: one component under 8-connectivity, two under 4; any non-zero byte is set
    d = np.array([[7, 0], [0, 128]], np.uint8)
    assert R.components(d, 8)[0].tolist() == [[1, 0], [0, 1]] and R.components(d, 4)[0].tolist() == [[1, 0], [0, 2]]
    # numbering follows the FIRST pixel: the component that starts further left in the same row comes first
    m = np.array([[0, 1, 0, 1], [1, 1, 0, 1]], np.uint8)
    assert R.components(m, 4)[0].tolist() == [[0, 1, 0, 2], [1, 1, 0, 2]]
    # a ring and the dot inside its hole stay distinct
    r = np.ones((5, 5), np.uint8); r[1:4, 1:4] = 0; r[2, 2] = 1
    assert R.components(r, 8)[1] == (2, 2) and R.components(r, 8)[0][2, 2] == 2
    # min_area filters, max_blobs truncates, the tail is zero; n_blobs still counts every component that passes
    labels, counts, table = R.components(u, 4, 1, 2)
    assert counts == (3, 3) and [int(t["label"]) for t in table] == [1, 2]
    labels, counts, table = R.components(u, 4, 2, 3)
    assert counts == (3, 1) and [int(t["label"]) for t in table] == [1, 0, 0] and table[1:].tobytes() == bytes(80)
    assert R.components(np.zeros((3, 4), np.uint8))[1] == (0, 0)
    for bad in ((6, 1, 1), (8, 0, 1), (8, 1, 0), (8, 1, 65536)):
        with pytest.raises(ValueError):
            R.components(u, *bad)


@pytest.mark.parametrize("cid", ["131x67-all-c4", "131x67-all-c8", "127x49-all-c8", "1x37-all-c4"])
def test_hull_of_all_blob_boxes_is_the_simple_bounding_box(cid):
    case = CC.BY_ID[cid]
    _, counts, tables = case.expected
    for b, mask in enumerate(case.masks):
        assert counts[b]["n_blobs"] <= case.max_blobs
        assert R.hull(tables[b]) == tuple(int(v) for v in fo.simple_bounding_box((mask != 0).astype(np.uint8))), (cid, case.names[b])

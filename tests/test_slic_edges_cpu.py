"""The CPU half of the SLIC edge cases (slic_cases.py): the oracle (oracle/tsar_oracle_slic.c) against the plain statement of each stage
— the centre update as a visited-set mask per superpixel (bit for bit in RGB space, within the derived bound in CIELAB and XYZ), the
association against float64 distances, connectivity against the pixel-by-pixel rule — and every known answer, on every case and at
every size class of the update's window.  The GPU test (test_gpu_slic_edges.py) holds the kernels to this oracle and to the same plain
statement on the same inputs: its oracle comparisons are worth what this file shows the oracle to be worth.

Measured on the oracle (profiles/slic_edges/README.md): the share of pixels the association check decides by the margin rule alone,
and the largest |got - mean| / bound of the float cases.  The tests assert the derived bound and the 1 % cap, not those figures."""
import numpy as np
import pytest

import oracle_lib as ol
import slic_cases as sc


def _lab(c, color_space):
    return ol.slic_convert(c["bgra"], color_space).reshape(c["h"], c["w"], 4)


def _pipeline(c, color_space=2):
    """(converted image, init centres, labels of the first association) by the oracle"""
    lab = _lab(c, color_space)
    init = ol.slic_init_centers(lab, c["mw"], c["mh"], c["S"])
    return lab, init, ol.slic_find_association(lab, init, c["mw"], c["mh"], c["S"], c["weight"])


def _label_sets(c, lab_labels):
    stray, empty = sc.stray_labels(c, lab_labels)
    return (("pipeline", lab_labels, []), ("random", sc.random_labels(c), []), ("stray", stray, empty))


def test_size_classes_counted_over_every_size():
    """the census the case table rests on: S = 4..256"""
    cls = {S: sc.size_class(S) for S in range(4, 257)}
    assert [S for S in cls if "clamped" in cls[S]] == [4, 5]
    assert [S for S in cls if "exact" in cls[S]] == [4, 5] + list(range(16, 257, 16))
    assert sum("truncated" in v for v in cls.values()) == 235
    ragged = [S for S in cls if "ragged" in cls[S]]
    assert len(ragged) == 103 and ragged[:7] == [11, 17, 22, 23, 27, 28, 33]
    assert [S for S in cls if "own_cell_cut" in cls[S]] == [9, 10]
    assert all(("exact" in v) != ("truncated" in v) for v in cls.values())
    v = sc.visited(11)
    assert v[32, :16].all() and not v[32, 16:32].any() and not v[:, 32].any()
    v = sc.visited(22)
    assert v[64:66, :32].all() and not v[64:66, 32:64].any() and not v[:, 64:].any()
    for tag in sc.TAGS:
        assert sc.size_class(sc.TABLE[tag][0]) == sc.EXPECTED_CLASS[tag], tag


@pytest.mark.parametrize("tag", sc.TAGS)
def test_case_reaches_what_it_is_for(tag):
    """independently of oracle and kernel: owned pixels the update must NOT count exist where the size class says so"""
    c = sc.case(tag)
    S, w, h = c["S"], c["w"], c["h"]
    assert (c["mw"], c["mh"]) == (w // S, h // S)
    _, _, labels = _pipeline(c)
    cls = sc.size_class(S)
    for name, lb, _ in _label_sets(c, labels)[:2]:
        right, ragged, own = sc.cut_census(lb, S)
        print(tag, name, "owned pixels cut: right columns %d, ragged row %d, own cell %d" % (right, ragged, own))
        if "truncated" in cls and c["mw"] > 1:
            assert right > 0, (tag, name)
        if "ragged" in cls:
            assert ragged > 0, (tag, name)
        if "own_cell_cut" in cls:
            assert own > 0, (tag, name)
        if "exact" in cls:
            assert (right, ragged, own) == (0, 0, 0)
    if tag.startswith("clamp"):
        assert w % S and h % S and 3 * S // 16 == 0
    if tag == "one-centre":
        assert c["mw"] == c["mh"] == 1 and w - S == S - 1 and h == S
    if tag == "one-row":
        assert c["mh"] == 1 and c["mw"] > 1
    if tag == "big":
        assert sc.grid_of(S) == (2304, 48) and c["mw"] == c["mh"] == 1


@pytest.mark.parametrize("tag", sc.EXACT_TAGS)
def test_oracle_update_equals_the_plain_statement_in_rgb(tag):
    c = sc.case(tag)
    lab, _, labels = _pipeline(c)
    for name, lb, empty in _label_sets(c, labels):
        got, want = sc.oracle_update(lab, lb, c["S"]), sc.plain_update(lab, lb, c["S"])
        assert sc.same_centres(got, want), (tag, name, np.nonzero(got["n"] != want["n"])[0][:5])
        assert sc.empty_records_ok(got) and all(got["n"][i] == 0 for i in empty), (tag, name)


@pytest.mark.parametrize("color_space", [0, 1])
@pytest.mark.parametrize("tag", sc.TAGS)
def test_oracle_update_within_the_derived_bound(tag, color_space):
    c = sc.case(tag)
    lab, _, labels = _pipeline(c, color_space)
    for name, lb, empty in _label_sets(c, labels):
        got = sc.oracle_update(lab, lb, c["S"])
        ok, ratio = sc.within_bound(got, lab, lb, c["S"])
        print(tag, name, "colour space %d: largest |got - mean| / bound %.4f" % (color_space, ratio))
        assert ok, (tag, name, ratio)
        assert sc.empty_records_ok(got) and all(got["n"][i] == 0 for i in empty), (tag, name)


def test_oracle_update_at_256_in_rgb_within_the_bound():
    c = sc.case("big")
    lab, _, labels = _pipeline(c)
    for name, lb, _ in _label_sets(c, labels):
        ok, ratio = sc.within_bound(sc.oracle_update(lab, lb, 256), lab, lb, 256)
        print("big", name, "RGB: largest |got - mean| / bound %.4f" % ratio)
        assert ok, (name, ratio)


@pytest.mark.parametrize("color_space", [0, 2])
@pytest.mark.parametrize("tag", sc.TAGS)
def test_oracle_association_passes_the_float64_check(tag, color_space):
    """from the init centres and from the centres after one update"""
    c = sc.case(tag)
    S, mw, mh, wt = c["S"], c["mw"], c["mh"], c["weight"]
    lab, init, l0 = _pipeline(c, color_space)
    after = sc.oracle_update(lab, l0, S)
    l1 = ol.slic_find_association(lab, after, mw, mh, S, wt, l0)
    for name, centres, lb in (("init", init, l0), ("one update", after, l1)):
        ok, share, detail = sc.plain_assoc_check(lab, centres, lb, mw, mh, S, wt)
        print(tag, name, "colour space %d: decided by the margin rule alone %.5f" % (color_space, share), detail)
        assert ok and share <= sc.MARGIN_SHARE_CAP, (tag, name, share, detail)
        assert lb.min() >= 0 and lb.max() < mw * mh


@pytest.mark.parametrize("tag", sc.TAGS)
def test_no_iterations_is_init_and_one_association(tag):
    c = sc.case(tag)
    for color_space in (0, 1, 2):
        _, _, l0 = _pipeline(c, color_space)
        assert np.array_equal(ol.slic(c["bgra"], c["S"], 0, c["weight"], 0, color_space), l0), (tag, color_space)


@pytest.mark.parametrize("key", list(sc.WEIGHT0))
def test_weight_zero_known_answer(key):
    c = sc.weight0_case(key)
    S, mw, mh = c["S"], c["mw"], c["mh"]
    for iters in (0, 1, 3):
        got, _, centres = ol.slic(c["bgra"], S, iters, 0.0, 0, 2, want_centers=True)
        assert np.array_equal(got, c["labels"]), (key, iters)
        if iters:
            empty = centres[:, 7] == 0
            assert int(empty.sum()) == c["n_empty"] and (centres[empty, :6] == 0).all(), (key, iters)
            assert np.array_equal(centres[:, 6], np.arange(mw * mh))
    lab, init, l0 = _pipeline(c)
    assert np.array_equal(l0, c["labels"])
    after = sc.oracle_update(lab, l0, S)
    assert sc.same_centres(after, sc.plain_update(lab, l0, S)) and sc.empty_records_ok(after)
    assert int((after["n"] == 0).sum()) == c["n_empty"]
    if key == (9, 3, 2, 0):
        assert (l0 == 1).any() and after["n"][1] == 0           # id 1 owns pixels and its update sees none of them
    own = after["n"] != 0
    assert (after["color"][own, :3] == np.array(sc.CONSTANT, np.float32)).all()
    l1 = ol.slic_find_association(lab, after, mw, mh, S, 0.0, l0)
    assert np.array_equal(l1, c["labels"])
    for centres, lb in ((init, l0), (after, l1)):               # empty centres (colour 0) among the candidates
        ok, _, detail = sc.plain_assoc_check(lab, centres, lb, mw, mh, S, 0.0)
        assert ok, (key, detail)


def test_tie_with_weight_known_answer():
    c = sc.tie_case()
    assert np.array_equal(ol.slic(c["bgra"], 4, 0, 5.0, 0, 2), c["labels"])
    lab, init, l0 = _pipeline(c)
    assert np.array_equal(init["center"], np.array([[2, 2], [6, 2], [10, 2]], np.float32))
    for x, a, b in ((4, 0, 1), (8, 1, 2)):
        for y in range(4):
            da, db = (ol.slic_distance(lab[y, x], x, y, init[k], 5.0, np.float32(1) / np.float32(4)) for k in (a, b))
            assert da == db and l0[y, x] == a, (x, y, da, db)
    assert sc.plain_assoc_check(lab, init, l0, 3, 1, 4, 5.0)[0]


def test_connectivity_known_answers():
    (at15, keep), (at16, take) = sc.threshold_images()
    out15, out16 = ol.slic_connectivity(at15), ol.slic_connectivity(at16)
    assert out15[4, 4] == keep == at15[4, 4] and out16[4, 4] == take != at16[4, 4]
    assert np.array_equal(out15, sc.plain_connectivity(at15)) and np.array_equal(out16, sc.plain_connectivity(at16))
    for lb in sc.all_border_images():
        out = ol.slic_connectivity(lb)
        assert np.array_equal(out, sc.plain_connectivity(lb))
        h, w = lb.shape
        if (h, w) == (5, 5):
            assert out[2, 2] == lb[4, 4] != lb[2, 2]
            out[2, 2] = lb[2, 2]
        assert np.array_equal(out, lb)


@pytest.mark.parametrize("tag", ["clamp4", "ragged-11", "one-row"])
def test_connectivity_on_pipeline_labels_is_the_plain_rule(tag):
    c = sc.case(tag)
    lb = ol.slic(c["bgra"], c["S"], 1, c["weight"], 0, 2)
    once = ol.slic_connectivity(lb)
    assert np.array_equal(once, sc.plain_connectivity(lb))
    assert np.array_equal(ol.slic(c["bgra"], c["S"], 1, c["weight"], 1, 2), sc.plain_connectivity(once))

"""The HIP SLIC kernels (slic_kernels.hip, through tsar_selftest_slic_stage and tsar_slic) on the inputs of slic_cases.py: every size
class of the centre update's window (bpl clamped at S = 4, 5; the superpixel's own cell cut at S = 9, 10; the ragged last block row at
S = 11, 17, 22, 27; right columns cut at S = 6, 21; exact at S = 16, 48), remainder stripes, centre maps of one row and of one centre,
S = 256 (2304 block rounds of the any_flag double buffer), empty superpixels entering the next association, first-wins ties,
no_iters == 0, the 15 / 16 threshold of the connectivity pass and images that are all border.

The centre update is held to the PLAIN STATEMENT of what it sums (slic_cases.plain_update: a visited-set mask per superpixel, no block
walk, no tree) bit for bit in RGB space, where every float32 partial sum is an exact integer whatever the order, and to the derived
bound (plain_update_bound) where sums round; and to the oracle bit for bit in all three colour spaces.  The association is held to
float64 distances (plain_assoc_check) and to the oracle label for label.  test_slic_edges_cpu.py holds the oracle to the same plain
statements on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import slic_cases as sc
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu

ITERS, CONNECT, SPACES = (0, 1, 3), (0, 1), (0, 1, 2)


@pytest.fixture(scope="module")
def m():
    mm = api.Matcher()
    yield mm
    mm.close()


_oracle = {}


def _ref(c, color_space):
    """the oracle's stages over a case: computed once, shared, left unchanged.  lab, init centres, labels of the first association,
    centres after one update, labels of the second association"""
    key = (c["tag"], color_space)
    if key not in _oracle:
        S, mw, mh, wt = c["S"], c["mw"], c["mh"], c["weight"]
        lab = ol.slic_convert(c["bgra"], color_space).reshape(c["h"], c["w"], 4)
        init = ol.slic_init_centers(lab, mw, mh, S)
        l0 = ol.slic_find_association(lab, init, mw, mh, S, wt)
        after = sc.oracle_update(lab, l0, S)
        l1 = ol.slic_find_association(lab, after, mw, mh, S, wt, l0)
        _oracle[key] = dict(lab=lab, init=init, l0=l0, after=after, l1=l1)
    return _oracle[key]


def _update(m, lab, labels, S):
    """slic_update_kernel into prefilled records: an empty superpixel's record must be written too"""
    h, w = labels.shape
    mw, mh = w // S, h // S
    return m._slic_stage(3, w, h, mw, mh, api.SlicSettings(S, 0, 5.0, 0, 0), np.ascontiguousarray(lab, np.float32),
                         np.ascontiguousarray(labels, np.int32), sc.prefilled_centres(mw * mh))


def _label_sets(c, labels):
    stray, empty = sc.stray_labels(c, labels)
    return (("pipeline", labels, []), ("random", sc.random_labels(c), []), ("stray", stray, empty))


@pytest.mark.parametrize("tag", sc.TAGS)
def test_centre_update_is_the_plain_statement(m, tag):
    c = sc.case(tag)
    S = c["S"]
    bad = []
    for color_space in SPACES:
        r = _ref(c, color_space)
        for name, lb, empty in _label_sets(c, r["l0"]):
            got = _update(m, r["lab"], lb, S)
            what = (tag, name, color_space)
            if not sc.same_centres(got, sc.oracle_update(r["lab"], lb, S)):
                bad.append(what + ("differs from the oracle",))
            if not (sc.empty_records_ok(got) and all(got["n"][i] == 0 for i in empty)):
                bad.append(what + ("an empty superpixel's record",))
            if color_space == 2 and tag in sc.EXACT_TAGS:
                want = sc.plain_update(r["lab"], lb, S)
                differing = (got["n"] != want["n"]) | (sc.bits(got["center"]) != sc.bits(want["center"])).any(1) | (sc.bits(got["color"]) != sc.bits(want["color"])).any(1)
                print(tag, name, "RGB: records differing from the plain statement %d of %d" % (int(differing.sum()), len(got)))
                if not sc.same_centres(got, want):
                    bad.append(what + ("differs from the plain statement",))
            else:
                ok, ratio = sc.within_bound(got, r["lab"], lb, S)
                print(tag, name, "colour space %d: largest |got - mean| / bound %.4f" % (color_space, ratio))
                if not ok:
                    bad.append(what + ("outside the derived bound", ratio))
    assert not bad, bad


@pytest.mark.parametrize("tag", sc.TAGS)
def test_association_is_the_float64_argmin(m, tag):
    """from the init centres and from the centres after one update: the oracle's labels, and the float64 check"""
    c = sc.case(tag)
    S, mw, mh, wt = c["S"], c["mw"], c["mh"], c["weight"]
    for color_space in (0, 2):
        r = _ref(c, color_space)
        assert sc.same_centres(m.slic_init_centers(r["lab"], mw, mh, S), r["init"]), (tag, color_space)
        l0 = m.slic_find_association(r["lab"], r["init"], mw, mh, S, wt)
        l1 = m.slic_find_association(r["lab"], r["after"], mw, mh, S, wt, l0)
        for name, centres, got, want in (("init", r["init"], l0, r["l0"]), ("one update", r["after"], l1, r["l1"])):
            ok, share, detail = sc.plain_assoc_check(r["lab"], centres, got, mw, mh, S, wt)
            print(tag, name, "colour space %d: labels differing from the oracle %d, decided by the margin rule alone %.5f"
                  % (color_space, int((got != want).sum()), share), detail)
            assert np.array_equal(got, want), (tag, name, color_space)
            assert ok and share <= sc.MARGIN_SHARE_CAP, (tag, name, color_space, share, detail)


@pytest.mark.parametrize("tag", sc.TAGS)
def test_tsar_slic_equals_the_oracle(m, tag):
    c = sc.case(tag)
    bad = []
    for color_space in SPACES:
        for iters in ITERS:
            for connect in CONNECT:
                got = m.slic(c["bgra"], api.SlicSettings(c["S"], iters, c["weight"], connect, color_space))
                want = ol.slic(c["bgra"], c["S"], iters, c["weight"], connect, color_space)
                if not (np.array_equal(got, want) and got.min() >= 0 and got.max() < c["mw"] * c["mh"]):
                    bad.append((tag, color_space, iters, connect, int((got != want).sum()), int(got.min()), int(got.max())))
    assert not bad, bad


@pytest.mark.parametrize("key", list(sc.WEIGHT0))
def test_weight_zero_known_answer(m, key):
    """a constant image, coh_weight 0: all candidates tie, the first in scan order wins, whatever the number of iterations — through
    updates that leave superpixels empty (at S = 9 one that owns pixels and sees none of them)"""
    c = sc.weight0_case(key)
    S, mw, mh = c["S"], c["mw"], c["mh"]
    for iters in ITERS:
        for connect in CONNECT:
            got = m.slic(c["bgra"], api.SlicSettings(S, iters, 0.0, connect, 2))
            assert np.array_equal(got, c["labels"] if not connect else sc.plain_connectivity(sc.plain_connectivity(c["labels"]))), (key, iters, connect)
            assert np.array_equal(got, ol.slic(c["bgra"], S, iters, 0.0, connect, 2)), (key, iters, connect)
    r = _ref(c, 2)
    l0 = m.slic_find_association(r["lab"], r["init"], mw, mh, S, 0.0)
    assert np.array_equal(l0, c["labels"])
    after = _update(m, r["lab"], l0, S)
    assert sc.same_centres(after, sc.plain_update(r["lab"], l0, S)) and sc.same_centres(after, r["after"])
    assert sc.empty_records_ok(after) and int((after["n"] == 0).sum()) == c["n_empty"]
    if key == (9, 3, 2, 0):
        assert (l0 == 1).any() and after["n"][1] == 0
    l1 = m.slic_find_association(r["lab"], after, mw, mh, S, 0.0, l0)
    assert np.array_equal(l1, c["labels"]) and np.array_equal(l1, r["l1"])
    for centres, lb in ((r["init"], l0), (after, l1)):          # empty centres (colour 0) among the candidates
        ok, _, detail = sc.plain_assoc_check(r["lab"], centres, lb, mw, mh, S, 0.0)
        assert ok, (key, detail)


def test_tie_with_weight_known_answer(m):
    c = sc.tie_case()
    assert np.array_equal(m.slic(c["bgra"], api.SlicSettings(4, 0, 5.0, 0, 2)), c["labels"])
    r = _ref(c, 2)
    assert np.array_equal(m.slic_find_association(r["lab"], r["init"], 3, 1, 4, 5.0), c["labels"])


def test_connectivity_known_answers(m):
    (at15, keep), (at16, take) = sc.threshold_images()
    out15, out16 = m.slic_connectivity(at15), m.slic_connectivity(at16)
    assert out15[4, 4] == keep and out16[4, 4] == take
    for lb, out in ((at15, out15), (at16, out16)):
        assert np.array_equal(out, sc.plain_connectivity(lb)) and np.array_equal(out, ol.slic_connectivity(lb))
    for lb in sc.all_border_images():
        out = m.slic_connectivity(lb)
        assert np.array_equal(out, ol.slic_connectivity(lb)) and np.array_equal(out, sc.plain_connectivity(lb))
        if lb.shape == (5, 5):
            assert out[2, 2] == lb[4, 4] != lb[2, 2]
            out[2, 2] = lb[2, 2]
        assert np.array_equal(out, lb)


@pytest.mark.parametrize("tag", ["big", "ragged-22"])
def test_two_runs_give_the_same_labels(m, tag):
    c = sc.case(tag)
    st = api.SlicSettings(c["S"], 3, c["weight"], 1, 0)
    assert np.array_equal(m.slic(c["bgra"], st), m.slic(c["bgra"], st))


def test_refusals_leave_the_context_usable(m):
    c = sc.case("clamp4")
    good = api.SlicSettings(4, 3, c["weight"], 1, 0)
    want = ol.slic(c["bgra"], 4, 3, c["weight"], 1, 0)
    assert np.array_equal(m.slic(c["bgra"], good), want)
    img = sc.noise_bgra(40, 40, 3)
    for what, bgra, st in (("S = 257", sc.noise_bgra(300, 300, 4), api.SlicSettings(257, 1, 5.0, 0, 0)),
                           ("w = S - 1", np.ascontiguousarray(img[:, :19]), api.SlicSettings(20, 1, 5.0, 0, 0)),
                           ("h = S - 1", np.ascontiguousarray(img[:19]), api.SlicSettings(20, 1, 5.0, 0, 0)),
                           ("no_iters = -1", img, api.SlicSettings(20, -1, 5.0, 0, 0)),
                           ("color_space = 3", img, api.SlicSettings(20, 1, 5.0, 0, 3))):
        with pytest.raises(api.TsarError) as e:
            m.slic(bgra, st)
        assert e.value.code == api.TSAR_ERR_INVALID, what
    out = np.zeros((40, 40), np.int32)
    st = api.SlicSettings(20, 1, 5.0, 0, 0)
    p_img, p_out = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for what, args in (("NULL image", (None, 40, 40, C.byref(st), p_out)), ("NULL settings", (p_img, 40, 40, None, p_out)),
                       ("NULL output", (p_img, 40, 40, C.byref(st), None))):
        assert m.L.tsar_slic(m._ctx, *args, api.MEM_HOST) == api.TSAR_ERR_INVALID, what
    assert not out.any()
    assert np.array_equal(m.slic(c["bgra"], good), want)

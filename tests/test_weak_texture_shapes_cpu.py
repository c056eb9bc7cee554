"""The weak-texture oracle (tsar_oracle_texture.c) against the plain statement of weak_texture_ref.py on shapes that are not axis-aligned
rectangles — oblique noise bands, two large components, a serpentine, a comb, a spiral — and on pairs of images one quarter-pixel apart
that sit on either side of the walk's and the classifier's thresholds.  Every output is an integer or a float that holds one: equality
throughout, no tolerance.

The conditions that make a case worth running (segments drawn off the axes, both walk majors, a negative rho, the closing separating
what the open detector joins, the exact threshold values) are asserted HERE, on the plain statement, so that the GPU test that reuses
the cases (test_gpu_weak_texture_shapes.py) cannot pass on images that exercise nothing.  The figures are what the plain statement and
the oracle give with the builders' seeds."""
import numpy as np
import pytest

import oracle_lib as ol
import weak_texture_ref as wr

OUTPUTS = ("labels", "labels4", "text", "size", "count", "edge")


def _weak(res):
    return int((res["text"] == -1).sum())


def _drawn(res):
    return [r for r in res["runs"] if r["drawn"]]


def test_hough_tables_equal_the_oracles_bit_for_bit():
    """float32(cos(double)), float32(sin(double)) from numpy and from the C library the oracle links: a difference would be a libm finding"""
    cs, sn = np.empty(180, np.float32), np.empty(180, np.float32)
    ol.lib().orc_hough_tables(ol._p(cs), ol._p(sn))
    pc, ps = wr.hough_tables()
    assert np.array_equal(cs.view(np.uint32), pc.view(np.uint32)) and np.array_equal(sn.view(np.uint32), ps.view(np.uint32))


@pytest.mark.parametrize("close", [True, False], ids=["closing", "open"])
@pytest.mark.parametrize("name", sorted(wr.CASES))
def test_oracle_equals_the_plain_statement(name, close):
    ref = ol.weak_texture(wr.image(name), connect="true", close_lines=close)
    pl = wr.plain(name, close)
    for k in OUTPUTS:
        assert np.array_equal(ref[k], pl[k]), k
    assert ref["text"].dtype == pl["text"].dtype == np.float32 and ref["size"].dtype == pl["size"].dtype
    assert ref["segments"] == pl["segments"]
    assert len(ref["text"]) == len(pl["text"]) == int(pl["labels4"].max()) + 1


def test_literal_bresenham_octants():
    """the drawing rule on its own, in all eight octants and on the axes: end points included, one pixel per step of the major axis,
    8-connected, never more than half a pixel off the ideal line"""
    for x1, y1 in ((9, 4), (4, 9), (-4, 9), (-9, 4), (-9, -4), (-4, -9), (4, -9), (9, -4), (7, 0), (0, -7), (5, 5), (0, 0)):
        px = wr.bresenham(0, 0, x1, y1)
        assert px[0] == (0, 0) and px[-1] == (x1, y1) and len(px) == max(abs(x1), abs(y1)) + 1
        for (ax, ay), (bx, by) in zip(px, px[1:]):
            assert max(abs(bx - ax), abs(by - ay)) == 1
        for x, y in px:                                   # never further than half a pixel from the ideal line, measured along the minor axis
            assert abs(x * y1 - y * x1) * 2 <= max(abs(x1), abs(y1))


# ---- oblique bands -------------------------------------------------------------------------------------------------------------------
BAND_SEGMENTS = {0: 6, 30: 6, 45: 5, 60: 6, 83: 6, 90: 6, 97: 6, 120: 6, 135: 6, 150: 6, 173: 6}
BAND_EDGE_PIXELS_ADDED = {0: 374, 30: 410, 45: 314, 60: 418, 83: 392, 90: 382, 97: 400, 120: 383, 135: 431, 150: 360, 173: 398}


@pytest.mark.parametrize("deg", wr.BAND_DEGREES)
def test_band_is_closed_by_an_oblique_line(deg):
    """902 x 1001: four segments on the frame of the flat area (205 and 230 quarter-pixels long) and one or two along the band, which
    bridge its 10-quarter-pixel gap: two weak regions with the closing, one without"""
    closed, opened = wr.plain("band%d" % deg, True), wr.plain("band%d" % deg, False)
    assert closed["segments"] == BAND_SEGMENTS[deg] >= 5
    added = int((closed["edge"] == 255).sum()) - int((opened["edge"] == 255).sum())
    assert added == BAND_EDGE_PIXELS_ADDED[deg] > 0
    assert (_weak(closed), _weak(opened)) == (2, 1)
    assert len(closed["count0"]) == 1 and 43000 < closed["count0"][0] < 45000
    if deg not in (0, 90):                                 # a drawn run along the band itself: neither horizontal nor vertical
        assert any(r["start"][0] != r["end"][0] and r["start"][1] != r["end"][1] and r["t"] not in (0, 90) for r in _drawn(closed))


def test_bands_cover_both_majors_both_length_clauses_and_negative_rho():
    drawn = [r for d in wr.BAND_DEGREES for r in _drawn(wr.plain("band%d" % d, True))]
    span = lambda r: (abs(r["end"][0] - r["start"][0]), abs(r["end"][1] - r["start"][1]))
    assert any(r["xmajor"] for r in drawn) and any(not r["xmajor"] for r in drawn)
    assert any(span(r)[1] >= 160 > span(r)[0] for r in drawn)
    assert any(span(r)[0] >= 160 > span(r)[1] for r in drawn)
    assert any(span(r)[0] >= 160 and span(r)[1] >= 160 for r in drawn)
    assert any(r["rho"] < 0 for r in drawn)                # bands above 90 degrees: the normal points to x < 0
    oblique = [r for r in drawn if r["t"] not in (0, 90)]
    assert any(r["xmajor"] for r in oblique) and any(not r["xmajor"] for r in oblique)
    assert any(r["max_gap"] >= 8 for r in oblique)         # the band's gap is bridged inside an oblique run
    # 0 degrees (a horizontal band, normal at 90 degrees) walks along x
    assert any(r["xmajor"] and r["t"] == 90 and 100 < r["start"][1] < 140 for r in _drawn(wr.plain("band0", True)))


def test_near_axis_band_draws_but_does_not_close():
    """7 degrees: the band's votes split over neighbouring cells and no peak along it reaches a run of 160; the frame is drawn, the
    two halves stay one region.  Kept because it fails to close."""
    closed, opened = wr.plain("band7", True), wr.plain("band7", False)
    assert closed["segments"] == 4 and all(r["t"] in (0, 90) for r in _drawn(closed))
    assert (_weak(closed), _weak(opened)) == (1, 1)


@pytest.mark.parametrize("name", ["short900x700_45", "short901x703_135"])
def test_band_shorter_than_the_minimum_length_is_left_open(name):
    """a flat area (700 - 80) / 4 = 155 quarter-pixels high: a steep band spans less than 160 in y and less than that in x; the two
    segments drawn lie on the frame's long horizontal sides"""
    closed = wr.plain(name, True)
    assert closed["segments"] == 2 and all(r["t"] == 90 and r["start"][1] == r["end"][1] for r in _drawn(closed))
    assert any(not r["drawn"] and r["t"] not in (0, 90) for r in closed["runs"])          # runs along the band were judged, and dropped
    assert (_weak(closed), _weak(wr.plain(name, False))) == (1, 1)


# ---- several large components, long chains -------------------------------------------------------------------------------------------
def test_two_bands_have_two_large_first_components():
    closed, opened = wr.plain("two_bands", True), wr.plain("two_bands", False)
    assert closed["count0"].tolist() == [28717, 28760]
    assert closed["segments"] == 8 and {r["component"] for r in _drawn(closed)} == {28717, 28760}
    assert (_weak(closed), _weak(opened)) == (4, 2)


@pytest.mark.parametrize("name,corridor,segments,piece", [("serpentine902", 17963, 39, 816), ("serpentine1203", 24455, 40, 1116)])
def test_serpentine_is_one_chain_until_the_closing_cuts_it(name, corridor, segments, piece):
    """19 corridors joined at alternate ends: one component; the closing draws the corridors' long sides through the joints and leaves
    single corridors.  Many parallel peaks, plateaus of equal votes."""
    closed, opened = wr.plain(name, True), wr.plain(name, False)
    assert closed["count0"].tolist() == [corridor] and int(opened["count"][1:].max()) == corridor
    assert closed["segments"] == segments and int(closed["count"][1:].max()) == piece
    assert (_weak(closed), _weak(opened)) == (0, 0)


@pytest.mark.parametrize("name,corridor,segments,piece", [("comb", 11937, 25, 772), ("spiral", 9048, 14, 817)])
def test_comb_and_spiral_are_one_component(name, corridor, segments, piece):
    """comb: 14 teeth that meet only in the spine along the bottom; spiral: 14 straight legs.  One component above 5000 without the closing"""
    closed, opened = wr.plain(name, True), wr.plain(name, False)
    assert closed["count0"].tolist() == [corridor] and int(opened["count"][1:].max()) == corridor > 5000
    assert closed["segments"] == segments and int(closed["count"][1:].max()) == piece


# ---- the walk's thresholds -----------------------------------------------------------------------------------------------------------
def test_gap_of_18_is_bridged_and_19_ends_the_run():
    """a vertical noise stripe with a flat hole of 72 resp. 76 pixels: along the stripe's left side (x = 69) the walk misses 18 resp. 19
    times in a row.  18: one run from frame to frame, drawn, the two halves separate; 19: two runs of about 90, dropped, one region."""
    a, b = (wr.plain(n, True) for n in wr.GAP_PAIR)
    ra = [r for r in wr.stripe_side_runs(a) if r["rho"] == 69]
    rb = [r for r in wr.stripe_side_runs(b) if r["rho"] == 69]
    assert len(ra) == 1 and ra[0]["max_gap"] == 18 and ra[0]["drawn"] and ra[0]["t"] == 0
    assert len(rb) == 2 and rb[0]["end_gap"] == 19 and not rb[0]["at_axis_end"] and not rb[0]["drawn"] and not rb[1]["drawn"]
    assert max(r["max_gap"] for r in rb) < 18
    assert (_weak(a), _weak(b)) == (2, 1)


def test_run_of_160_is_kept_and_159_dropped():
    """a stripe of 644 resp. 640 pixels, an island in the flat area: its side runs span 160 and 161 (drawn) resp. 157 and 159 (dropped)"""
    a, b = (wr.plain(n, True) for n in wr.LEN_PAIR)
    span = lambda r: max(abs(r["end"][0] - r["start"][0]), abs(r["end"][1] - r["start"][1]))
    ra, rb = wr.stripe_side_runs(a), wr.stripe_side_runs(b)
    assert any(span(r) == 160 and r["drawn"] for r in ra)
    assert max(span(r) for r in rb) == 159 and not any(r["drawn"] for r in rb)
    assert a["segments"] == b["segments"] + sum(r["drawn"] for r in ra)


def test_sawtooth_has_a_tie_between_neighbouring_rho_cells():
    """the right side of the flat area steps one quarter-pixel in and out so that at 0 degrees the cells rho = 138 and rho = 139 hold the
    same number of votes, at least 110: the peak rule (v > left, v >= right) keeps the left one, and its run from y = 10 to 225 is drawn
    through the flat pixels of the rows that are not stepped in.  With v > right neither cell would be a peak."""
    img = wr.image("sawtooth")
    edge = wr.roberts_edges(wr.pyr_down(wr.pyr_down(img)))
    lab, n = wr.components(edge)
    comp = lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
    near = np.zeros_like(comp)
    near[:, 1:] |= comp[:, :-1]; near[:, :-1] |= comp[:, 1:]; near[1:] |= comp[:-1]; near[:-1] |= comp[1:]
    votes = (near & ~comp).sum(axis=0)                      # at 0 degrees rho = x: the cell's votes are the column's boundary pixels
    assert votes[138] == votes[139] >= 110 and votes[137] < votes[138] > votes[140]
    closed = wr.plain("sawtooth", True)
    tie = [r for r in _drawn(closed) if r["t"] == 0 and r["rho"] in (138, 139)]
    assert len(tie) == 1 and tie[0]["rho"] == 138 and (tie[0]["start"], tie[0]["end"]) == ((138, 10), (138, 225))
    assert int((closed["edge"][:, 138] == 255).sum()) > int((wr.plain("sawtooth", False)["edge"][:, 138] == 255).sum()) + 50


# ---- the classifier's thresholds -----------------------------------------------------------------------------------------------------
def _largest(res):
    i = int(np.argmax(res["count"][1:])) + 1
    return i, int(res["count"][i]), int(res["xs"][i]), int(res["ys"][i])


@pytest.mark.parametrize("close", [True, False], ids=["closing", "open"])
def test_count_5000_is_not_weak_and_5001_is(close):
    """a rectangle with a protrusion, compact (69 * 79 < 2 * 5000): 5000 quarter-pixels with one 4 x 4 noise block in the protrusion, 5001
    without it.  The first value above the threshold is reached."""
    a, b = (wr.plain(n, close) for n in wr.COUNT_PAIR)
    (ia, ca, xa, ya), (ib, cb, xb, yb) = _largest(a), _largest(b)
    assert (ca, cb) == (5000, 5001) and xa * ya < 2 * ca and xb * yb < 2 * cb
    assert a["text"][ia] == 1 and a["size"][ia] == 0 and _weak(a) == 0
    assert b["text"][ib] == -1 and b["size"][ib] == max(xb, yb) == 79 and _weak(b) == 1


@pytest.mark.parametrize("close", [True, False], ids=["closing", "open"])
def test_box_clause_at_equality_and_one_below(close):
    """an L in a box of xs * ys = 134 * 133 = 17822: with 8911 pixels xs ys == 2 count (not weak), with 8912 (the protrusion one
    quarter-pixel taller) 17822 < 17824 (weak)"""
    a, b = (wr.plain(n, close) for n in wr.BOX_PAIR)
    (ia, ca, xa, ya), (ib, cb, xb, yb) = _largest(a), _largest(b)
    assert (xa, ya, ca) == (134, 133, 8911) and xa * ya == 2 * ca and a["text"][ia] == 1 and a["size"][ia] == 0
    assert (xb, yb, cb) == (134, 133, 8912) and xb * yb < 2 * cb and b["text"][ib] == -1 and b["size"][ib] == 134

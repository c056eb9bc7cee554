"""The CPU half of the weighted median filter's edge cases (wmf_cases.py): the oracle (orc_wmf_detect / orc_wmf_fill, built with
-DORC_NO_FMA) against the literal restatement of the reference's text (_wmf_pixel(..., literal=True) of
test_oracle_independent_sweep.py: gipuma_WMF gipuma.cu:1499-1698, gipuma_WMF_Final :1294-1497, the bubble sort that drags the zero
slot in), bit for bit, on every target / island pixel and on seeded random pixels per pass — and the conditions that make each case
reach what it is for.  The GPU test (test_gpu_wmf_edges.py) holds the kernel to this oracle on the same inputs: it is worth what the
oracle is worth on them."""
import ctypes as C

import numpy as np
import pytest

import wmf_cases as wc
from test_oracle_independent_sweep import _Cam, _depth_of_plane, _plane_offset, _wmf_pixel

f32 = np.float32
RANDOM_PIXELS = 40             # per pass
EXTRA_PIXELS = 12              # per pass, drawn from the pixels the pass is about (full windows; active pixels of a fill pass)


def _eq(a, b):
    return bool(wc.same_bits(a, b).all())


def _pixels_of_interest(c):
    px = [(t["x"], t["y"]) for t in c.get("targets", ())]
    for _, _, cx, cy in c.get("islands", ()):
        px += [(cx + i, cy + j) for j in range(wc.ISLAND) for i in range(wc.ISLAND)]
    return px


def _draw(rng, where, n):
    ys, xs = np.nonzero(where)
    pick = rng.choice(len(ys), size=min(n, len(ys)), replace=False) if len(ys) else []
    return [(int(xs[k]), int(ys[k])) for k in pick]


@pytest.mark.parametrize("name", wc.NAMES + wc.BELOW_THE_ABI)
def test_oracle_follows_the_text_at_the_edges(name):
    c = wc.case(name, nofma=True)
    h, w = c["mask"].shape
    rng = np.random.default_rng(77)
    textured = c["region_text"][c["labels"]] == 1
    checked = dict(detect=0, fill=0, filled=0)

    def hook(kind, it, before, orc, start):
        L = orc.L
        L.orc_expf.restype = C.c_float
        cam = _Cam(orc.camera(0))
        fb = cam.f * cam.baseline
        scale_in, depth_in, n_in = before["scale"], before["depth"], before["norm4"]
        pixels = _pixels_of_interest(c) + _draw(rng, np.ones((h, w), bool), RANDOM_PIXELS)
        with np.errstate(all="ignore"):
            if kind == "detect":
                radius, gap, ths = wc.detect_grid(it)
                pixels += _draw(rng, wc.tap_count(scale_in, radius, gap) == 121, EXTRA_PIXELS)
                for x, y in pixels:
                    num, nm = _wmf_pixel(orc, L, cam, scale_in, depth_in, n_in, x, y, radius, gap, 2 ** (3 - it), literal=True)
                    want = f32(0)
                    if num > 0 and nm is not None:
                        disp_now = fb / _depth_of_plane(cam, nm, x, y)
                        disp_org = fb / _depth_of_plane(cam, n_in[y, x], x, y)
                        want = f32(0) if abs(disp_now - disp_org) > f32(ths) else f32(1)
                    assert orc.scale[y, x] == want, (name, kind, it, x, y, num)
                    checked["detect"] += 1
                return
            radius, gap, ths = wc.fill_grid(it)
            active = textured & (scale_in == 0)
            pixels += _draw(rng, active, EXTRA_PIXELS)
            for x, y in pixels:
                same = _eq(orc.norm4[y, x], n_in[y, x]) and orc.scale[y, x] == scale_in[y, x] and _eq(orc.depth[y, x], depth_in[y, x])
                if not active[y, x]:
                    assert same, (name, start, it, x, y)
                    continue
                num, nm = _wmf_pixel(orc, L, cam, scale_in, depth_in, n_in, x, y, radius, gap, 2 ** it, literal=True)
                checked["fill"] += 1
                if num < ths or nm is None:
                    assert same, (name, start, it, x, y, num)
                    continue
                assert _eq(orc.norm4[y, x], nm), (name, start, it, x, y, num)
                disp = fb / _depth_of_plane(cam, nm, x, y)
                if disp <= f32(orc.min_disp) or disp >= f32(orc.max_disp):
                    assert orc.scale[y, x] == 0 and orc.depth[y, x] == f32(orc.min_disp), (name, start, it, x, y)
                else:
                    assert orc.scale[y, x] == 1 and orc.depth[y, x] == disp, (name, start, it, x, y)
                checked["filled"] += 1

    wc.run_oracle(c, nofma=True, hook=hook)                # (asserts the case's conditions)
    assert checked["detect"] >= 4 * min(RANDOM_PIXELS, w * h)
    if not name.startswith("tiny"):
        assert checked["fill"] > 0 and checked["filled"] > 0


@pytest.mark.parametrize("nofma", [False, True])
def test_plane_offset_keeps_the_sign_of_an_exact_zero(nofma):
    """getD_cu (gipuma.cu:71-86) returns -(n . X): through a point at depth +-0 (a median tap whose lines->depth is infinite) the
    offset is an exact zero whose SIGN decides whether the detection pass sees inf - inf or inf + inf.  The oracle's default build
    once negated inside a fused multiply-subtract, (-a b) - c, and returned +0 where the text — and the kernel — give -0."""
    c = wc.case("ties", nofma)
    orc = wc.oracle_of(c["scene"], nofma)
    cam = _Cam(orc.camera(0))
    rng = np.random.default_rng(8)
    for _ in range(50):
        n = rng.normal(size=3).astype(np.float32)
        x, y = int(rng.integers(0, 96)), int(rng.integers(0, 64))
        for depth in (0.0, -0.0):
            got, want = f32(orc.getD(n, x, y, depth)), _plane_offset(cam, n, x, y, f32(depth))
            assert got == 0 and want == 0 and np.signbit(got) == np.signbit(want), (n, x, y, depth)


def test_tap_count_counts_the_taps_of_the_text():
    """tap_count against the double loop of gipuma.cu:1538-1545 on a small mask, clamped windows included"""
    rng = np.random.default_rng(3)
    mask = (rng.random((9, 13)) < 0.6).astype(np.float32)
    for radius, gap in ((5, 1), (10, 2), (20, 4), (80, 16)):
        got = wc.tap_count(mask, radius, gap)
        for y in range(9):
            for x in range(13):
                want = sum(1 for i in range(-radius, radius + 1, gap) for j in range(-radius, radius + 1, gap)
                           if 0 <= x + i < 13 and 0 <= y + j < 9 and mask[y + j, x + i] == 1)
                assert got[y, x] == want, (radius, gap, x, y)

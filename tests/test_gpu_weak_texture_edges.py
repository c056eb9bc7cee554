"""tsar_detect_weak_texture at image sizes that are no multiple of four — where w / 2 and (w / 2) / 2 truncate, the odd pyramid levels
reflect at their borders and the label upsampling's `if (sx >= w4) sx--` clause has columns / rows to serve — at the smallest
accepted size, on a constant image, with an output capacity below the label count; and the live chain behind it (detect -> getview ->
region fit -> plane fill) against the oracle run on the oracle's own detection output."""
import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu


def _cameras(w, h):
    K = np.array([[900.0, 0, w / 2], [0, 900.0, h / 2], [0, 0, 1]], np.float32)
    return K[None], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)


SEED = 2024              # of the region fit's Philox draws: the library's default is 0, the oracle binding's 2024


def _matcher(img, flags=0):
    """a context holding the reference view alone (the refinement operators read no source image)"""
    h, w = img.shape
    K, R, t = _cameras(w, h)
    m = api.Matcher()
    m.set_params(api.default_params(depth_min=1.0, depth_max=10.0, flags=flags, seed=SEED))
    m.set_views([img.astype(np.float32)], K, R, t)
    return m


def _stripe_image(w, h):
    """uniform noise with two flat rectangles left and right of a vertical noise stripe, joined through a 40-pixel gap in it; the
    stripe is (h - 120) / 4 >= 160 quarter-resolution pixels long, so the Hough step has a boundary to close"""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    x0, x1 = w // 2 - 20, w // 2 + 20
    img[60:h - 60, 40:x0] = 120
    img[60:h - 60, x1:w - 40] = 120
    img[h // 2 - 20:h // 2 + 20, x0:x1] = 120
    return img


@pytest.mark.parametrize("w,h", [(611, 899), (609, 898), (610, 897)])
def test_detection_at_sizes_that_are_no_multiple_of_four(w, h):
    assert (h - 120) // 4 >= 160 and (w % 4 or h % 4)
    img = _stripe_image(w, h)
    weak = {}
    for flags, close in ((0, True), (api.FLAG_NO_LINE_CLOSING, False)):
        ref = ol.weak_texture(img, connect="true", close_lines=close)
        m = _matcher(img, flags)
        labels, text, size = m.detect_weak_texture()
        assert m.n_regions == len(ref["text"])
        assert np.array_equal(labels, ref["labels"])
        assert np.array_equal(text, ref["text"]) and np.array_equal(size, ref["size"])
        labels2, text2, size2 = m.detect_weak_texture()          # again: temporaries recycled from the scratch arena
        assert np.array_equal(labels, labels2) and np.array_equal(text, text2) and np.array_equal(size, size2)
        m.close()
        weak[close] = int((ref["text"] == -1).sum())
        if close:
            assert ref["segments"] > 0
        # the last columns / rows beyond 4 * (w / 4) exist and repeat their neighbours' labels
        w4, h4 = (w // 2) // 2, (h // 2) // 2
        assert 4 * w4 < w or 4 * h4 < h
        assert np.array_equal(labels[:, 4 * w4:], np.repeat(labels[:, 4 * w4 - 1:4 * w4], w - 4 * w4, axis=1))
        assert np.array_equal(labels[4 * h4:], np.repeat(labels[4 * h4 - 1:4 * h4], h - 4 * h4, axis=0))
    assert weak == {True: 2, False: 1}                          # the closing separates the two rectangles


@pytest.mark.parametrize("w,h", [(12, 12), (15, 13)])
def test_smallest_accepted_size(w, h):
    """quarter resolution 3 x 3, of which Roberts marks all but the centre: the constant 12 x 12 image ends as one flat label (the
    border fix clears the marks next to a flat pixel), the 15 x 13 noise image as edge pixels only; nothing weak"""
    img = np.random.default_rng(w).integers(0, 256, size=(h, w)).astype(np.uint8)
    img[:] = 77 if w == 12 else img
    ref = ol.weak_texture(img, connect="true", close_lines=True)
    m = _matcher(img)
    labels, text, size = m.detect_weak_texture()
    m.close()
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(text, ref["text"]) and np.array_equal(size, ref["size"])
    assert len(text) <= 2 and (text == 1).all() and labels.max() == len(text) - 1


def test_too_small_an_image_is_refused():
    img = np.zeros((12, 11), np.uint8)                           # 11 wide: quarter resolution 2 x 3
    m = _matcher(img)
    with pytest.raises(api.TsarError) as e:
        m.detect_weak_texture()
    assert e.value.code == api.TSAR_ERR_INVALID
    m.close()


def test_constant_image_is_one_weak_region():
    """1300 x 330, constant: the whole image is one flat component of 325 x 82 = 26 650 quarter-resolution pixels (more than
    weaktextnum = 5000; the border fix clears Roberts' border marks next to it) filling its bounding box, hence weak.
    (The `count > 100000` clause of the classification needs 100 001 quarter-resolution pixels: not reachable at this size.)"""
    img = np.full((330, 1300), 93, np.uint8)
    ref = ol.weak_texture(img, connect="true", close_lines=True)
    m = _matcher(img)
    labels, text, size = m.detect_weak_texture()
    m.close()
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(text, ref["text"]) and np.array_equal(size, ref["size"])
    assert (text == -1).sum() == 1 and (labels == int(np.nonzero(text == -1)[0][0])).mean() > 0.9


def _l_shaped_image(w=2402, h=1601):
    """noise with one flat L: a vertical band and a horizontal one along the left and bottom sides"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    img[20:h - 20, 20:700] = 120
    img[h - 380:h - 20, 20:w - 20] = 120
    return img


def test_sparse_region_above_100000_pixels_is_weak():
    """the classification's second clause (main.cpp:526): a region that fills less than half of its bounding box is weak all the
    same once it has more than 100 000 quarter-resolution pixels.  An L of about 102 000 such pixels in a box of 228 000, at a size
    that is no multiple of four either."""
    img = _l_shaped_image()
    ref = ol.weak_texture(img, connect="true", close_lines=True)
    big = int(np.argmax(ref["count"][1:])) + 1
    assert ref["count"][big] > 100000 and ref["text"][big] == -1
    ys, xs = np.nonzero(ref["labels4"] == big)
    assert (xs.max() - xs.min()) * (ys.max() - ys.min()) >= 2 * ref["count"][big]          # the first clause does not hold
    m = _matcher(img)
    labels, text, size = m.detect_weak_texture()
    m.close()
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(text, ref["text"]) and np.array_equal(size, ref["size"])


def test_capacity_below_the_label_count():
    img = _stripe_image(611, 899)
    ref = ol.weak_texture(img, connect="true", close_lines=True)
    n = len(ref["text"])
    assert n > 100
    m = _matcher(img)
    for cap in (1, n - 1, n, n + 5):
        labels, text, size = m.detect_weak_texture(cap=cap)
        assert m.n_regions == n                                   # reported in full
        k = min(cap, n)
        assert len(text) == k and np.array_equal(text, ref["text"][:k]) and np.array_equal(size, ref["size"][:k])
        assert np.array_equal(labels, ref["labels"])
    m.close()


def test_live_chain_behind_the_detection():
    """load_planes -> reliability mask -> detect -> getview -> ransac_regions -> fake_depth -> fill_textureless at 611 x 899, against
    the oracle fed with the ORACLE's detection output.  Flat pixels are reliable with probability 0.4: both weak regions keep more
    than 50 000 reliable pixels, the region fit's subsampling branch.  Depth and normals bit for bit."""
    w, h = 611, 899
    img = _stripe_image(w, h)
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (5.0 + 0.002 * xx + 0.001 * yy + rng.normal(0, 0.01, (h, w))).astype(np.float32)
    normal = np.array([0.1, -0.05, -1.0]) + rng.normal(0, 0.05, (h, w, 3))
    normal = np.ascontiguousarray(normal / np.linalg.norm(normal, axis=-1, keepdims=True), np.float32)
    flat = img == 120
    mask = np.where(flat, rng.uniform(size=(h, w)) < 0.4, rng.uniform(size=(h, w)) < 0.7).astype(np.float32)
    K, R, t = _cameras(w, h)
    det = ol.weak_texture(img, connect="true", close_lines=True)
    weak_ids = np.nonzero(det["text"] == -1)[0]
    assert len(weak_ids) == 2
    for rg in weak_ids:
        assert int(((det["labels"] == rg) & (mask == 1.0)).sum()) > 50000
    orc = ol.Oracle([img.astype(np.float32)], K, R, t, 1.0, 10.0, seed=SEED)
    orc.load_planes(depth, normal)
    orc.scale[:] = mask
    orc.set_regions(det["labels"], det["text"], det["size"])
    orc.getview()
    planes_ref, ratio_ref = orc.ransac_regions()
    orc.fake_depth()
    orc.update_scale()
    ref = orc.compute_disp()
    m = _matcher(img)
    m.load_planes(depth, normal)
    m.set_reliable_mask(mask)
    m.detect_weak_texture(want_labels=False)
    m.getview()
    planes, ratio = m.ransac_regions()
    assert np.array_equal(planes[weak_ids].view(np.uint32), planes_ref[weak_ids].view(np.uint32)) and np.array_equal(ratio, ratio_ref)
    m.fake_depth()
    m.fill_textureless()
    res = m.get_result(("depth", "normal"))
    m.close()
    assert np.array_equal(res["depth"].view(np.uint32), ref[..., 3].view(np.uint32))
    assert np.array_equal(res["normal"].view(np.uint32), ref[..., :3].view(np.uint32))
    assert not np.array_equal(res["depth"][flat], depth[flat])       # the fill did replace the flat areas' planes

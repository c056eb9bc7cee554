"""tsar_detect_weak_texture off the axes: the cases of weak_texture_ref.py — oblique noise bands (Hough votes and walks where cos and
sin both round, both walk majors, negative rho, Bresenham in the oblique octants), two large first-labelling components (the host loop
over the arrival-order list), a serpentine, a comb and a spiral (long union-find chains), and the pairs on either side of the gap 18 /
19, length 159 / 160, count 5000 / 5001 and xs ys = / < 2 count thresholds — against the oracle AND against the plain statement, with
and without the closing.  What makes each case worth running is asserted on the plain statement in test_weak_texture_shapes_cpu.py."""
import numpy as np
import pytest
import torch          # before the library is loaded, as the files that import synth do: torch's HIP runtime finds no device when it loads second

import oracle_lib as ol
import weak_texture_ref as wr
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu

MODES = ((0, True), (api.FLAG_NO_LINE_CLOSING, False))


def _matcher(img, flags=0, device=False):
    """a context holding the reference view alone, as test_gpu_weak_texture_edges.py builds it"""
    h, w = img.shape
    K = np.array([[900.0, 0, w / 2], [0, 900.0, h / 2], [0, 0, 1]], np.float32)
    view = img.astype(np.float32)
    if device:
        view = torch.from_numpy(view).cuda()
    m = api.Matcher()
    m.set_params(api.default_params(depth_min=1.0, depth_max=10.0, flags=flags, seed=2024))
    m.set_views([view], K[None], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32))
    return m


def _check(m, got, name, close):
    labels, text, size = got
    ref = ol.weak_texture(wr.image(name), connect="true", close_lines=close)
    pl = wr.plain(name, close)
    for want in (ref, pl):
        assert m.n_regions == len(want["text"])
        assert np.array_equal(labels, want["labels"])
        assert np.array_equal(text, want["text"]) and np.array_equal(size, want["size"])


@pytest.mark.parametrize("close", [True, False], ids=["closing", "open"])
@pytest.mark.parametrize("name", sorted(wr.CASES))
def test_detection_equals_oracle_and_plain_statement(name, close):
    flags = 0 if close else api.FLAG_NO_LINE_CLOSING
    m = _matcher(wr.image(name), flags)
    got = m.detect_weak_texture()
    m.close()
    _check(m, got, name, close)


@pytest.mark.parametrize("name", ["two_bands", "serpentine902", "serpentine1203"])
def test_repeated_call_and_device_view(name):
    """the same context twice (temporaries recycled from the arena; the large components' list arrives in another order), and once with the
    view handed over as a device tensor"""
    for flags, close in MODES:
        m = _matcher(wr.image(name), flags)
        first = m.detect_weak_texture()
        second = m.detect_weak_texture()
        _check(m, first, name, close)
        for a, b in zip(first, second):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        m.close()
    m = _matcher(wr.image(name), 0, device=True)
    got = m.detect_weak_texture()
    m.close()
    _check(m, got, name, True)

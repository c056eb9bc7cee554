"""Depth-map fusion stated a second time: numpy float64 from the prose of include/tsar.h and of oracle/tsar_oracle_fusion.c's header
(tests/fusion_ref.py), against the CPU oracle's orc_fuse — the function the GPU fuser is compared with bit for bit
(tests/test_gpu_parity.py, tests/test_gpu_fusion_edges.py) and whose loop the kernel shares line for line.  No GPU needed."""
import numpy as np
import pytest

import fusion_ref as fr
import oracle_lib as ol


@pytest.fixture(scope="module")
def inputs():
    return fr.make_inputs(173, 61)


def _orc(inp, used_list=0):
    def fuse_fn(depths, normals, grays, num_consistent):
        return ol.fuse(depths, normals, grays, inp["K"], inp["R"], inp["t"], inp["pairs"], num_consistent=num_consistent, used_list=used_list)
    return fuse_fn


def test_every_rejection_bites(inputs):
    """the inputs make each way of dropping a (pixel, source entry) pair matter: the image border, a hole in the source's depth map,
    the relative-depth test and the angle test each reject at least 1 % of the pairs of every view that has sources (measured at
    173 x 61: 9-15 % outside, 3-4 % no depth, 6-9 % depth test, 20-27 % angle test)"""
    seen = 0
    for i in range(inputs["n"]):
        rej = fr.restate_view(inputs, i)["rej"]
        if not inputs["pairs"][i]:
            assert rej["pairs"] == 0
            continue
        seen += 1
        for k in ("outside", "no_depth", "depth", "angle"):
            assert rej[k] >= 0.01 * rej["pairs"], (i, k, rej)
    assert seen == 3


@pytest.mark.parametrize("num_consistent", [1, 2, 3])
def test_orc_fuse_is_the_fusion_the_header_describes(inputs, num_consistent):
    """orc_fuse with used_list = 0 against the float64 restatement: the same (view, pixel) pairs kept, the same number of agreeing
    views, position / normal / gray within RECORD_TOL.  Pixels with a decision (nearest-pixel rounding, reprojection error, relative
    depth, cosine) within MARGIN_SCALE * MARGIN_UNIT of its threshold are left out.

    Measured here (fusion_ref.py has the figures next to the constants): without a margin orc_fuse and the restatement differ on 5
    of 40 083 candidate pixels at 173 x 61 and on 76 of 317 615 at 333 x 251, every one of them a nearest-pixel rounding within
    2.1e-5 px of a tie (0.0208 units of the margin triple 1e-3 px, 1e-5 relative depth, 1e-4 cosine); the margin is ten times that,
    0.21 units, and leaves out 0.23 % of the candidates — asserted below its cap of 3 %.  Agreeing records deviate by at most 1.75e-7
    (position, relative to the scene's coordinate scale), 1.4e-7 (normal), 4e-8 (gray / 255); the tolerance is four times the largest."""
    s = fr.compare(_orc(inputs), inputs, num_consistent, fr.MARGIN_SCALE, fr.RECORD_TOL)
    print("num_consistent %d: %d candidates, %.3f %% left out, %d kept pixels compared, needed margin %.4f units, deviations %.2e %.2e %.2e"
          % (num_consistent, s["candidates"], 100 * s["excluded_share"], s["compared_kept"], s["needed"], s["dpos"], s["dnrm"], s["dgray"]))
    assert s["excluded_share"] <= fr.EXCLUDED_CAP
    assert s["compared_kept"] > 0.1 * s["candidates"]            # the comparison is not vacuous: thousands of kept pixels


def test_first_view_does_not_depend_on_the_used_list(inputs):
    """marks made by a view gate the views after it: the first view's points are the same with and without them, the later views'
    are fewer with them"""
    a = _orc(inputs, 0)(inputs["depths"], inputs["normals"], inputs["grays"], 1)
    b = _orc(inputs, 1)(inputs["depths"], inputs["normals"], inputs["grays"], 1)
    assert np.array_equal(a[a[:, 8] == 0].view(np.uint32), b[b[:, 8] == 0].view(np.uint32))
    assert 0 < len(b) < len(a)

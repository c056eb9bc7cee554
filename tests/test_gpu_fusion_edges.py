"""tsar_fuse at the edges the parity test leaves out: pixel counts that are no multiple of the 256-thread workgroup (173 x 61 = 10 553,
333 x 251 = 83 583: a partial last workgroup), perturbed normals (the angle test rejects a fifth of the pairs), source lists that
are uneven, empty, hold the view itself or an entry twice, a view nobody lists, num_consistent 1 / 2 / 3, an output buffer smaller
than the cloud, and device-resident inputs.  Against the CPU oracle bit for bit, and against the float64 restatement of what fusion
computes (tests/fusion_ref.py; tests/test_fusion_cpu.py holds the oracle to the same restatement)."""
import numpy as np
import pytest

import fusion_ref as fr
import oracle_lib as ol
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu

_inputs = {}


@pytest.fixture(scope="module", params=[(173, 61), (333, 251)], ids=["173x61", "333x251"])
def inputs(request):
    if request.param not in _inputs:
        _inputs[request.param] = fr.make_inputs(*request.param)
    return _inputs[request.param]


def _gpu(inp, prm, **kw):
    return api.fuse(inp["depths"], inp["normals"], inp["grays"], inp["K"], inp["R"], inp["t"], inp["pairs"], prm, **kw)


@pytest.mark.parametrize("used_list", [0, 1])
def test_fusion_edges_bit_exact(inputs, used_list):
    inp = inputs
    assert (inp["w"] * inp["h"]) % 256 != 0
    m = api.Matcher()
    counts = []
    for num_consistent in (1, 2, 3):
        ref = ol.fuse(inp["depths"], inp["normals"], inp["grays"], inp["K"], inp["R"], inp["t"], inp["pairs"], num_consistent=num_consistent,
                      used_list=used_list)
        prm = api.FusionParams(num_consistent, 2.0, 0.01, 15.0, used_list)
        for kw in ({}, {"matcher": m}):
            got = _gpu(inp, prm, **kw)
            assert got.shape == ref.shape, (got.shape, ref.shape)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        assert not (ref[:, 8] == 2).any()                        # the view with the empty list keeps nothing
        assert (ref[:, 8] == 3).any()                            # the view nobody lists is fused like any other
        counts.append(len(ref))
    m.close()
    assert counts[0] > counts[1] > counts[2] > 0


def test_fusion_matches_the_float64_restatement(inputs):
    """the GPU's records, used_list = 0, held to tests/fusion_ref.py like orc_fuse is in tests/test_fusion_cpu.py: same kept
    (view, pixel) pairs, same counts, records within RECORD_TOL, outside the margin MARGIN_SCALE (whose derivation and measured
    figures stand next to those constants); the share left out stays under its cap"""
    inp = inputs
    m = api.Matcher()

    def fuse_fn(depths, normals, grays, num_consistent):
        return api.fuse(depths, normals, grays, inp["K"], inp["R"], inp["t"], inp["pairs"], api.FusionParams(num_consistent, 2.0, 0.01, 15.0, 0), matcher=m)
    for num_consistent in (1, 2, 3):
        s = fr.compare(fuse_fn, inp, num_consistent, fr.MARGIN_SCALE, fr.RECORD_TOL)
        print("%dx%d num_consistent %d: %d candidates, %.3f %% left out, %d kept pixels compared, needed margin %.4f units, deviations %.2e %.2e %.2e"
              % (inp["w"], inp["h"], num_consistent, s["candidates"], 100 * s["excluded_share"], s["compared_kept"], s["needed"], s["dpos"], s["dnrm"], s["dgray"]))
        assert s["excluded_share"] <= fr.EXCLUDED_CAP
        assert s["compared_kept"] > 0.1 * s["candidates"]
    m.close()


def test_first_view_ignores_the_used_list(inputs):
    inp = inputs
    a = _gpu(inp, api.FusionParams(1, 2.0, 0.01, 15.0, 0))
    b = _gpu(inp, api.FusionParams(1, 2.0, 0.01, 15.0, 1))
    assert np.array_equal(a[a[:, 8] == 0].view(np.uint32), b[b[:, 8] == 0].view(np.uint32))
    assert (a[:, 8] == 0).sum() > 1000 and 0 < len(b) < len(a)


def test_small_output_buffer_gets_the_prefix_and_the_full_count(inputs):
    inp = inputs
    prm = api.FusionParams(1, 2.0, 0.01, 15.0, 1)
    full, count = _gpu(inp, prm, return_count=True)
    assert count == len(full) > 2
    first_view = int((full[:, 8] == 0).sum())
    for cap in (1, first_view, count - 1):                       # inside the first view, at a view boundary, one short of everything
        part, n = _gpu(inp, prm, cap=cap, return_count=True)
        assert n == count
        assert part.shape == (cap, 9) and np.array_equal(part.view(np.uint32), full[:cap].view(np.uint32))


def test_device_tensors_in_device_tensor_out(inputs):
    """maps on the device: the cloud comes back as a tensor on that device (include/tsar.h: `mem` names where points_out lies too),
    with the bits of the host-array call; also through a context, and into a buffer smaller than the cloud"""
    import torch
    inp = inputs
    prm = api.FusionParams(2, 2.0, 0.01, 15.0, 1)
    ref = _gpu(inp, prm)
    dev = [[torch.from_numpy(a).cuda() for a in inp[k]] for k in ("depths", "normals", "grays")]
    m = api.Matcher()
    for kw in ({}, {"matcher": m}, {"cap": len(ref) - 1}):
        got, n = api.fuse(dev[0], dev[1], dev[2], inp["K"], inp["R"], inp["t"], inp["pairs"], prm, return_count=True, **kw)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
        assert n == len(ref)
        want = ref[: kw.get("cap", len(ref))]
        assert tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    m.close()

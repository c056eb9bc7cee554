"""Whole calls under the plane prior (include/tsar.h tsar_set_plane_prior) on the device against the CPU oracle's own statement of the
term (oracle/tsar_oracle.c prior_term, written from the header; tests/test_plane_prior_oracle_cpu.py), bit for bit.

tests/test_gpu_plane_prior.py compares the library with itself (its score without the prior plus the numpy restatement, one
propagation launch as the composition of its own scorer, memo on / off / packed).  An error shared by the rolled and the packed form
-- the prior read at the lane's own pixel where another lane's pixel is scored, a prior applied to an invalid hypothesis in the
redraw path -- passes all of that.  Here, modelled on tests/test_gpu_call_parity.py sections 3-4:
  1. pm_init + pm_iterate(6) in one call, the prior alone and with the ground-truth maps, strict and fast, over the box-11 loop (two and
     four best views) and the general-window loop, at 192 x 128 and at 101 x 67 (partial tiles in x and y: packed lanes without a pixel
     of their own score other lanes' pixels), at the four (TSAR_BLOCK, TSAR_COMPACT_FROM) launch shapes against one oracle run;
  2. one prior strong enough to decide (weight_depth 1, weight_normal 0.5, depth_clip 0.005);
  3. api.run_geom_pass with prior= and with build_prior= end to end (load_planes, the maps, the prior, rescore with its redraw, four
     iterations, compute_disp);
  4. tsar_upsample_merge and tsar_pm_merge_depths on a context with a prior against the host composition over the oracle's scorer.
The oracle takes the prior as the matcher holds it (get_plane_prior); that array is also held to hold_prior over the oracle's
load_planes (the conversion test_held_normals_are_load_planes_normals pins)."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_call_parity import SHAPES, _assert_same, _gt_maps, _knobs, _matcher, _oracle, _packed_expected, _state, _u8
from test_gpu_geom_multiscale import host_merge
from test_plane_prior_oracle_cpu import held_prior
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rcp_table():
    m = api.Matcher()
    t = ol.rcp_table_from_device(m)
    m.close()
    return t


_scenes = {}


def _scene(w, h):
    if (w, h) not in _scenes:
        _scenes[(w, h)] = synth.make_scene(w, h, 4, seed=71 + w, all_gt=True)
    return _scenes[(w, h)]


def _prior(sc, scale=1.01):
    """(depth, normal_world): ground truth scaled by 1.01, a 12 x 16 hole of depth 0 and one NaN normal"""
    depth = (sc.gt_depth.numpy().astype(np.float64) * scale).astype(F32)
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    h, w = depth.shape
    depth[h // 2:h // 2 + 12, w // 2:w // 2 + 16] = 0
    normal_world[5, 7] = np.nan
    return depth, normal_world


def _params(m):
    q = m.plane_prior_params
    return F32(q.weight_depth), F32(q.weight_normal), F32(q.depth_clip), F32(q.normal_clip)


def _install(orc, m, prior, held=None):
    """the matcher's held prior and settings into the oracle; the held array is hold_prior over the oracle's load_planes"""
    held = m.get_plane_prior() if held is None else held
    if prior is not None:
        want = held_prior(orc, *prior)
        assert np.array_equal(held.view(np.uint32), want.view(np.uint32))
    orc.set_plane_prior(held, _params(m))
    return held


def _prior_call(sc, imgs, maps, prior, box, n_best, strict, iters, **prior_kw):
    m = _matcher(sc, imgs, box, n_best, strict, 23)
    mats = None
    if maps is not None:
        m.set_geom_depths(maps, weight=0.2, clip=3.0)
        mats = [None] + [m.get_geom_matrices(v) for v in range(1, len(imgs))]
    m.set_plane_prior(*prior, **prior_kw)
    held, params = m.get_plane_prior(), _params(m)
    m.pm_init()
    m.pm_iterate(iters)                                               # one call: memo and packed form live
    got = m.get_plane()
    t = m.kernel_timing()
    m.close()
    return got, t, mats, held, params


def _oracle_call(sc, imgs, maps, mats, prior, held, params, box, n_best, strict, iters, table):
    orc = _oracle(sc, imgs, box, n_best, strict, 23, table)
    if maps is not None:
        orc.set_geom(maps, mats, weight=0.2, clip=3.0)
    assert np.array_equal(held.view(np.uint32), held_prior(orc, *prior).view(np.uint32))
    orc.set_plane_prior(held, params)
    orc.pm_init()
    orc.pm_iterate(iters)
    assert not orc.rcp_out_of_range
    return orc


# ---- 1. the main matrix ----------------------------------------------------------------------------------------------------------
_wanted = {}        # one oracle run per case, shared by the case's four launch shapes (the oracle knows neither knob)


@pytest.mark.parametrize("block,compact", SHAPES, ids=[f"block{b}-compact{c or 'default'}" for b, c in SHAPES])
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("size", [(192, 128), (101, 67)], ids=["192x128", "101x67"])
@pytest.mark.parametrize("box,n_best", [(11, 1), (11, 2), (11, 3), (19, 2)])
@pytest.mark.parametrize("with_maps", [False, True], ids=["prior", "prior+maps"])
def test_prior_call_forced_shapes(monkeypatch, rcp_table, mode, size, box, n_best, with_maps, block, compact):
    sc = _scene(*size)
    imgs = _u8(sc)
    strict = mode == "strict"
    maps = _gt_maps(sc) if with_maps else None
    prior = _prior(sc)
    iters = 6
    _knobs(monkeypatch, block, compact)
    got, t, mats, held, params = _prior_call(sc, imgs, maps, prior, box, n_best, strict, iters)
    key = (mode, size, box, n_best, with_maps)
    if key not in _wanted:
        _wanted[key] = _state(_oracle_call(sc, imgs, maps, mats, prior, held, params, box, n_best, strict, iters, rcp_table))
    want = _wanted[key]
    _assert_same(got, want, f"prior{' + maps' if with_maps else ''}, TSAR_BLOCK={block} TSAR_COMPACT_FROM={compact}")
    assert t["pm_sweep_geom"][0] == 2 * iters and "pm_sweep" not in t
    assert t["pm_sweep_packed"][0] == _packed_expected(2 * iters, compact)
    assert (want[2] >= 0).mean() > 0.5


# ---- 2. a decisive prior ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_prior_call_with_a_decisive_prior(monkeypatch, rcp_table, mode):
    """weight_depth 1, weight_normal 0.5, depth_clip 0.005: the term outweighs most photometric differences"""
    sc = _scene(101, 67)
    imgs = _u8(sc)
    strict = mode == "strict"
    prior = _prior(sc)
    kw = dict(weight_depth=1.0, weight_normal=0.5, depth_clip=0.005)
    _knobs(monkeypatch, "256", "2")
    got, t, mats, held, params = _prior_call(sc, imgs, None, prior, 11, 1, strict, 6, **kw)
    assert params[:3] == (F32(1.0), F32(0.5), F32(0.005))
    assert t["pm_sweep_geom"][0] == 12 and "pm_sweep" not in t and t["pm_sweep_packed"][0] == 10
    orc = _oracle_call(sc, imgs, None, None, prior, held, params, 11, 1, strict, 6, rcp_table)
    _assert_same(got, _state(orc), "decisive prior")
    weak = _oracle(sc, imgs, 11, 1, strict, 23, rcp_table)
    weak.set_plane_prior(held, (F32(0.1), F32(0.05), F32(0.02), params[3]))
    weak.pm_init()
    weak.pm_iterate(6)
    moved = (got[0].view(np.uint32) != weak.norm4.view(np.uint32)).any(-1).mean()
    assert moved > 0.05, moved                                       # (not the default prior's result)


# ---- 3. the geometric pass end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("how", ["prior", "build_prior"])
def test_geom_pass_with_a_prior_end_to_end(monkeypatch, rcp_table, mode, how):
    sc = _scene(192, 128)
    imgs = _u8(sc)
    strict = mode == "strict"
    maps = _gt_maps(sc)
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[40:60, 50:90] = 0                                          # no estimate: rescore draws pm_init's hypotheses there
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    prior = _prior(sc)
    _knobs(monkeypatch, "256", None)
    m = _matcher(sc, imgs, 11, 1, strict, 29)
    if how == "prior":
        api.run_geom_pass(m, depth, normal_world, maps, 4, prior=prior)
    else:
        api.run_geom_pass(m, depth, normal_world, maps, 4, build_prior={})
    got = m.get_result(("depth", "normal"))
    state = m.get_plane()
    mats = [None] + [m.get_geom_matrices(v) for v in range(1, len(imgs))]
    held = m.get_plane_prior()
    params = _params(m)
    t = m.kernel_timing()
    m.close()
    assert t["pm_rescore"][0] == (1 if how == "prior" else 2) and t["pm_sweep_geom"][0] == 8 and "pm_sweep" not in t
    assert t["pm_sweep_packed"][0] == 2
    assert (held[..., 3] > 0).mean() > 0.1                           # (a built prior that covers next to nothing would test nothing)
    orc = _oracle(sc, imgs, 11, 1, strict, 29, rcp_table)
    orc.load_planes(depth, normal_world)
    orc.set_geom(maps, mats, weight=0.2, clip=3.0)
    if how == "prior":
        assert np.array_equal(held.view(np.uint32), held_prior(orc, *prior).view(np.uint32))
    orc.set_plane_prior(held, params)
    orc.rescore()
    orc.pm_iterate(4)
    ref = orc.compute_disp()
    assert not orc.rcp_out_of_range
    _assert_same(state, _state(orc), f"run_geom_pass({how}) state")
    assert np.array_equal(got["depth"].view(np.uint32), np.ascontiguousarray(ref[..., 3]).view(np.uint32))
    assert np.array_equal(got["normal"].view(np.uint32), np.ascontiguousarray(ref[..., :3]).view(np.uint32))
    assert (got["depth"][40:60, 50:90] > 0).mean() > 0.5


# ---- 4. the merges on a context with a prior -------------------------------------------------------------------------------------
def _terms(m, maps, prior):
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.set_plane_prior(*prior)


def _oracle_from(sc, imgs, m, maps, prior, strict, table):
    """an oracle with the matcher's terms and the matcher's state"""
    orc = _oracle(sc, imgs, 11, 1, strict, 11, table)
    orc.set_geom(maps, [None] + [m.get_geom_matrices(v) for v in range(1, len(imgs))], weight=0.2, clip=3.0)
    _install(orc, m, prior)
    P, Cst, bv, rt = m.get_plane()
    orc.norm4[...], orc.c[...], orc.beview[...], orc.ratio[...] = P, Cst, bv, rt
    return orc


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_upsample_merge_under_a_prior_is_the_composition_over_the_oracle(rcp_table, mode):
    strict = mode == "strict"
    sc = _scene(101, 67)
    imgs = _u8(sc)
    maps, prior = _gt_maps(sc), _prior(sc)
    m = _matcher(sc, imgs, 11, 1, strict, 11)
    coarse = api.Matcher()
    coarse.pyramid_from(m)                                           # (refused once the fine context holds a term)
    coarse.pm_init()
    coarse.pm_iterate(2)
    coarse_planes = coarse.get_plane()[0]
    _terms(m, maps, prior)
    m.pm_init()
    m.pm_iterate(1)
    orc = _oracle_from(sc, imgs, m, maps, prior, strict, rcp_table)
    want = host_merge(orc, orc.norm4.copy(), coarse_planes)
    m.upsample_merge(coarse)
    got = m.get_plane()
    t = m.kernel_timing()
    m.close()
    coarse.close()
    assert not orc.rcp_out_of_range
    _assert_same(got, want, "upsample_merge under a prior")
    took = (np.ascontiguousarray(want[0]).view(np.uint32) != orc.norm4.view(np.uint32)).any(-1).mean()
    assert 0.02 < took < 0.98, took                                  # (both the own plane and a coarse one win somewhere)
    assert "pm_sweep" not in t


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_merge_depths_under_a_prior_is_the_composition_over_the_oracle(rcp_table, mode):
    strict = mode == "strict"
    sc = _scene(101, 67)
    imgs = _u8(sc)
    maps, prior = _gt_maps(sc), _prior(sc)
    h, w = sc.gt_depth.shape
    depth = (sc.gt_depth.numpy().astype(np.float64) * 1.002).astype(F32)
    ys, xs = np.mgrid[0:h, 0:w]
    pick = (xs * 7 + ys * 3) % 23
    for k, val in enumerate([0.0, np.nan, np.inf, F32(sc.depth_min) * F32(0.5), F32(sc.depth_max) * F32(2.0)]):
        depth[pick == k] = val
    m = _matcher(sc, imgs, 11, 1, strict, 11)
    _terms(m, maps, prior)
    m.pm_init()
    m.pm_iterate(1)
    orc = _oracle_from(sc, imgs, m, maps, prior, strict, rcp_table)
    # include/tsar.h tsar_pm_merge_depths from the oracle: rescore; Q = the own normal through the offered depth; strictly lower wins
    orc.rescore()
    P, Cst, bv, rt = _state(orc)
    with np.errstate(all="ignore"):
        usable = np.isfinite(depth) & (depth >= F32(sc.depth_min)) & (depth <= F32(sc.depth_max))
    assert 0.05 < (~usable).mean() < 0.6
    Q = P.copy()
    for y, x in zip(*np.nonzero(usable)):
        Q[y, x, 3] = orc.getD(P[y, x, :3], int(x), int(y), float(depth[y, x]))
    cq, bq, rq = orc.pm_cost_planes(Q)
    take = usable & (cq < Cst)
    want = (np.where(take[..., None], Q, P), np.where(take, cq, Cst), np.where(take, bq, bv), np.where(take, rq, rt))
    assert take.mean() > 0.1
    n_taken = m.merge_depths(depth)
    got = m.get_plane()
    t = m.kernel_timing()
    m.close()
    assert not orc.rcp_out_of_range
    _assert_same(got, want, "merge_depths under a prior")
    assert n_taken == int(take.sum())
    assert t["pm_merge_depths"][0] == 2 and t["pm_rescore"][0] == 1

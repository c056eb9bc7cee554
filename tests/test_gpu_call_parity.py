"""Whole tsar_pm_iterate calls on the device against the CPU oracle, bit for bit: the forms of the sweep that only a call of several
launches reaches.

Within one call the propagation memo is live from the second launch and the packed form (pm_sweep_impl.h SweepMemo / CMP) runs from
launch TSAR_COMPACT_FROM (default 6) on; the 256-thread workgroup shape is chosen by size from SWEEP_SMALL_IMAGE_TILES 256-thread tiles
on, or forced by TSAR_BLOCK.  tests/test_gpu_memo.py compares those forms with the library itself; here every case is one call
(pm_init + pm_iterate(n)) held to the oracle — planes, costs, best views and ratios as uint32 — in the strict arithmetic and in the
fast one (the oracle's S7 restatement with the device's v_rcp_f32 table), and kernel_timing() shows that the forms under test ran:
  1. the photometric sweep at both forced shapes, with and without the early packed form, over the box-11 loop (two and four best
     views) and the general-window loop (box 19; box 15 with five best views), at a size with whole tiles and one with partial tiles,
     and with a view subset;
  2. the bench's own shape and schedule: 2050 x 1590 (6500 tiles, the 256-thread shape by size), pm_iterate(8) with default knobs;
  3. the geometric-consistency term (tsar_set_geom_depths) over the same matrix, and one term strong enough to change decisions;
  4. api.run_geom_pass end to end (load_planes, the term, rescore, 4 iterations, compute_disp);
  5. the fine level of coarse-to-fine after tsar_upsample_planes, whose stored costs make the memo live from the first sweep.
The oracle does not depend on TSAR_BLOCK or TSAR_COMPACT_FROM: each oracle run is compared with several device runs.  Packed TRIP
counts are not asserted (same-colour memo.changed reads race within a launch; see pm_sweep_impl.h), only launch counts."""
import numpy as np
import pytest

import oracle_lib as ol
from test_pyramid_cpu import coarse_K, pyr_down
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = [("128", "2"), ("128", None), ("256", "2"), ("256", None)]     # (TSAR_BLOCK, TSAR_COMPACT_FROM); None = the default (6)


@pytest.fixture(scope="module")
def rcp_table():
    m = api.Matcher()
    t = ol.rcp_table_from_device(m)
    m.close()
    return t


def _knobs(monkeypatch, block, compact):
    """the knobs tsar_create reads: set before the matcher exists"""
    for name, val in (("TSAR_BLOCK", block), ("TSAR_COMPACT_FROM", compact)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _u8(sc):
    return [im.numpy().astype(np.uint8) for im in sc.images]


def _matcher(sc, imgs, box, n_best, strict, seed, subset=None):
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=box, box_vsize=box, n_best=n_best, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV if strict else 0, seed=seed))
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=isinstance(imgs[0], np.ndarray) and imgs[0].dtype == np.uint8)
    if subset is not None:
        m.set_view_subset(subset)
    m.enable_kernel_timing(True)
    return m


def _oracle(sc, imgs, box, n_best, strict, seed, table, subset=None, K=None):
    o = ol.Oracle([np.asarray(i, F32) for i in imgs], sc.K if K is None else K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=box,
                  n_best=n_best, seed=seed, subset=subset, flags=0 if strict else ol.FLAGS_FAST_8BIT_IMAGERY)
    if not strict:
        o.set_rcp_table(table)
    return o


def _state(orc):
    return orc.norm4.copy(), orc.c.copy(), orc.beview.copy(), orc.ratio.copy()


def _assert_same(got, want, what):
    for name, a, b in zip(("planes", "cost", "beview", "ratio"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape, (what, name)
        bad = a.view(np.uint32) != b.view(np.uint32)
        if bad.ndim == 3:
            bad = bad.any(-1)
        assert not bad.any(), f"{what}: {name} differs from the oracle at {int(bad.sum())} pixels, first {np.argwhere(bad)[:3].tolist()}"


def _packed_expected(launches, compact):
    return launches - (int(compact) if compact is not None else 6)


# ---- 1. photometric, forced shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("size", [(192, 128), (101, 67)])
@pytest.mark.parametrize("box,n_best,subset", [(11, 1, None), (11, 2, None), (11, 3, None), (19, 2, None), (11, 2, [1, 3])])
def test_photometric_call_forced_shapes(monkeypatch, rcp_table, mode, size, box, n_best, subset):
    """101 x 67: the last tiles are partial in x and y, so in the packed form lanes without a pixel of their own score other lanes'
    pairs.  box 11 / n_best 1 and 2: the box-11 two-best kernel; n_best 3: its four-best kernel; box 19: the general-window loop"""
    w, h = size
    strict = mode == "strict"
    sc = synth.make_scene(w, h, 4, seed=41 + w)
    iters = 6
    orc = _oracle(sc, sc.images, box, n_best, strict, 19, rcp_table, subset=subset)
    orc.pm_init()
    orc.pm_iterate(iters)
    want = _state(orc)
    assert not orc.rcp_out_of_range
    for block, compact in SHAPES:
        _knobs(monkeypatch, block, compact)
        m = api.matcher_from_scene(sc, box=box, n_best=n_best, seed=19, flags=api.FLAG_STRICT_DIV if strict else 0, subset=subset)
        m.enable_kernel_timing(True)
        m.pm_init()
        m.pm_iterate(iters)                                           # one call: memo and packed form live
        got = m.get_plane()
        t = m.kernel_timing()
        m.close()
        _assert_same(got, want, f"TSAR_BLOCK={block} TSAR_COMPACT_FROM={compact}")
        assert t["pm_sweep"][0] == 2 * iters
        assert t["pm_sweep_packed"][0] == _packed_expected(2 * iters, compact)
    assert (want[1] < 2.0).mean() > 0.5


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_photometric_call_general_window_many_best_views(monkeypatch, rcp_table, mode):
    """box 15 / n_best 5 over 6 sources: the general-window loop's 32-entry selection (NB = 32), rolled and packed"""
    strict = mode == "strict"
    sc = synth.make_scene(160, 96, 6, seed=43)
    orc = _oracle(sc, sc.images, 15, 5, strict, 19, rcp_table)
    orc.pm_init()
    orc.pm_iterate(4)
    want = _state(orc)
    assert not orc.rcp_out_of_range
    for compact in ("2", None):
        _knobs(monkeypatch, None, compact)
        m = api.matcher_from_scene(sc, box=15, n_best=5, seed=19, flags=api.FLAG_STRICT_DIV if strict else 0)
        m.enable_kernel_timing(True)
        m.pm_init()
        m.pm_iterate(4)
        got = m.get_plane()
        t = m.kernel_timing()
        m.close()
        _assert_same(got, want, f"box 15 / n_best 5, TSAR_COMPACT_FROM={compact}")
        assert t["pm_sweep_packed"][0] == _packed_expected(8, compact)


# ---- 2. photometric, the bench's shape and schedule ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_photometric_call_natural_256_thread_shape(rcp_table, mode):
    """2050 x 1590, 3 sources: 6500 tiles, so the 256-thread shape is chosen by size; the last tile column is 2 pixels wide and the last
    row 6 high.  pm_iterate(8) with default knobs is bench.py's launch schedule: 16 launches, the last 10 packed, the late ones with
    most arms dropped by the memo.  In fast mode the packed launches are bench.py's own kernel,
    pm_sweep_kernel<2, 5, false, true, 2228474, 256, true> (box-11 loop, buffer loads, difference texture)."""
    strict = mode == "strict"
    sc = synth.make_scene(2050, 1590, 3, seed=3)
    iters = 8
    m = api.matcher_from_scene(sc, seed=2024, flags=api.FLAG_STRICT_DIV if strict else 0)
    m.enable_kernel_timing(True)
    m.pm_init()
    m.pm_iterate(iters)
    got = m.get_plane()
    t = m.kernel_timing()
    m.close()
    assert t["pm_sweep"][0] == 2 * iters and t["pm_sweep_packed"][0] == 2 * iters - 6
    orc = _oracle(sc, sc.images, 11, 1, strict, 2024, rcp_table)
    orc.pm_init()
    orc.pm_iterate(iters)
    assert not orc.rcp_out_of_range
    _assert_same(got, _state(orc), "2050 x 1590, default knobs")


# ---- 3. the geometric-consistency term -------------------------------------------------------------------------------------------
def _gt_maps(sc):
    """every source view's ground-truth depth with a block of 0 (no estimate); the last view has no map"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
    maps[0] = None
    maps[-1] = None
    return maps


@pytest.fixture(scope="module")
def geom_scene():
    return synth.make_scene(192, 128, 4, seed=71, all_gt=True)


def _geom_call(sc, imgs, maps, box, n_best, strict, weight, clip, iters):
    m = _matcher(sc, imgs, box, n_best, strict, 23)
    m.set_geom_depths(maps, weight=weight, clip=clip)
    mats = [None] + [m.get_geom_matrices(v) for v in range(1, len(imgs))]
    m.pm_init()
    m.pm_iterate(iters)
    got = m.get_plane()
    t = m.kernel_timing()
    m.close()
    return got, t, mats


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("box,n_best", [(11, 1), (11, 2), (11, 3), (19, 2)])
def test_geometric_call_forced_shapes(monkeypatch, rcp_table, geom_scene, mode, box, n_best):
    sc = geom_scene
    imgs = _u8(sc)
    strict = mode == "strict"
    maps = _gt_maps(sc)
    iters = 6
    want = None
    for block, compact in SHAPES:
        _knobs(monkeypatch, block, compact)
        got, t, mats = _geom_call(sc, imgs, maps, box, n_best, strict, 0.2, 3.0, iters)
        if want is None:
            orc = _oracle(sc, imgs, box, n_best, strict, 23, rcp_table)
            orc.set_geom(maps, mats, weight=0.2, clip=3.0)
            orc.pm_init()
            orc.pm_iterate(iters)
            assert not orc.rcp_out_of_range
            want = _state(orc)
        _assert_same(got, want, f"geom, TSAR_BLOCK={block} TSAR_COMPACT_FROM={compact}")
        assert t["pm_sweep_geom"][0] == 2 * iters and "pm_sweep" not in t
        assert t["pm_sweep_packed"][0] == _packed_expected(2 * iters, compact)


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_geometric_call_with_a_decisive_term(monkeypatch, rcp_table, geom_scene, mode):
    """weight 1, clip 1: the term outweighs most photometric differences, so it changes which hypotheses win"""
    sc = geom_scene
    imgs = _u8(sc)
    strict = mode == "strict"
    maps = _gt_maps(sc)
    _knobs(monkeypatch, "256", "2")
    got, t, mats = _geom_call(sc, imgs, maps, 11, 1, strict, 1.0, 1.0, 6)
    assert t["pm_sweep_geom"][0] == 12 and t["pm_sweep_packed"][0] == 10
    orc = _oracle(sc, imgs, 11, 1, strict, 23, rcp_table)
    orc.pm_init()
    orc.pm_iterate(6)
    photometric = _state(orc)
    orc.set_geom(maps, mats, weight=1.0, clip=1.0)
    orc.pm_init()
    orc.pm_iterate(6)
    assert not orc.rcp_out_of_range
    _assert_same(got, _state(orc), "geom weight 1 clip 1")
    moved = (got[0].view(np.uint32) != photometric[0].view(np.uint32)).any(-1).mean()
    assert moved > 0.05, moved


# ---- 4. the geometric pass end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_geom_pass_end_to_end(monkeypatch, rcp_table, geom_scene, mode):
    sc = geom_scene
    imgs = _u8(sc)
    strict = mode == "strict"
    maps = _gt_maps(sc)
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[40:60, 50:90] = 0                                          # no estimate: rescore draws pm_init's hypotheses there
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    _knobs(monkeypatch, "256", None)
    m = _matcher(sc, imgs, 11, 1, strict, 29)
    api.run_geom_pass(m, depth, normal_world, maps, 4)
    got = m.get_result(("depth", "normal"))
    state = m.get_plane()
    mats = [None] + [m.get_geom_matrices(v) for v in range(1, len(imgs))]
    t = m.kernel_timing()
    m.close()
    assert t["pm_rescore"][0] == 1 and t["pm_sweep_geom"][0] == 8 and t["pm_sweep_packed"][0] == 2
    orc = _oracle(sc, imgs, 11, 1, strict, 29, rcp_table)
    orc.load_planes(depth, normal_world)
    orc.set_geom(maps, mats, weight=0.2, clip=3.0)
    orc.rescore()
    orc.pm_iterate(4)
    ref = orc.compute_disp()
    assert not orc.rcp_out_of_range
    _assert_same(state, _state(orc), "run_geom_pass state")
    assert np.array_equal(got["depth"].view(np.uint32), np.ascontiguousarray(ref[..., 3]).view(np.uint32))
    assert np.array_equal(got["normal"].view(np.uint32), np.ascontiguousarray(ref[..., :3]).view(np.uint32))
    assert (got["depth"][40:60, 50:90] > 0).mean() > 0.5


# ---- 5. the fine level of coarse-to-fine ------------------------------------------------------------------------------------------
def _host_upsample(orc_fine, coarse_planes, h, w):
    """the four candidates of every fine pixel scored by the oracle, argmin with the first winning ties (include/tsar.h
    tsar_upsample_planes)"""
    ch, cw = coarse_planes.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    best = None
    for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):            # (i, j) = (0,0), (1,0), (0,1), (1,1)
        cand = np.ascontiguousarray(coarse_planes[np.minimum(ys // 2 + j, ch - 1), np.minimum(xs // 2 + i, cw - 1)])
        c, bv, rt = orc_fine.pm_cost_planes(cand)
        if best is None:
            best = [cand, c, bv, rt]
            continue
        take = c < best[1]
        best[0] = np.where(take[..., None], cand, best[0])
        best[1] = np.where(take, c, best[1])
        best[2] = np.where(take, bv, best[2])
        best[3] = np.where(take, rt, best[3])
    return best


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_fine_level_after_upsampling(monkeypatch, rcp_table, mode):
    """tsar_upsample_planes leaves every stored cost its plane's score, so the memo is live from the first fine sweep and, with
    TSAR_COMPACT_FROM=2, the packed form from the third"""
    strict = mode == "strict"
    sc = synth.make_scene(128, 96, 3, seed=23, textureless=True)
    imgs = _u8(sc)
    _knobs(monkeypatch, "256", "2")
    fine = _matcher(sc, imgs, 11, 1, strict, 9)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    coarse.pm_init()
    coarse.pm_iterate(2)
    fine.upsample_planes(coarse)
    fine.pm_iterate(4)
    got = fine.get_plane()
    t = fine.kernel_timing()
    coarse_planes = coarse.get_plane()[0]
    fine.close()
    coarse.close()
    assert t["pm_sweep"][0] == 8 and t["pm_sweep_packed"][0] == 6
    oc = _oracle(sc, [pyr_down(i, True) for i in imgs], 11, 1, strict, 9, rcp_table, K=coarse_K(sc.K))
    oc.pm_init()
    oc.pm_iterate(2)
    assert np.array_equal(coarse_planes.view(np.uint32), oc.norm4.view(np.uint32))
    of = _oracle(sc, imgs, 11, 1, strict, 9, rcp_table)
    wp, wc, wbv, wrt = _host_upsample(of, oc.norm4.copy(), sc.h, sc.w)
    of.norm4[...] = wp
    of.c[...] = wc
    of.beview[...] = wbv
    of.ratio[...] = wrt
    of.set_launch(0)
    of.pm_iterate(4)
    assert not of.rcp_out_of_range and not oc.rcp_out_of_range
    _assert_same(got, _state(of), "fine level after upsampling")

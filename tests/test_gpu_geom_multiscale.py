"""The geometric-consistency pass coarse to fine (include/tsar.h tsar_geom_pyramid / tsar_pyramid_planes / tsar_upsample_merge,
api.run_geom_pass_multiscale, tsar_gipuma --geom_multi_scale) against the CPU oracle, bit for bit, in the strict arithmetic and in the
fast one (the oracle's restatement with the device's v_rcp_f32 table):
  - tsar_geom_pyramid: the coarse context's cost with the term equals the oracle's on the pyramid images, with the coarse K and the
    maps decimated in numpy by the statement's rule (holes at (2x, 2y) so that every fallback runs, odd sizes, a NULL map, two levels);
  - tsar_pyramid_planes: planes decimated bit for bit, then rescored as the oracle rescores them (invalid planes redrawn);
  - tsar_upsample_merge: a host composition from the oracle's pm_cost_planes (own plane first, then the four coarse candidates, argmin,
    the earlier candidate winning ties), with and without the term, box 11 and other windows, odd sizes, a view subset, a forced tie;
  - whole calls of run_geom_pass_multiscale at L = 1 and 2 against the same chain on the oracle; L = 0 is run_geom_pass;
  - the error paths; the CLI against the Python chain; what the coarse levels do on the textureless synthetic scene."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from test_pyramid_cpu import coarse_K, pyr_down
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rcp_table():
    m = api.Matcher()
    t = ol.rcp_table_from_device(m)
    m.close()
    return t


def _u8(sc):
    return [im.numpy().astype(np.uint8) for im in sc.images]


def _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=5, subset=None, box_v=None, K=None, R=None, t=None):
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=box, box_vsize=box if box_v is None else box_v, n_best=n_best, depth_min=sc.depth_min,
                                    depth_max=sc.depth_max, flags=api.FLAG_STRICT_DIV if strict else 0, seed=seed))
    m.set_views(imgs, sc.K if K is None else K, sc.R if R is None else R, sc.t if t is None else t, u8=True)
    if subset is not None:
        m.set_view_subset(subset)
    m.enable_kernel_timing(True)
    return m


def _levels(sc, imgs, n):
    """images and K of the fine level and n levels below it (tsar_pyramid_views: pyrDown of the 8-bit views, K halved)"""
    out = [(list(imgs), np.asarray(sc.K, F32))]
    for _ in range(n):
        im, K = out[-1]
        out.append(([pyr_down(i, True) for i in im], coarse_K(K)))
    return out


def _oracle(sc, imgs, K, box, n_best, strict, seed, table, subset=None, box_v=None):
    o = ol.Oracle([np.asarray(i, F32) for i in imgs], K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=box, n_best=n_best, seed=seed,
                  subset=subset, box_v=box_v, flags=0 if strict else ol.FLAGS_FAST_8BIT_IMAGERY)
    if not strict:
        o.set_rcp_table(table)
    return o


def geom_down(d):
    """include/tsar.h tsar_geom_pyramid: Dc[y][x] = Df[2y][2x] if > 0, else the first > 0 of (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1)
    inside the image, else 0"""
    h, w = d.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    p = np.zeros((2 * ch, 2 * cw), F32)
    p[:h, :w] = d
    out = np.zeros((ch, cw), F32)
    for c in (p[1::2, 1::2], p[1::2, 0::2], p[0::2, 1::2], p[0::2, 0::2]):     # the first in the order wins: written last
        out = np.where(c > 0, c, out)
    return out


def _maps(sc, null_view=None, seed=3):
    """ground-truth depth of every view with holes: a random third of the pixels and a block are 0, so that (2x, 2y) and its
    fallbacks are holes in every combination"""
    rng = np.random.default_rng(seed)
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][rng.random((h, w)) < 0.35] = 0
        maps[v][h // 3:h // 3 + 9, w // 4:w // 4 + 13] = 0
    if null_view is not None:
        maps[null_view] = None
    return maps


def _mats(m):
    return [None] + [m.get_geom_matrices(v) for v in range(1, m.n_views)]


def _state(orc):
    return orc.norm4.copy(), orc.c.copy(), orc.beview.copy(), orc.ratio.copy()


def _assert_same(got, want, what):
    for name, a, b in zip(("planes", "cost", "beview", "ratio"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape, (what, name)
        bad = a.view(np.uint32) != b.view(np.uint32)
        if bad.ndim == 3:
            bad = bad.any(-1)
        assert not bad.any(), f"{what}: {name} differs at {int(bad.sum())} pixels, first {np.argwhere(bad)[:3].tolist()}"


def host_merge(orc_fine, own, coarse_planes):
    """include/tsar.h tsar_upsample_merge composed from the oracle: the pixel's own plane, then the coarse planes at
    (x / 2 + i, y / 2 + j), clamped, (i, j) = (0,0), (1,0), (0,1), (1,1); argmin, the earlier candidate winning ties"""
    h, w = own.shape[:2]
    ch, cw = coarse_planes.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    cands = [np.ascontiguousarray(own)]
    for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cands.append(np.ascontiguousarray(coarse_planes[np.minimum(ys // 2 + j, ch - 1), np.minimum(xs // 2 + i, cw - 1)]))
    best = None
    for cand in cands:
        c, bv, rt = orc_fine.pm_cost_planes(cand)
        if best is None:
            best = [cand.copy(), c, bv, rt]
            continue
        take = c < best[1]
        best[0] = np.where(take[..., None], cand, best[0])
        best[1] = np.where(take, c, best[1])
        best[2] = np.where(take, bv, best[2])
        best[3] = np.where(take, rt, best[3])
    return best


def _merge_into(orc, coarse_planes):
    p, c, bv, rt = host_merge(orc, orc.norm4.copy(), coarse_planes)
    orc.norm4[...] = p
    orc.c[...] = c
    orc.beview[...] = bv
    orc.ratio[...] = rt
    orc.set_launch(0)


# ---- tsar_geom_pyramid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_geom_pyramid_is_the_decimated_term(rcp_table, mode):
    strict = mode == "strict"
    sc = synth.make_scene(101, 75, 4, seed=81, all_gt=True)           # 101 x 75 -> 51 x 38 -> 26 x 19: odd at every level
    imgs = _u8(sc)
    maps = _maps(sc, null_view=2)
    fine = _matcher(sc, imgs, strict=strict, seed=7)
    chain = [fine, api.Matcher(), api.Matcher()]
    for finer, coarser in zip(chain[:-1], chain[1:]):
        coarser.pyramid_from(finer)
    fine.set_geom_depths(maps, weight=0.5, clip=2.0)
    for finer, coarser in zip(chain[:-1], chain[1:]):
        coarser.geom_pyramid_from(finer)
    lv = _levels(sc, imgs, 2)
    want_maps = maps
    gt = synth.gt_planes(sc).numpy()
    branches = np.zeros(4, np.int64)
    for k in (1, 2):
        prev = want_maps
        want_maps = [None if d is None else geom_down(d) for d in want_maps]
        d = prev[1]                                                   # every branch of the rule ran
        h, w = d.shape
        p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), F32)
        p[:h, :w] = d
        c0, c1, c2 = p[0::2, 0::2] > 0, p[0::2, 1::2] > 0, p[1::2, 0::2] > 0
        branches += [c0.sum(), (~c0 & c1).sum(), (~c0 & ~c1 & c2).sum(), (~c0 & ~c1 & ~c2).sum()]
        m = chain[k]
        orc = _oracle(sc, lv[k][0], lv[k][1], 11, 1, strict, 7, rcp_table)
        orc.set_geom(want_maps, _mats(m), weight=0.5, clip=2.0)
        m.pm_init()
        random = m.get_plane()[0]
        decimated = np.ascontiguousarray(gt[::2 ** k, ::2 ** k])
        for planes in (random, decimated):
            got = m.pm_cost_planes(planes)
            want = orc.pm_cost_planes(planes)
            _assert_same(got, want, f"level {k}")
        assert not orc.rcp_out_of_range
        orc.clear_geom()                                              # the term is not a no-op at this level
        assert (orc.pm_cost_planes(decimated)[0] != got[0]).mean() > 0.2
    assert (branches > 0).all(), branches
    for m in chain:
        m.close()


# ---- tsar_pyramid_planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_pyramid_planes_decimate_and_rescore(rcp_table, mode):
    strict = mode == "strict"
    sc = synth.make_scene(99, 67, 4, seed=82, all_gt=True)
    imgs = _u8(sc)
    maps = _maps(sc)
    fine = _matcher(sc, imgs, strict=strict, seed=11)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[20:34, 30:52] = 0                                           # invalid planes: redrawn at the coarse level
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    fine.load_planes(depth, normal_world)
    fine.set_geom_depths(maps)
    coarse.geom_pyramid_from(fine)
    coarse.pyramid_planes_from(fine)
    got = coarse.get_plane()
    fp = fine.get_plane()[0]
    dec = np.ascontiguousarray(fp[::2, ::2])
    lv = _levels(sc, imgs, 1)
    orc = _oracle(sc, lv[1][0], lv[1][1], 11, 1, strict, 11, rcp_table)
    orc.set_geom([None if d is None else geom_down(d) for d in maps], _mats(coarse))
    orc.norm4[...] = dec
    orc.rescore()
    assert not orc.rcp_out_of_range
    _assert_same(got, _state(orc), "pyramid_planes")
    kept = (got[0].view(np.uint32) == dec.view(np.uint32)).all(-1)
    redrawn = ~kept
    assert kept.mean() > 0.8 and redrawn[10:17, 15:26].all()
    fine.close()
    coarse.close()


def test_pyramid_planes_timing_and_counter():
    sc = synth.make_scene(96, 64, 3, seed=83, all_gt=True)
    imgs = _u8(sc)
    fine = _matcher(sc, imgs, strict=True, seed=3)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    coarse.enable_kernel_timing(True)
    fine.pm_init()
    coarse.pyramid_planes_from(fine)                                   # also without any term
    t = coarse.kernel_timing()
    assert t["pm_pyramid_planes"][0] == 1 and t["pm_rescore"][0] == 1
    fine.close()
    coarse.close()


# ---- tsar_upsample_merge ----------------------------------------------------------------------------------------------------------
MERGE_CASES = [  # (size, box, box_v, n_best, subset)
    ((101, 67), 11, None, 1, None),
    ((101, 67), 15, None, 2, None),
    ((96, 70), 11, 7, 1, None),
    ((101, 67), 11, None, 2, [1, 3]),
]


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("term", [False, True])
@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
def test_upsample_merge_is_the_host_composition(rcp_table, mode, term, case):
    (w, h), box, box_v, n_best, subset = MERGE_CASES[case]
    strict = mode == "strict"
    sc = synth.make_scene(w, h, 4, seed=84 + case, all_gt=True)
    imgs = _u8(sc)
    maps = _maps(sc, null_view=3 if case == 1 else None)
    fine = _matcher(sc, imgs, box, n_best, strict, 13, subset=subset, box_v=box_v)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    if term:
        fine.set_geom_depths(maps)
        coarse.geom_pyramid_from(fine)
    coarse.pm_init()
    coarse.pm_iterate(2)
    fine.pm_init()
    fine.pm_iterate(1)
    own = fine.get_plane()[0]
    coarse_planes = coarse.get_plane()[0]
    fine.upsample_merge(coarse)
    got = fine.get_plane()
    t = fine.kernel_timing()
    fine.close()
    coarse.close()
    assert t["pm_upsample_merge"][0] == 1 and "pm_upsample" not in t
    orc = _oracle(sc, imgs, sc.K, box, n_best, strict, 13, rcp_table, subset=subset, box_v=box_v)
    if term:
        orc.set_geom(maps, _mats_of(sc, imgs, box, n_best, strict, subset, box_v, maps))
    want = host_merge(orc, own, coarse_planes)
    assert not orc.rcp_out_of_range
    _assert_same(got, want, f"merge term={term}")
    kept = (got[0].view(np.uint32) == own.view(np.uint32)).all(-1)
    assert kept.any() and not kept.all()                              # both kinds of winner occur


def _mats_of(sc, imgs, box, n_best, strict, subset, box_v, maps):
    m = _matcher(sc, imgs, box, n_best, strict, 13, subset=subset, box_v=box_v)
    mats = _mats(m)
    m.close()
    return mats


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_upsample_merge_own_plane_wins_ties(rcp_table, mode):
    """own planes n = (+0, 0, -1, d) and coarse planes n = (-0, 0, -1, d): the same plane, so every candidate scores the same, and
    the sign bit shows which one was kept"""
    strict = mode == "strict"
    sc = synth.make_scene(101, 67, 3, seed=88, all_gt=True)
    imgs = _u8(sc)
    fine = _matcher(sc, imgs, strict=strict, seed=17)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    d = F32(0.5) * (F32(sc.depth_min) + F32(sc.depth_max))
    own = np.zeros((sc.h, sc.w, 4), F32)
    own[..., 2] = -1.0
    own[..., 3] = d
    cp = np.zeros((coarse.h, coarse.w, 4), F32)
    cp[..., 0] = -0.0
    cp[..., 2] = -1.0
    cp[..., 3] = d
    fine.set_plane(own, np.zeros((sc.h, sc.w), F32))
    coarse.set_plane(cp, np.zeros((coarse.h, coarse.w), F32))
    fine.upsample_merge(coarse)
    got = fine.get_plane()
    orc = _oracle(sc, imgs, sc.K, 11, 1, strict, 17, rcp_table)
    c_own = orc.pm_cost_planes(own)[0]
    c_cand = orc.pm_cost_planes(np.ascontiguousarray(cp[np.minimum(np.arange(sc.h) // 2, coarse.h - 1)][:, np.minimum(np.arange(sc.w) // 2, coarse.w - 1)]))[0]
    assert np.array_equal(c_own.view(np.uint32), c_cand.view(np.uint32))            # a tie at every pixel
    _assert_same(got, host_merge(orc, own, cp), "tie")
    assert not np.signbit(got[0][..., 0]).any()                                    # the own plane won every tie
    fine.close()
    coarse.close()


# ---- whole calls ------------------------------------------------------------------------------------------------------------------
def _own_result(sc, holes=True):
    """a perturbed ground truth as the view's phase-1 result; holes: a block without estimate (depth 0).  The fine level scores its own
    plane there unrescored (tsar_upsample_merge), a plane through the camera centre whose fast-mode reciprocals leave the oracle's
    v_rcp_f32 table, so the fast-mode comparisons run without holes (the coarse levels' redraws are covered by the pyramid_planes test)"""
    depth = sc.gt_depth.numpy().astype(F32).copy()
    rng = np.random.default_rng(5)
    depth *= (1.0 + 0.03 * rng.standard_normal(depth.shape)).astype(F32)
    if holes:
        depth[30:50, 40:80] = 0
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    return depth, normal_world


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("levels", [1, 2])
def test_run_geom_pass_multiscale_is_the_oracle_chain(rcp_table, mode, levels):
    strict = mode == "strict"
    sc = synth.make_scene(160, 120, 4, seed=89, all_gt=True)
    imgs = _u8(sc)
    maps = _maps(sc)
    depth, normal_world = _own_result(sc, holes=strict)
    coarse_iters, fine_iters = 3, 2
    m = _matcher(sc, imgs, strict=strict, seed=29)
    coarse = [api.Matcher() for _ in range(levels)]
    for c in coarse:
        c.enable_kernel_timing(True)
    back = api.run_geom_pass_multiscale(m, depth, normal_world, maps, levels, coarse_iters, fine_iters, coarse=coarse)
    assert back == coarse
    got = m.get_plane()
    res = m.get_result(("depth", "normal"))
    chain = [m] + coarse
    mats = [_mats(c) for c in chain]
    timing = [c.kernel_timing() for c in chain]
    coarse_state = [c.get_plane() for c in coarse]
    for c in chain:
        c.close()
    for k, t in enumerate(timing):
        assert t.get("pm_upsample_merge", (0,))[0] == (1 if k < levels else 0), (k, t)
        assert t["pm_sweep_geom"][0] == 2 * (coarse_iters if k == levels else fine_iters), (k, t)
        assert "pm_sweep" not in t
        if k:
            assert t["geom_pyramid"][0] == len(imgs) - 1 and t["pm_pyramid_planes"][0] == 1 and t["pm_rescore"][0] == 1
    lv = _levels(sc, imgs, levels)
    orcs = [_oracle(sc, lv[k][0], lv[k][1], 11, 1, strict, 29, rcp_table) for k in range(levels + 1)]
    lmaps = maps
    orcs[0].load_planes(depth, normal_world)
    orcs[0].set_geom(lmaps, mats[0])
    for k in range(1, levels + 1):
        lmaps = [None if d is None else geom_down(d) for d in lmaps]
        orcs[k].set_geom(lmaps, mats[k])
        orcs[k].norm4[...] = np.ascontiguousarray(orcs[k - 1].norm4[::2, ::2])
        orcs[k].rescore()
    orcs[levels].pm_iterate(coarse_iters)
    for k in range(levels - 1, -1, -1):
        _merge_into(orcs[k], orcs[k + 1].norm4.copy())
        orcs[k].pm_iterate(fine_iters)
    ref = orcs[0].compute_disp()
    assert not any(o.rcp_out_of_range for o in orcs)
    for k in range(1, levels + 1):
        _assert_same(coarse_state[k - 1], _state(orcs[k]), f"level {k}")
    _assert_same(got, _state(orcs[0]), "fine level")
    assert np.array_equal(res["depth"].view(np.uint32), np.ascontiguousarray(ref[..., 3]).view(np.uint32))
    assert np.array_equal(res["normal"].view(np.uint32), np.ascontiguousarray(ref[..., :3]).view(np.uint32))


def test_level_zero_is_run_geom_pass():
    sc = synth.make_scene(128, 96, 4, seed=90, all_gt=True)
    imgs = _u8(sc)
    maps = _maps(sc)
    depth, normal_world = _own_result(sc)
    out = []
    for ms in (False, True):
        m = _matcher(sc, imgs, strict=False, seed=31)
        if ms:
            assert api.run_geom_pass_multiscale(m, depth, normal_world, maps, 0, 5, 3) == []
        else:
            api.run_geom_pass(m, depth, normal_world, maps, 3)
        out.append((m.get_plane(), m.get_result(("depth", "normal")), m.kernel_timing()))
        m.close()
    _assert_same(out[1][0], out[0][0], "L = 0")
    for k in ("depth", "normal"):
        assert np.array_equal(out[1][1][k].view(np.uint32), out[0][1][k].view(np.uint32))
    assert {k: v[0] for k, v in out[1][2].items()} == {k: v[0] for k, v in out[0][2].items()}


def test_reused_contexts_give_the_same_result():
    """a second view through the same coarse contexts (their terms still installed) equals a run on fresh ones"""
    sc = synth.make_scene(128, 96, 4, seed=91, all_gt=True)
    sc2 = synth.make_scene(128, 96, 4, seed=92, all_gt=True)
    runs = []
    for reuse in (False, True):
        coarse = None
        if reuse:
            m = _matcher(sc2, _u8(sc2), strict=False, seed=3)
            d2, n2 = _own_result(sc2)
            coarse = api.run_geom_pass_multiscale(m, d2, n2, _maps(sc2), 2, 2, 1)
            m.close()
        m = _matcher(sc, _u8(sc), strict=False, seed=3)
        d, n = _own_result(sc)
        coarse = api.run_geom_pass_multiscale(m, d, n, _maps(sc), 2, 2, 1, coarse=coarse)
        runs.append(m.get_plane())
        m.close()
        for c in coarse:
            c.close()
    _assert_same(runs[1], runs[0], "reused coarse contexts")


# ---- contracts --------------------------------------------------------------------------------------------------------------------
def _code(fn, *a):
    with pytest.raises(api.TsarError) as e:
        fn(*a)
    return e.value.code


def test_error_paths():
    sc = synth.make_scene(64, 48, 3, seed=93, all_gt=True)
    imgs = _u8(sc)
    maps = _maps(sc)
    fine = _matcher(sc, imgs)
    c1, c2, odd = api.Matcher(), api.Matcher(), api.Matcher()
    c1.pyramid_from(fine)
    c2.pyramid_from(c1)
    assert _code(c1.geom_pyramid_from, fine) == api.TSAR_ERR_STATE           # fine has no term
    fine.set_geom_depths(maps)
    assert _code(fine.geom_pyramid_from, fine) == api.TSAR_ERR_INVALID        # itself
    assert _code(c2.geom_pyramid_from, fine) == api.TSAR_ERR_INVALID          # two levels down
    assert _code(odd.geom_pyramid_from, fine) == api.TSAR_ERR_INVALID         # no views
    # the pyramid's images with fine's K (not halved)
    odd.set_params(api.default_params(box_hsize=11, box_vsize=11, depth_min=sc.depth_min, depth_max=sc.depth_max))
    odd.set_views([pyr_down(i, True) for i in imgs], sc.K, sc.R, sc.t, u8=True)
    assert _code(odd.geom_pyramid_from, fine) == api.TSAR_ERR_INVALID
    c1.geom_pyramid_from(fine)
    c2.geom_pyramid_from(c1)                                                 # chains
    # pyramid_planes: fine without plane state, a coarse context of another size
    assert _code(c1.pyramid_planes_from, fine) == api.TSAR_ERR_INVALID
    fine.pm_init()
    assert _code(c2.pyramid_planes_from, fine) == api.TSAR_ERR_INVALID
    assert _code(api.Matcher().pyramid_planes_from, fine) == api.TSAR_ERR_INVALID
    # upsample_merge: coarse without plane state, fine without plane state, a coarse of another size
    assert _code(fine.upsample_merge, c1) == api.TSAR_ERR_INVALID
    assert _code(c1.upsample_merge, c2) == api.TSAR_ERR_INVALID
    c1.pyramid_planes_from(fine)
    c2.pyramid_planes_from(c1)
    assert _code(fine.upsample_merge, c2) == api.TSAR_ERR_INVALID
    assert _code(fine.upsample_merge, fine) == api.TSAR_ERR_INVALID
    fine.upsample_merge(c1)
    # the existing entries keep refusing a term, on either context
    assert _code(c2.pyramid_from, c1) == api.TSAR_ERR_STATE
    assert _code(fine.upsample_planes, c1) == api.TSAR_ERR_STATE
    fine.clear_geom()
    assert _code(fine.upsample_planes, c1) == api.TSAR_ERR_STATE            # c1 still holds its own term
    c1.clear_geom()                                                          # frees c1's maps
    fine.upsample_planes(c1)
    c2.clear_geom()
    c2.pyramid_from(c1)
    for m in (fine, c1, c2, odd):
        m.close()


# ---- quality on the textureless synthetic scene -----------------------------------------------------------------------------------
def test_coarse_levels_on_the_textureless_scene():
    """phase 1 (photometric, 3 iterations) on every view, then phase 2 at L = 0, 1, 2 with the same fine iterations (2; 4 at the
    coarsest level); median relative depth error on textured and textureless pixels"""
    sc = synth.make_scene(256, 192, 4, seed=94, textureless=True, all_gt=True)
    imgs = _u8(sc)
    n = len(imgs)
    res = quality(sc, imgs, n)
    tl0, tl1, tl2 = (res[L]["textureless"] for L in (0, 1, 2))
    tx0, tx1, tx2 = (res[L]["textured"] for L in (0, 1, 2))
    print("quality", res)
    # measured: textureless 0.0296 / 0.0301 / 0.0297, textured 0.00637 / 0.00649 / 0.00649 at L = 0 / 1 / 2.  The coarse levels do not
    # help on this scene; the bound holds them to no worse than 10 % above single scale
    assert tl1 < 1.1 * tl0 and tl2 < 1.1 * tl0, res
    assert tx1 < 1.1 * tx0 and tx2 < 1.1 * tx0, res


def quality(sc, imgs, n, fine_iters=2, coarse_iters=4, phase1_iters=3):
    """{L: {"textured": e, "textureless": e}}: median |D - D_gt| / D_gt of the reference view's phase-2 depth (shared with
    tools/geom_multiscale_timing.py --quality)"""
    from test_gpu_geom import _reorder
    depths, normals = [], []
    for k in range(n):
        im_k, K, R, t, _ = _reorder(sc, imgs, k)
        m = _matcher(sc, im_k, strict=False, seed=41 + k, K=K, R=R, t=t)
        m.pm_init()
        m.pm_iterate(phase1_iters)
        m.compute_disp()
        r = m.get_result(("depth", "normal"))
        m.close()
        depths.append(r["depth"])
        normals.append(r["normal"])
    gt = sc.gt_depth.numpy().astype(np.float64)
    tl = ~sc.textured.numpy()
    out = {}
    for L in (0, 1, 2):
        m = _matcher(sc, imgs, strict=False, seed=41)
        api.run_geom_pass_multiscale(m, depths[0], normals[0], [None] + depths[1:], L, coarse_iters, fine_iters)
        d = m.get_result(("depth",))["depth"].astype(np.float64)
        m.close()
        err = np.abs(d - gt) / gt
        out[L] = {"textured": float(np.median(err[~tl])), "textureless": float(np.median(err[tl]))}
    return out


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")


def _cli(*args, ok=True):
    import subprocess
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    if ok:
        assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_cli_geom_multi_scale(tmp_path):
    from tsar_mvs_amd import io as tio
    sc = synth.make_scene(128, 96, 3, seed=95, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    common = ["-mslp_folder", root, "-images_folder", root + "images/", "--iterations=3", "--blocksize=11", "--n_best=1", "--seed=7"]
    geom = ["--all", "--gpus=1", *common, "--geom_consistency", "--geom_iterations=2"]
    vd = lambda k: root + f"APD/{k:08d}/"
    base = _cli(CLI, *geom)
    assert base.stdout.count("(geom): ok") == n
    rec0 = open(vd(0) + "TSAR_geom.txt").read()
    assert "geom_multi_scale" not in rec0 and rec0.count("\n") == 1
    ms = geom + ["--geom_multi_scale=1", "--geom_coarse_iterations=3"]
    first = _cli(CLI, *ms)
    assert first.stdout.count("(geom): ok") == n
    assert "outputs present, skipped" in first.stdout                          # phase 1 is not recomputed
    assert first.stdout.count("outputs present, skipped") == n
    rec = open(vd(0) + "TSAR_geom.txt").read()
    assert rec == rec0 + "geom_multi_scale=1 geom_coarse_iterations=3\n", rec
    for k in range(n):
        ids = [k] + [s for s in range(n) if s != k]
        imgs = [tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views(imgs, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), np.stack([c[2] for c in cams]), u8=True)
        src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
        coarse = api.run_geom_pass_multiscale(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, 1, 3, 2)
        r = m.get_result(("depth", "normal"))
        m.close()
        for c in coarse:
            c.close()
        assert np.array_equal(r["depth"].view(np.uint32), tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb").view(np.uint32)), k
        assert np.array_equal(r["normal"].view(np.uint32), tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb").view(np.uint32)), k
    again = _cli(CLI, *ms)
    assert again.stdout.count("geom outputs present, skipped") == n
    # --geom_coarse_iterations defaults to --geom_iterations
    dflt = _cli(CLI, *geom, "--geom_multi_scale=1")
    assert dflt.stdout.count("(geom): ok") == n
    assert open(vd(0) + "TSAR_geom.txt").read() == rec0 + "geom_multi_scale=1 geom_coarse_iterations=2\n"
    # back to L = 0: phase 2 only, and the record is today's byte for byte
    back = _cli(CLI, *geom)
    assert back.stdout.count("(geom): ok") == n and back.stdout.count("outputs present, skipped") == n
    assert open(vd(0) + "TSAR_geom.txt").read() == rec0


def test_cli_every_geom_switch_at_once(tmp_path):
    """--geom_multi_scale, --geom_cross_view, --geom_plane_prior and --consistency_filter in one run: each view's geom maps are, bit for
    bit, api.run_geom_pass_multiscale with the same switches on the files the tool read (the term, then the prior, then the merge, then the
    chain down), and its filtered map is Matcher.geom_check on the geom maps"""
    import shutil
    from tsar_mvs_amd import io as tio
    sc = synth.make_scene(96, 72, 2, seed=95)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    vd = lambda k: root + f"APD/{k:08d}/"
    common = ["--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=2", "--blocksize=11", "--n_best=1", "--seed=7"]
    _cli(CLI, *common)
    for k in range(n):                                 # P: a copy of each view's phase-1 maps
        shutil.copy(vd(k) + "TSAR_disp.dmb", vd(k) + "P_disp.dmb")
        shutil.copy(vd(k) + "TSAR_normals.dmb", vd(k) + "P_normals.dmb")
    out = _cli(CLI, *common, "--geom_consistency", "--geom_iterations=1", "--geom_multi_scale=1", "--geom_cross_view=1", "--geom_plane_prior=P",
               "--consistency_filter=1")
    assert out.stdout.count("(geom): ok") == n and out.stdout.count("(filter): ok") == n and "no plane prior" not in out.stdout
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for k in range(n):
        ids = [k] + [s for s in range(n) if s != k]
        imgs = [tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views(imgs, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), np.stack([c[2] for c in cams]), u8=True)
        src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
        coarse = api.run_geom_pass_multiscale(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, levels=1,
                                              coarse_iters=1, fine_iters=1, cross_view=1,
                                              prior=(tio.read_dmb(vd(k) + "P_disp.dmb"), tio.read_dmb(vd(k) + "P_normals.dmb")))
        r = m.get_result(("depth", "normal"))
        geom_depth = tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb")
        assert np.array_equal(bits(r["depth"]), bits(geom_depth)), k
        assert np.array_equal(bits(r["normal"]), bits(tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb"))), k
        # the filter: the geom maps checked against the sources' geom maps, K = 1
        m.clear_plane_prior()
        m.set_geom_depths([None] + [tio.read_dmb(vd(i) + "TSAR_geom_disp.dmb") for i in ids[1:]], weight=0.0)
        kept = m.geom_check(geom_depth, min_consistent=1, want=("depth",))["depth"]
        m.close()
        for c in coarse:
            c.close()
        assert np.array_equal(bits(kept), bits(tio.read_dmb(vd(k) + "TSAR_filtered_disp.dmb"))), k

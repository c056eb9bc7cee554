"""The plane-prior term (include/tsar.h tsar_set_plane_prior / tsar_clear_plane_prior / tsar_get_plane_prior): bit for bit against
the library's own score without it plus the numpy float32 restatement of the term (test_plane_prior_cpu.py); the held prior; one
propagation launch as the composition of the library's scorer; stored costs; weights 0; the memo and the packed form; what the
term is for; the error paths; run_geom_pass; the command line."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from test_plane_prior_cpu import MAXCOST, add_plane_prior
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def _u8(sc):
    return [im.numpy().astype(np.uint8) for im in sc.images]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same(a, b):
    for u, v in zip(a, b):
        assert _bits_equal(u, v)


def _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=5, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m = api.Matcher()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m.set_params(api.default_params(box_hsize=box, box_vsize=box, n_best=n_best, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV if strict else 0, seed=seed))
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    return m


def _oracle(sc):
    """the CPU oracle of the scene, for its per-pixel helpers (depth_from_plane, select_candidates): they do not depend on the
    arithmetic mode, the window or the images"""
    return ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max)


def _gt_maps(sc):
    """every view's ground-truth depth with a block of 0 (no estimate) in each source map; entry 0 is None"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
    maps[0] = None
    return maps


def _gt_prior(sc, scale=1.0):
    """(depth, normal_world) of the reference view's ground truth: camera -> world is R^T n"""
    depth = (sc.gt_depth.numpy().astype(np.float64) * scale).astype(F32)
    R0 = np.asarray(sc.R[0], np.float64)
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ R0).astype(F32)
    return depth, normal_world


def _plane_depths(orc, planes, mask=None):
    h, w = planes.shape[:2]
    D = np.zeros((h, w), F32)
    for y in range(h):
        for x in range(w):
            if mask is None or mask[y, x]:
                D[y, x] = orc.depth_from_plane(planes[y, x], x, y)
    return D


# ---- 1. the term equals the restatement, bit for bit -----------------------------------------------------------------------------
HOLE = (slice(20, 32), slice(30, 46))          # 12 x 16 pixels of depth 0
NAN_AT = (5, 7)                                # one NaN normal


def _prior_with_holes(sc):
    depth, normal = _gt_prior(sc)
    depth[HOLE] = 0
    normal[NAN_AT] = np.nan
    return depth, normal


def _test_planes(sc, m, kind, depth_clip):
    h, w = sc.gt_depth.shape
    gt = np.ascontiguousarray(synth.gt_planes(sc).numpy())
    if kind == "gt":
        return gt
    if kind == "random":
        m.pm_init()
        return m.get_plane()[0]
    if kind == "outside":                                        # fronto-parallel, far outside both clips
        planes = np.zeros((h, w, 4), F32)
        planes[..., 2] = -1.0
        planes[..., 3] = F32(sc.depth_max) * F32(0.97)
        return planes
    # ground truth scaled so that rel = |D - Dp| / Dp falls within 1e-6 of depth_clip, on both sides (the plane's depth at every
    # pixel scales with its offset d)
    ys, xs = np.mgrid[0:h, 0:w]
    delta = np.where((xs + ys) % 2 == 0, 5e-7, -5e-7)
    sign = np.where(xs % 2 == 0, 1.0, -1.0)
    planes = gt.copy()
    planes[..., 3] = (gt[..., 3].astype(np.float64) * (1.0 + sign * (float(depth_clip) + delta))).astype(F32)
    return planes


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("box", [11, 19])
@pytest.mark.parametrize("n_best", [1, 2])
@pytest.mark.parametrize("kind", ["gt", "random", "outside", "clip_edge"])
def test_term_is_the_restatement_bit_for_bit(strict, box, n_best, kind):
    sc = synth.make_scene(64, 48, 3, seed=61, all_gt=True)
    imgs = _u8(sc)
    m = _matcher(sc, imgs, box=box, n_best=n_best, strict=strict)
    orc = _oracle(sc)
    pd, pn = _prior_with_holes(sc)
    planes = _test_planes(sc, m, kind, 0.02)
    D = _plane_depths(orc, planes)
    for maps in (None, _gt_maps(sc)):                            # (a) no geometric term, (b) ground-truth maps at weight 0.2
        m.clear_plane_prior()
        m.clear_geom()
        if maps is not None:
            m.set_geom_depths(maps, weight=0.2, clip=3.0)
        c0, bv0, rt0 = m.pm_cost_planes(planes)
        m.set_plane_prior(pd, pn)
        held = m.get_plane_prior()
        q = m.plane_prior_params
        params = (F32(q.weight_depth), F32(q.weight_normal), F32(q.depth_clip), F32(q.normal_clip))
        c1, bv1, rt1 = m.pm_cost_planes(planes)
        want = add_plane_prior(c0, bv0, held, planes, D, params)
        bad = c1.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (kind, maps is not None, int(bad.sum()), c1[bad][:4], want[bad][:4])
        assert np.array_equal(bv1, bv0) and _bits_equal(rt1, rt0)
        assert _bits_equal(c1[HOLE], c0[HOLE]) and c1[NAN_AT] == c0[NAN_AT]
        assert not held[HOLE].any() and not held[NAN_AT].any()
        invalid = bv0 < 0
        assert np.all(c0[invalid] == MAXCOST) and _bits_equal(c1[invalid], c0[invalid])
        if maps is None:
            assert np.array_equal(invalid, c0 == MAXCOST)        # without the geometric term only the invalid cost equals MAXCOST
        assert not _bits_equal(c1, c0)                           # the term is not idle
        if kind == "clip_edge":
            rel = np.abs(D - held[..., 3]) / np.where(held[..., 3] > 0, held[..., 3], 1)
            at = (held[..., 3] > 0) & (np.abs(rel - F32(0.02)) < 1e-6)
            assert (rel[at] < F32(0.02)).any() and (rel[at] >= F32(0.02)).any() and at.mean() > 0.5
    m.close()


# ---- 2. the held prior ------------------------------------------------------------------------------------------------------------
def test_held_normals_are_load_planes_normals():
    sc = synth.make_scene(64, 48, 3, seed=61, all_gt=True)
    m = _matcher(sc, _u8(sc))
    depth, normal = _gt_prior(sc)
    m.load_planes(depth, normal)
    loaded = m.get_plane()[0]
    m.set_plane_prior(depth, normal)
    held = m.get_plane_prior()
    assert _bits_equal(held[..., :3], loaded[..., :3])
    assert _bits_equal(held[..., 3], depth)
    pd, pn = _prior_with_holes(sc)
    pd[0, 0], pd[0, 1], pd[0, 2] = np.inf, -1.0, np.nan
    pn[1, 1, 2] = np.inf
    m.set_plane_prior(pd, pn)
    held = m.get_plane_prior()
    none = np.zeros(pd.shape, bool)
    none[HOLE] = True
    none[NAN_AT] = True
    none[0, :3] = True
    none[1, 1] = True
    assert not held[none].any()
    assert _bits_equal(held[~none][:, :3], loaded[~none][:, :3]) and _bits_equal(held[~none][:, 3], depth[~none])
    m.close()


# ---- 3. one propagation-only launch is the composition of the library's scorer ------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
def test_propagation_launch_is_the_composition_of_the_scorer(strict):
    sc = synth.make_scene(101, 67, 3, seed=69, all_gt=True)
    m = _matcher(sc, _u8(sc), strict=strict, seed=21)
    orc = _oracle(sc)
    cam = orc.camera(0)
    dmin, dmax = F32(cam.depthMin), F32(cam.depthMax)
    m.set_geom_depths(_gt_maps(sc), weight=0.2)
    m.set_plane_prior(*_gt_prior(sc, 1.01))
    m.pm_init()
    m.pm_iterate(1)
    h, w = m.h, m.w
    ys, xs = np.mgrid[0:h, 0:w]
    taken = 0
    for colour in (0, 1):
        P, Cst, BV, RT = (a.copy() for a in m.get_plane())
        active = (xs + ys) % 2 == colour
        cand = np.full((h, w, 8), -1, np.int32)
        for y in range(h):
            for x in range(w):
                if active[y, x]:
                    cand[y, x] = orc.select_candidates(Cst, x, y)          # -1: the arm's border test fails
        flatP = P.reshape(-1, 4)
        eP, eC, eBV, eRT = P.copy(), Cst.copy(), BV.copy(), RT.copy()
        for a in range(8):
            has = active & (cand[..., a] >= 0)
            planes_a = np.where(has[..., None], flatP[np.maximum(cand[..., a], 0)], P).astype(F32)
            ca, bva, rta = m.pm_cost_planes(planes_a)
            Da = _plane_depths(orc, planes_a, has)
            take = has & (Da >= dmin) & (Da <= dmax) & (ca < eC)         # the range test, then the strict <, in arm order
            eP[take], eC[take], eBV[take], eRT[take] = planes_a[take], ca[take], bva[take], rta[take]
            taken += int(take.sum())
        m.pm_sweep(colour, do_prop=True, do_refine=False)
        gP, gC, gBV, gRT = m.get_plane()
        assert _bits_equal(gP, eP), int((gP.view(np.uint32) != eP.view(np.uint32)).any(-1).sum())
        assert _bits_equal(gC, eC)
        assert np.array_equal(gBV, eBV) and _bits_equal(gRT, eRT)
    assert taken > h * w // 50                                       # the launches did something
    m.close()


# ---- 4. the stored cost is the plane's score -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("with_maps", [False, True])
def test_stored_cost_is_the_planes_score(strict, with_maps):
    sc = synth.make_scene(160, 120, 3, seed=64, all_gt=True)
    m = _matcher(sc, _u8(sc), strict=strict, seed=11)
    m.enable_kernel_timing(True)
    depth, normal = _gt_prior(sc)
    own = depth.copy()
    own[40:60, 50:90] = 0                                            # no estimate here: rescore draws
    m.load_planes(own, normal)
    if with_maps:
        m.set_geom_depths(_gt_maps(sc), weight=0.2)
    pd = depth.copy()
    pd[10:30, 100:140] = 0
    m.set_plane_prior(pd, normal)
    m.rescore()
    planes, c, bv, rt = m.get_plane()
    cc, cbv, crt = m.pm_cost_planes(planes)
    assert _bits_equal(c, cc) and np.array_equal(bv, cbv) and _bits_equal(rt, crt)
    m.pm_iterate(3)
    planes, c, _, _ = m.get_plane()
    cc, _, _ = m.pm_cost_planes(planes)
    assert _bits_equal(c, cc)
    t = m.kernel_timing()
    assert "pm_rescore" in t and "pm_sweep_geom" in t and "pm_sweep" not in t and "plane_prior" in t
    m.close()


# ---- 5. both weights 0 ----------------------------------------------------------------------------------------------------------------
def _run(sc, prior, strict, iters, env=None, per_call=False, timing=False, maps=None, **prior_kw):
    m = _matcher(sc, _u8(sc), strict=strict, seed=9, env=env)
    if timing:
        m.enable_kernel_timing(True)
    if maps is not None:
        m.set_geom_depths(maps, weight=0.2)
    if prior is not None:
        m.set_plane_prior(*prior, **prior_kw)
    m.pm_init()
    if per_call:
        for _ in range(iters):
            m.pm_iterate(1)
    else:
        m.pm_iterate(iters)
    st = m.get_plane()
    t = m.kernel_timing() if timing else None
    m.close()
    return st, t


@pytest.mark.parametrize("strict", [True, False])
def test_both_weights_zero_is_the_photometric_path(strict):
    sc = synth.make_scene(160, 120, 3, seed=62, all_gt=True)
    a, _ = _run(sc, None, strict, 4)
    b, t = _run(sc, _gt_prior(sc, 1.05), strict, 4, timing=True, weight_depth=0.0, weight_normal=0.0)
    _same(a, b)
    assert "pm_sweep_geom" in t and "pm_sweep" not in t              # (every sweep ran the kernels with the term)


# ---- 6. the memo and the packed form change no bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
def test_memo_and_packed_form_change_no_bit_under_the_prior(strict):
    sc = synth.make_scene(333, 251, 4, seed=63, all_gt=True)
    prior = _gt_prior(sc, 1.01)
    prior[0][100:140, 60:200] = 0                                    # pixels without a prior among them
    iters = 6
    plain, t = _run(sc, prior, strict, iters, {"TSAR_MEMO": "0"}, timing=True)
    assert "pm_sweep_packed" not in t                                # (no memo: no packed form either)
    early, t = _run(sc, prior, strict, iters, {"TSAR_COMPACT_FROM": "2"}, timing=True)
    assert "pm_sweep_packed" in t
    rolled, t = _run(sc, prior, strict, iters, {"TSAR_COMPACT_FROM": "-1"}, timing=True)
    assert "pm_sweep_packed" not in t
    calls, _ = _run(sc, prior, strict, iters, {}, per_call=True)
    _same(plain, early)
    _same(plain, rolled)
    _same(plain, calls)
    photometric, _ = _run(sc, None, strict, iters)
    assert not _bits_equal(plain[0], photometric[0])                 # the prior changed the result


# ---- 7. does what it is for -----------------------------------------------------------------------------------------------------------
def test_prior_does_what_it_is_for():
    """The simulated set-up of DESIGN.md section 8 on the GPU, strict mode.  Bars, from the CPU simulation (half of its gains, and the
    size of its wrong-prior difference on the other side): constant albedo with the true prior >= control + 0.19, textured with the
    true prior >= control + 0.10, textured with the wrong prior (depth x 1.1) >= control - 0.03."""
    sc = synth.make_scene(160, 120, 3, seed=65, textureless=True, all_gt=True, step=0.2)
    rng = np.random.default_rng(3)
    imgs = []
    for im in sc.images:                                             # in view order
        a = im.numpy().astype(np.int64)
        imgs.append(np.clip(a + rng.integers(-1, 2, a.shape), 0, 255).astype(np.uint8))
    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()

    def shares(prior):
        m = _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=77)
        if prior is not None:
            m.set_plane_prior(*prior)
        m.pm_init()
        m.pm_iterate(3)
        m.compute_disp()
        d = m.get_result(("depth",))["depth"]
        m.close()
        ok = np.abs(d - gt) <= 1e-2 * gt
        return float(ok[tex].mean()), float(ok[~tex].mean())

    c_tex, c_flat = shares(None)
    g_tex, g_flat = shares(_gt_prior(sc))
    w_tex, w_flat = shares(_gt_prior(sc, 1.1))
    print(f"within 1e-2 of ground truth, textured / constant albedo: control {c_tex:.4f} / {c_flat:.4f}; ground-truth prior {g_tex:.4f} / "
          f"{g_flat:.4f}; wrong prior (depth x 1.1) {w_tex:.4f} / {w_flat:.4f}")
    assert g_flat >= c_flat + 0.19
    assert g_tex >= c_tex + 0.10
    assert w_tex >= c_tex - 0.03


# ---- 8. the error paths ----------------------------------------------------------------------------------------------------------------
def test_error_paths():
    sc = synth.make_scene(64, 48, 2, seed=66, all_gt=True)
    imgs = _u8(sc)
    depth, normal = _gt_prior(sc)
    m = _matcher(sc, imgs)
    with pytest.raises(api.TsarError) as e:
        m.get_plane_prior()                                          # no prior yet
    assert e.value.code == api.TSAR_ERR_STATE
    for kw in ({"weight_depth": -0.1}, {"weight_depth": float("nan")}, {"weight_depth": float("inf")}, {"weight_normal": -1.0},
               {"weight_normal": float("inf")}, {"depth_clip": 0.0}, {"depth_clip": -0.02}, {"depth_clip": float("inf")},
               {"depth_clip": float("nan")}, {"angle_clip_deg": 0.0}, {"angle_clip_deg": float("nan")}):
        with pytest.raises(api.TsarError) as e:
            m.set_plane_prior(depth, normal, **kw)
        assert e.value.code == api.TSAR_ERR_INVALID, kw
    import ctypes as C
    d, n = api._ptr(depth)[0], api._ptr(normal)[0]
    good = api.PlanePriorParams(0.1, 0.05, 0.02, 0.134)
    L = m.L
    assert L.tsar_set_plane_prior(m._ctx, None, n, api.MEM_HOST, C.byref(good)) == api.TSAR_ERR_INVALID
    assert L.tsar_set_plane_prior(m._ctx, d, None, api.MEM_HOST, C.byref(good)) == api.TSAR_ERR_INVALID
    assert L.tsar_set_plane_prior(m._ctx, d, n, api.MEM_HOST, None) == api.TSAR_ERR_INVALID
    assert L.tsar_set_plane_prior(m._ctx, d, n, 77, C.byref(good)) == api.TSAR_ERR_INVALID
    for clip in (2.5, -0.1):                                         # normal_clip outside (0, 2]
        bad = api.PlanePriorParams(0.1, 0.05, 0.02, clip)
        assert L.tsar_set_plane_prior(m._ctx, d, n, api.MEM_HOST, C.byref(bad)) == api.TSAR_ERR_INVALID
    assert L.tsar_set_plane_prior(m._ctx, d, n, api.MEM_HOST, C.byref(api.PlanePriorParams(0.1, 0.05, 0.02, 2.0))) == api.TSAR_OK
    assert L.tsar_get_plane_prior(m._ctx, None, api.MEM_HOST) == api.TSAR_ERR_INVALID
    dflt = api.PlanePriorParams()
    L.tsar_default_plane_prior_params(C.byref(dflt))
    assert (dflt.weight_depth, dflt.weight_normal, dflt.depth_clip) == (F32(0.1), F32(0.05), F32(0.02))
    assert dflt.normal_clip == F32(1.0 - np.cos(np.deg2rad(30.0)))
    # coarse-to-fine refuses a context with a prior, as with the geometric term
    m.set_plane_prior(depth, normal)
    c = api.Matcher()
    with pytest.raises(api.TsarError) as e:
        c.pyramid_from(m)
    assert e.value.code == api.TSAR_ERR_STATE
    m.clear_plane_prior()
    c.pyramid_from(m)
    c.pm_init()
    m.set_plane_prior(depth, normal)
    with pytest.raises(api.TsarError) as e:
        m.upsample_planes(c)
    assert e.value.code == api.TSAR_ERR_STATE
    m.clear_plane_prior()
    with pytest.raises(api.TsarError) as e:
        m.get_plane_prior()                                          # refused after clear_plane_prior
    assert e.value.code == api.TSAR_ERR_STATE
    m.upsample_planes(c)
    c.close()
    # set_views removes the prior
    m.set_plane_prior(depth, normal)
    assert m.get_plane_prior()[..., 3].any()
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    assert m.plane_prior_params is None
    with pytest.raises(api.TsarError) as e:
        m.get_plane_prior()
    assert e.value.code == api.TSAR_ERR_STATE
    m.close()


def test_a_context_without_source_views_refuses_a_prior():
    sc = synth.make_scene(64, 48, 2, seed=66, all_gt=True)
    depth, normal = _gt_prior(sc)
    only = api.Matcher()
    only.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, flags=0, seed=1))
    only.set_views(_u8(sc)[:1], sc.K[:1], sc.R[:1], sc.t[:1], u8=True)
    with pytest.raises(api.TsarError) as e:
        only.set_plane_prior(depth, normal)
    assert e.value.code == api.TSAR_ERR_STATE
    only.close()


# ---- 9. run_geom_pass ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pass_inputs():
    """a scene, every view's photometric result (view 0 as reference; the sources' maps are their ground truth), computed once"""
    sc = synth.make_scene(128, 96, 3, seed=70, all_gt=True, textureless=True)
    imgs = _u8(sc)
    m = _matcher(sc, imgs, strict=False, seed=13)
    m.pm_init()
    m.pm_iterate(3)
    m.compute_disp()
    r = m.get_result(("depth", "normal"))
    m.close()
    return sc, imgs, r["depth"].copy(), r["normal"].copy(), _gt_maps(sc)


def _result(m):
    r = m.get_result(("depth", "normal"))
    return r["depth"].copy(), r["normal"].copy()


def test_run_geom_pass_with_and_without_a_prior(pass_inputs):
    sc, imgs, d1, n1, maps = pass_inputs
    prior = _gt_prior(sc, 1.02)
    kw = {"weight_depth": 0.2, "angle_clip_deg": 20.0}
    # prior=None: the pass as it was, call for call
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, d1, n1, maps, 2)
    none = _result(m)
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    m.load_planes(d1, n1)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.rescore()
    m.pm_iterate(2)
    m.compute_disp()
    _same(none, _result(m))
    m.close()
    # with a prior: the hand-written sequence
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, d1, n1, maps, 2, prior=prior, prior_params=kw)
    with_prior = _result(m)
    assert m.plane_prior_params is not None and m.plane_prior_params.weight_depth == F32(0.2)
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    m.load_planes(d1, n1)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.set_plane_prior(*prior, **kw)
    m.rescore()
    m.pm_iterate(2)
    m.compute_disp()
    _same(with_prior, _result(m))
    m.close()
    assert not _bits_equal(with_prior[0], none[0])
    with pytest.raises(ValueError):
        api.run_geom_pass(m, d1, n1, maps, 2, prior_params=kw)       # settings without a prior


def test_run_geom_pass_multiscale_with_a_prior(pass_inputs):
    sc, imgs, d1, n1, maps = pass_inputs
    prior = _gt_prior(sc, 1.02)
    m = _matcher(sc, imgs, strict=False, seed=13)
    coarse = api.run_geom_pass_multiscale(m, d1, n1, maps, 1, 2, 2, prior=prior)
    got = _result(m)
    with pytest.raises(api.TsarError):
        coarse[0].get_plane_prior()                                  # the prior is on the full-resolution context only
    assert m.get_plane_prior()[..., 3].any()
    for c in coarse:
        c.close()
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    c = api.Matcher()
    c.pyramid_from(m)
    m.load_planes(d1, n1)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.set_plane_prior(*prior)
    c.geom_pyramid_from(m)
    c.pyramid_planes_from(m)
    c.pm_iterate(2)
    m.upsample_merge(c)
    m.pm_iterate(2)
    m.compute_disp()
    _same(got, _result(m))
    c.close()
    m.close()
    # without a prior the multi-scale pass is what it was
    m = _matcher(sc, imgs, strict=False, seed=13)
    coarse = api.run_geom_pass_multiscale(m, d1, n1, maps, 1, 2, 2)
    none = _result(m)
    for c in coarse:
        c.close()
    m.close()
    assert not _bits_equal(none[0], got[0])


# ---- 10. the command line: tsar_gipuma --all --geom_consistency --geom_plane_prior=STEM -------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")


def _cli(*args):
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_cli_geom_plane_prior(tmp_path):
    from tsar_mvs_amd import io as tio
    sc = synth.make_scene(128, 96, 3, seed=68, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    vd = lambda k: root + f"APD/{k:08d}/"
    common = ["-mslp_folder", root, "-images_folder", root + "images/", "--iterations=3", "--blocksize=11", "--n_best=1", "--seed=7"]
    _cli(CLI, "--all", "--gpus=1", *common)
    for k in range(n):
        shutil.copy(vd(k) + "TSAR_disp.dmb", vd(k) + "PRIOR_disp.dmb")
        shutil.copy(vd(k) + "TSAR_normals.dmb", vd(k) + "PRIOR_normals.dmb")
    geom = ["--all", "--gpus=1", *common, "--geom_consistency", "--geom_iterations=2"]
    # the same command without the switch writes the record it always wrote
    _cli(CLI, *geom, "--force")
    plain_record = open(vd(0) + "TSAR_geom.txt").read()
    assert plain_record.count("\n") == 1 and plain_record.startswith("geom_iterations=2 geom_weight=") and "prior" not in plain_record
    plain_depth = tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb")
    prior = [*geom, "--geom_plane_prior=PRIOR", "--geom_prior_weight_depth=0.2", "--geom_prior_angle_clip=20"]
    first = _cli(CLI, *prior, "--force")
    assert first.stdout.count("(geom): ok") == n and "no plane prior" not in first.stdout
    record = open(vd(0) + "TSAR_geom.txt").read()
    assert record == plain_record + "geom_plane_prior=PRIOR geom_prior_weight_depth=0.200000003 geom_prior_weight_normal=0.0500000007 " \
                                    "geom_prior_depth_clip=0.0199999996 geom_prior_angle_clip=20\n"
    assert not _bits_equal(plain_depth, tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb"))
    # bit for bit against api.run_geom_pass with the same prior and settings
    for k in range(n):
        ids = [k] + [s for s in range(n) if s != k]
        imgs = [tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views(imgs, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), np.stack([c[2] for c in cams]), u8=True)
        src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
        api.run_geom_pass(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, 2,
                          prior=(tio.read_dmb(vd(k) + "PRIOR_disp.dmb"), tio.read_dmb(vd(k) + "PRIOR_normals.dmb")),
                          prior_params={"weight_depth": 0.2, "angle_clip_deg": 20.0})
        r = m.get_result(("depth", "normal"))
        m.close()
        assert _bits_equal(r["depth"], tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb")), k
        assert _bits_equal(r["normal"], tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb")), k
    # a rerun skips; touching a prior file recomputes that view
    again = _cli(CLI, *prior)
    assert again.stdout.count("geom outputs present, skipped") == n
    os.utime(vd(1) + "PRIOR_normals.dmb")
    touched = _cli(CLI, *prior)
    assert touched.stdout.count("(geom): ok") == 1 and touched.stdout.count("geom outputs present, skipped") == n - 1
    # a view with a missing prior file runs without it and is named
    os.remove(vd(2) + "PRIOR_disp.dmb")
    missing = _cli(CLI, *prior, "--force")
    assert missing.stdout.count("(geom): ok") == n
    lines = [ln for ln in missing.stdout.splitlines() if "no plane prior" in ln]
    assert len(lines) == 1 and "view 00000002" in lines[0]
    # the same command without the switch: a record byte-identical to the one before
    _cli(CLI, *geom, "--force")
    assert open(vd(0) + "TSAR_geom.txt").read() == plain_record
    assert _bits_equal(plain_depth, tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb"))

"""The plane-prior builder on the GPU (include/tsar.h tsar_build_plane_prior, Matcher.build_plane_prior, run_geom_pass's build_prior,
tsar_gipuma --geom_build_prior): depth, normal and level bit for bit against the numpy restatement (test_plane_prior_build_cpu.py), every
pixel, with and without a score, in host and device memory, in strict and fast contexts; the call moves nothing in the context; the
error codes; the passes' composition; what the built prior is for; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_plane_prior_build_cpu import build_plane_prior_ref, level_shapes
from test_gpu_geom import _bits_equal, _gt_maps, _matcher, _reorder, _u8
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")

# ---- 1. bit for bit -----------------------------------------------------------------------------------------------------------------
# name: (w, h, cell)
CASES = {"all_64x48_c4": (64, 48, 4), "thinned_101x67_c8": (101, 67, 8), "thinned_101x67_c5": (101, 67, 5), "hole_192x128_c4": (192, 128, 4)}
_SCENES, _REFS = {}, {}


def _scene(w, h):
    """per size, built once: the scene and a strict and a fast context holding its views"""
    if (w, h) not in _SCENES:
        sc = synth.make_scene(w, h, 2, seed=81, all_gt=True, textureless=True)
        imgs = _u8(sc)
        _SCENES[(w, h)] = (sc, {strict: _matcher(sc, imgs, strict=strict) for strict in (True, False)})
    return _SCENES[(w, h)]


def _inputs(name, score_kind):
    w, h, cell = CASES[name]
    sc, _ = _scene(w, h)
    gt = sc.gt_depth.numpy().astype(F32)
    rng = np.random.default_rng(11)
    depth = gt.copy()
    if name.startswith("thinned"):
        # the textured pixels thinned to about 90 %, and every kind of non-candidate among the dropped
        drop = ~sc.textured.numpy() | (rng.random((h, w)) >= 0.9)
        bad = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf], F32)
        depth[drop] = bad[rng.integers(0, len(bad), int(drop.sum()))]
    if name.startswith("hole"):
        depth[34:94, 56:136] = 0                                     # 80 x 60 pixels
    score = None
    if score_kind == "cost":
        score = rng.random((h, w)).astype(F32) * F32(2)
        pick = rng.integers(0, 40, (h, w))
        for k, val in enumerate([np.nan, -1.0, np.inf, -0.0, 0.0]):  # no candidates, except the two zeros
            score[pick == k] = val
    if score_kind == "ties":
        score = rng.integers(0, 3, (h, w)).astype(F32)
    return sc, depth, score, cell


def _ref(name, score_kind):
    """the restatement's outputs, computed once and shared"""
    if (name, score_kind) not in _REFS:
        sc, depth, score, cell = _inputs(name, score_kind)
        out = build_plane_prior_ref(depth, score, sc.K[0], sc.R[0], cell)
        for a in out:
            a.setflags(write=False)
        _REFS[(name, score_kind)] = out
    return _REFS[(name, score_kind)]


def _equal(res, ref):
    d, n, lv = ref
    return _bits_equal(res["depth"], d) and _bits_equal(res["normal"], n) and res["level"].dtype == np.uint8 and np.array_equal(res["level"], lv)


@pytest.mark.parametrize("score_kind", ["none", "cost", "ties"])
@pytest.mark.parametrize("name", list(CASES))
def test_builder_is_the_restatement_bit_for_bit(name, score_kind):
    import torch
    sc, depth, score, cell = _inputs(name, score_kind)
    _, ms = _scene(*CASES[name][:2])
    ref = _ref(name, score_kind)
    levels = set(np.unique(ref[2]).tolist())
    for strict, m in ms.items():                                     # (the same reference for both contexts: they give the same bits)
        host = m.build_plane_prior(depth, score, cell=cell)
        assert _equal(host, ref), (name, score_kind, strict, int((host["level"] != ref[2]).sum()))
        dev = m.build_plane_prior(torch.from_numpy(depth).cuda(), None if score is None else torch.from_numpy(score).cuda(), cell=cell)
        assert all(v.is_cuda for v in dev.values()) and dev["level"].dtype == torch.uint8
        assert _equal({k: v.cpu().numpy() for k, v in dev.items()}, ref), (name, score_kind, strict)
        only = m.build_plane_prior(depth, score, cell=cell, want=("level",))
        assert set(only) == {"level"} and np.array_equal(only["level"], ref[2])
    # the inputs exercise what they are there for
    if name.startswith("all"):
        assert levels == {0, 255} if score_kind == "none" else 0 in levels
    if name.startswith("thinned"):
        assert {0, 1} <= levels                                      # empty cells: some pixels go up
    if name.startswith("hole"):
        assert len(levels - {255}) >= 3, levels                      # the hole is spanned by coarser levels


def test_max_levels_and_other_cells():
    sc, depth, score, _ = _inputs("hole_192x128_c4", "cost")
    _, ms = _scene(192, 128)
    m = ms[False]
    for cell, max_levels in ((4, 1), (4, 2), (2, 0), (16, 0), (7, 3)):
        ref = build_plane_prior_ref(depth, score, sc.K[0], sc.R[0], cell, max_levels)
        assert _equal(m.build_plane_prior(depth, score, cell=cell, max_levels=max_levels), ref), (cell, max_levels)
        if max_levels:
            assert int(ref[2][ref[2] != 255].max()) <= max_levels - 1


# ---- 2. the context is untouched ------------------------------------------------------------------------------------------------------
def test_nothing_in_the_context_moves():
    sc = synth.make_scene(101, 67, 3, seed=82, all_gt=True, textureless=True)
    imgs = _u8(sc)
    maps = _gt_maps(sc)
    maps[0] = None
    gt = sc.gt_depth.numpy().astype(F32)
    R0 = np.asarray(sc.R[0], np.float64)
    prior = ((gt.astype(np.float64) * 1.02).astype(F32), (sc.gt_normal.numpy().astype(np.float64) @ R0).astype(F32))

    def run(build):
        m = _matcher(sc, imgs, strict=False, seed=9)
        m.enable_kernel_timing(True)
        m.set_geom_depths(maps, weight=0.2)
        m.set_plane_prior(*prior)
        m.pm_init()
        m.pm_iterate(2)
        m.compute_disp()
        m.geom_check(gt)                                             # (writes the mask the call must leave alone)
        if build:
            before = (m.get_plane(), m.get_reliable_mask(), m.get_plane_prior(), m.get_result())
            kept = m.geom_check(gt, want=("depth",))["depth"]
            mask = m.get_reliable_mask()
            m.build_plane_prior(kept, before[0][1], cell=4)
            m.build_plane_prior(kept, None, cell=5, want=("level",))
            after = (m.get_plane(), m.get_reliable_mask(), m.get_plane_prior(), m.get_result())
            assert all(_bits_equal(a, b) for a, b in zip(before[0], after[0]))
            assert _bits_equal(mask, after[1]) and _bits_equal(before[2], after[2])
            assert all(_bits_equal(before[3][k], after[3][k]) for k in before[3])
            assert m.plane_prior_params is not None
        m.pm_iterate(1)                                              # the memo, the stored costs, the sweep counter and both terms survived
        state, t = m.get_plane(), m.kernel_timing()
        m.close()
        return state, t

    (with_build, t1), (without, t0) = run(True), run(False)
    assert all(_bits_equal(a, b) for a, b in zip(with_build, without))
    assert t1["plane_prior_build"][0] == 2 and t1["plane_prior_build_supports"][0] == 2 and not any(k.startswith("plane_prior_build") for k in t0)
    sweeps = lambda t: {k: v[0] for k, v in t.items() if k.startswith("pm_")}
    assert sweeps(t1) == sweeps(t0)                                  # (the builder launched no sweep and no rescore of its own)


# ---- 3. the error paths: one test per code -----------------------------------------------------------------------------------------------
def test_without_views_is_a_state_error():
    m = api.Matcher()
    d = np.ones((48, 64), F32)
    out = np.empty_like(d)
    p = api.PlanePriorBuildParams(4, 0)
    rc = m.L.tsar_build_plane_prior(m._ctx, d.ctypes.data_as(C.c_void_p), None, api.MEM_HOST, C.byref(p), out.ctypes.data_as(C.c_void_p), None, None)
    assert rc == api.TSAR_ERR_STATE
    m.close()


def test_invalid_arguments():
    sc, ms = _scene(64, 48)
    m = ms[True]
    gt = sc.gt_depth.numpy().astype(F32)
    out = np.empty_like(gt)
    L, d, o = m.L, gt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = api.PlanePriorBuildParams(4, 0)
    call = lambda depth, mem, p, od, on, ol: L.tsar_build_plane_prior(m._ctx, depth, None, mem, p, od, on, ol)
    assert call(None, api.MEM_HOST, C.byref(good), o, None, None) == api.TSAR_ERR_INVALID          # depth NULL
    assert call(d, api.MEM_HOST, None, o, None, None) == api.TSAR_ERR_INVALID                      # params NULL
    assert call(d, api.MEM_HOST, C.byref(good), None, None, None) == api.TSAR_ERR_INVALID          # every output NULL
    assert call(d, 77, C.byref(good), o, None, None) == api.TSAR_ERR_INVALID                       # unknown mem
    for cell, max_levels in ((1, 0), (0, 0), (-4, 0), (257, 0), (4, -1), (4, 17)):                # out of range
        assert call(d, api.MEM_HOST, C.byref(api.PlanePriorBuildParams(cell, max_levels)), o, None, None) == api.TSAR_ERR_INVALID, (cell, max_levels)
    for cell in (48, 64, 256):                                                                     # too small for one level: h <= cell
        assert call(d, api.MEM_HOST, C.byref(api.PlanePriorBuildParams(cell, 0)), o, None, None) == api.TSAR_ERR_INVALID, cell
    for cell, max_levels in ((2, 16), (47, 0), (4, 1)):                                            # the ends of the ranges are inside
        assert call(d, api.MEM_HOST, C.byref(api.PlanePriorBuildParams(cell, max_levels)), o, None, None) == api.TSAR_OK, (cell, max_levels)
    with pytest.raises(api.TsarError) as e:
        m.build_plane_prior(gt, cell=300)
    assert e.value.code == api.TSAR_ERR_INVALID
    dflt = api.PlanePriorBuildParams()
    L.tsar_default_plane_prior_build_params(C.byref(dflt))
    assert (dflt.cell, dflt.max_levels) == (4, 0)
    assert level_shapes(64, 48, 47) == [(2, 2)]


# ---- 4. composition ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pass_inputs():
    """a scene, view 0's photometric result and every source's ground-truth map, computed once"""
    sc = synth.make_scene(128, 96, 3, seed=70, all_gt=True, textureless=True)
    imgs = _u8(sc)
    m = _matcher(sc, imgs, strict=False, seed=13)
    m.pm_init()
    m.pm_iterate(3)
    m.compute_disp()
    r = m.get_result(("depth", "normal"))
    m.close()
    maps = _gt_maps(sc)
    maps[0] = None
    return sc, imgs, r["depth"].copy(), r["normal"].copy(), maps


def _result(m):
    r = m.get_result(("depth", "normal"))
    return r["depth"].copy(), r["normal"].copy()


BUILD = {"cell": 5, "max_levels": 3, "reproj_error": 1.5, "depth_diff": 0.02, "min_consistent": 1}
PRIOR_KW = {"weight_depth": 0.2, "angle_clip_deg": 20.0}


def _by_hand(m, d1, n1, maps):
    """the calls of run_geom_pass's build_prior, up to the prior's rescore"""
    m.load_planes(d1, n1)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.rescore()
    score = m.get_plane()[1]
    kept = m.geom_check(d1, reproj_error=1.5, depth_diff=0.02, min_consistent=1, want=("depth",))["depth"]
    built = m.build_plane_prior(kept, score, cell=5, max_levels=3, want=("depth", "normal"))
    assert (built["depth"] > 0).mean() > 0.5
    m.set_plane_prior(built["depth"], built["normal"], **PRIOR_KW)
    m.rescore()
    return built


def test_run_geom_pass_builds_the_prior(pass_inputs):
    sc, imgs, d1, n1, maps = pass_inputs
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, d1, n1, maps, 2, build_prior=BUILD, prior_params=PRIOR_KW)
    got, held = _result(m), m.get_plane_prior()
    assert m.plane_prior_params.weight_depth == F32(0.2)
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    built = _by_hand(m, d1, n1, maps)
    m.pm_iterate(2)
    m.compute_disp()
    assert all(_bits_equal(a, b) for a, b in zip(got, _result(m)))
    assert _bits_equal(held, m.get_plane_prior()) and _bits_equal(held[..., 3], built["depth"])
    m.close()
    # build_prior=None is the pass as it was, call for call
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, d1, n1, maps, 2, build_prior=None)
    none = _result(m)
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    m.load_planes(d1, n1)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    m.rescore()
    m.pm_iterate(2)
    m.compute_disp()
    assert all(_bits_equal(a, b) for a, b in zip(none, _result(m)))
    with pytest.raises(api.TsarError):
        m.get_plane_prior()                                          # no prior was installed
    assert not _bits_equal(none[0], got[0])
    # mutually exclusive with prior=; unknown settings are refused
    with pytest.raises(ValueError):
        api.run_geom_pass(m, d1, n1, maps, 2, prior=(d1, n1), build_prior=BUILD)
    with pytest.raises(ValueError):
        api.run_geom_pass(m, d1, n1, maps, 2, build_prior={"cells": 4})
    m.close()


def test_run_geom_pass_multiscale_builds_the_prior(pass_inputs):
    sc, imgs, d1, n1, maps = pass_inputs
    m = _matcher(sc, imgs, strict=False, seed=13)
    coarse = api.run_geom_pass_multiscale(m, d1, n1, maps, 1, 2, 2, build_prior=BUILD, prior_params=PRIOR_KW)
    got = _result(m)
    with pytest.raises(api.TsarError):
        coarse[0].get_plane_prior()                                  # the prior is on the full-resolution context only
    for c in coarse:
        c.close()
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    c = api.Matcher()
    c.pyramid_from(m)
    _by_hand(m, d1, n1, maps)
    c.geom_pyramid_from(m)
    c.pyramid_planes_from(m)
    c.pm_iterate(2)
    m.upsample_merge(c)
    m.pm_iterate(2)
    m.compute_disp()
    assert all(_bits_equal(a, b) for a, b in zip(got, _result(m)))
    c.close()
    m.close()
    # levels = 0 is run_geom_pass
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass_multiscale(m, d1, n1, maps, 0, 2, 2, build_prior=BUILD, prior_params=PRIOR_KW)
    a = _result(m)
    m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, d1, n1, maps, 2, build_prior=BUILD, prior_params=PRIOR_KW)
    assert all(_bits_equal(u, v) for u, v in zip(a, _result(m)))
    m.close()


# ---- 5. does what it is for ----------------------------------------------------------------------------------------------------------------
def test_built_prior_does_what_it_is_for():
    """Phase 1 (pm_init + 3 iterations, strict mode, box 11, seed 77 + view) on every view; view 0's depth checked at the defaults
    against the others' phase-1 maps; the builder on the kept depths with view 0's phase-1 cost as the score, cell 4; view 0 rerun with
    the built prior as test_prior_does_what_it_is_for reruns it with the ground-truth one.  The scene of that test (160 x 120, step 0.2)
    does not serve: the check at its defaults keeps nothing right of x = 144 there and 26 % of its constant-albedo pixels, and the built
    prior covers at most 0.79 of them whatever the cell, so this is the scene of test_check_does_what_it_is_for at a
    quarter of its size (200 x 144), with the same integer noise in {-1, 0, 1}.  Bars from the CPU simulation
    (tools/plane_prior_build_oracle_bars.py: control 0.6012 / 0.0358, built 0.7700 / 0.1283 textured / constant albedo, coverage of the
    constant-albedo pixels 0.8929), control plus half the simulated gain: textured >= control + 0.0844, constant albedo >= control + 0.0462;
    and the prior covers >= 0.85 of the constant-albedo pixels."""
    sc = synth.make_scene(200, 144, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True)
    rng = np.random.default_rng(3)
    imgs = []
    for im in sc.images:                                             # in view order
        a = im.numpy().astype(np.int64)
        imgs.append(np.clip(a + rng.integers(-1, 2, a.shape), 0, 255).astype(np.uint8))
    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()
    n = len(imgs)
    depth1, cost0 = [], None
    for k in range(n):
        iv, K, R, t, _ = _reorder(sc, imgs, k)
        m = _matcher(sc, iv, box=11, n_best=1, strict=True, seed=77 + k, K=K, R=R, t=t)
        m.pm_init()
        m.pm_iterate(3)
        if k == 0:
            cost0 = m.get_plane()[1].copy()
        m.compute_disp()
        depth1.append(m.get_result(("depth",))["depth"].copy())
        m.close()
    m = _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=77)
    m.set_geom_depths([None] + depth1[1:], weight=0.0)
    kept = m.geom_check(depth1[0], want=("depth",))["depth"]
    built = m.build_plane_prior(kept, cost0, cell=4)
    m.close()
    covered = float((built["level"][~tex] != 255).mean())

    def shares(d):
        ok = np.abs(d - gt) <= 1e-2 * gt
        return float(ok[tex].mean()), float(ok[~tex].mean())

    m = _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=77)
    m.set_plane_prior(built["depth"], built["normal"])
    m.pm_init()
    m.pm_iterate(3)
    m.compute_disp()
    b_tex, b_flat = shares(m.get_result(("depth",))["depth"])
    m.close()
    c_tex, c_flat = shares(depth1[0])
    print(f"check keeps {float((kept > 0).mean()):.4f}; prior covers {covered:.4f} of the constant-albedo pixels, levels "
          f"{sorted(np.unique(built['level']).tolist())}; within 1e-2 of ground truth, textured / constant albedo: control {c_tex:.4f} / "
          f"{c_flat:.4f}; built prior {b_tex:.4f} / {b_flat:.4f}")
    assert covered >= 0.85
    assert b_tex >= c_tex + 0.0844
    assert b_flat >= c_flat + 0.0462


# ---- 6. the command line: tsar_gipuma --all --geom_consistency --geom_build_prior[=CELL] ----------------------------------------------------
def _cli(*args, ok=True):
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out


def test_cli_geom_build_prior(tmp_path):
    sc = synth.make_scene(128, 96, 3, seed=68, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    vd = lambda k: root + f"APD/{k:08d}/"
    common = ["-mslp_folder", root, "-images_folder", root + "images/", "--iterations=3", "--blocksize=11", "--n_best=1", "--seed=7"]
    _cli(CLI, "--all", "--gpus=1", *common)
    geom = ["--all", "--gpus=1", *common, "--geom_consistency", "--geom_iterations=2"]
    _cli(CLI, *geom, "--force")
    plain_record = open(vd(0) + "TSAR_geom.txt").read()
    assert plain_record.count("\n") == 1 and "prior" not in plain_record
    plain_depth = tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb")
    build = [*geom, "--geom_build_prior=5", "--geom_build_prior_levels=3", "--geom_prior_weight_depth=0.2", "--geom_prior_angle_clip=20"]
    first = _cli(CLI, *build, "--force")
    assert first.stdout.count("(geom): ok") == n
    record = open(vd(0) + "TSAR_geom.txt").read()
    assert record == plain_record + "geom_build_prior=5 geom_build_prior_levels=3 geom_build_min_consistent=2 geom_build_reproj_error=2 " \
                                    "geom_build_depth_diff=0.00999999978 geom_prior_weight_depth=0.200000003 geom_prior_weight_normal=0.0500000007 " \
                                    "geom_prior_depth_clip=0.0199999996 geom_prior_angle_clip=20\n"
    assert not _bits_equal(plain_depth, tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb"))
    # bit for bit against api.run_geom_pass with the same settings
    for k in range(n):
        ids = [k] + [s for s in range(n) if s != k]
        imgs = [tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views(imgs, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), np.stack([c[2] for c in cams]), u8=True)
        src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
        api.run_geom_pass(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, 2,
                          build_prior={"cell": 5, "max_levels": 3}, prior_params={"weight_depth": 0.2, "angle_clip_deg": 20.0})
        r = m.get_result(("depth", "normal"))
        m.close()
        assert _bits_equal(r["depth"], tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb")), k
        assert _bits_equal(r["normal"], tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb")), k
    # a rerun skips; other settings recompute
    again = _cli(CLI, *build)
    assert again.stdout.count("geom outputs present, skipped") == n
    other = _cli(CLI, *geom, "--geom_build_prior")
    assert other.stdout.count("(geom): ok") == n and "geom_build_prior=4 geom_build_prior_levels=0 " in open(vd(0) + "TSAR_geom.txt").read()
    # refusals
    for args, message in (([*common, "--all", "--geom_build_prior"], "--geom_consistency"),
                          ([*geom, "--geom_build_prior", "--geom_plane_prior=PRIOR"], "mutually exclusive"),
                          ([*geom, "--geom_build_prior=1"], "2..256"), ([*geom, "--geom_build_prior=300"], "2..256"),
                          ([*geom, "--geom_build_prior", "--geom_build_prior_levels=17"], "0..16"),
                          ([*geom, "--geom_build_prior_levels=2"], "--geom_build_prior")):
        out = _cli(CLI, *args, ok=False)
        assert message in out.stdout + out.stderr, (args, out.stdout + out.stderr)
    # the same command without the switch: the record it always wrote
    _cli(CLI, *geom, "--force")
    assert open(vd(0) + "TSAR_geom.txt").read() == plain_record
    assert _bits_equal(plain_depth, tio.read_dmb(vd(0) + "TSAR_geom_disp.dmb"))

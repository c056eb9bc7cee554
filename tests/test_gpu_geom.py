"""Geometric-consistency PatchMatch (include/tsar.h tsar_set_geom_depths / tsar_clear_geom / tsar_pm_rescore): the term bit for bit
against the oracle's photometric per-view cost plus the numpy float32 restatement of the term (test_geom_cpu.py); weight 0 is the
photometric path; the memo and the packed form change no bit under the term; the stored cost is the plane's score after rescore; the
pass does what it is for on a synthetic scene; the error paths."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from test_geom_cpu import expected_cost_planes, geom_term
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def _u8(sc):
    return [im.numpy().astype(np.uint8) for im in sc.images]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _matcher(sc, imgs, box=11, n_best=1, strict=True, seed=5, K=None, R=None, t=None):
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=box, box_vsize=box, n_best=n_best, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV if strict else 0, seed=seed))
    m.set_views(imgs, sc.K if K is None else K, sc.R if R is None else R, sc.t if t is None else t, u8=True)
    return m


_RCP = {}


def _oracle(sc, imgs, box, n_best, strict, matcher):
    o = ol.Oracle([np.asarray(i, np.float32) for i in imgs], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=box, n_best=n_best, seed=5,
                  flags=0 if strict else ol.FLAGS_FAST_8BIT_IMAGERY)
    if not strict:
        if "t" not in _RCP:
            _RCP["t"] = ol.rcp_table_from_device(matcher)
        o.set_rcp_table(_RCP["t"])
    return o


def _gt_maps(sc, hole=True):
    """every view's ground-truth depth, with a block of 0 (no estimate) in each source map"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    if hole:
        h, w = maps[0].shape
        for v in range(1, len(maps)):
            maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
    return maps


def _test_planes(sc, m, maps, kind):
    """[h, w, 4] planes of one kind: ground truth, random (tsar_pm_init's), fronto-parallel ones whose point lands outside view 1,
    and fronto-parallel ones whose projection into view 1 falls within 4e-4 px of a rounding boundary of step 3"""
    h, w = sc.gt_depth.shape
    if kind == "gt":
        return np.ascontiguousarray(synth.gt_planes(sc).numpy())
    if kind == "random":
        m.pm_init()
        return m.get_plane()[0]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = np.zeros((h, w, 4), F32)
    planes[..., 2] = -1.0                                    # n = (0, 0, -1): the plane's depth is d at every pixel
    if kind == "outside":
        planes[..., 3] = F32(sc.depth_min) * F32(0.05)       # very near: the point projects far off view 1's image
        return planes
    F, _ = m.get_geom_matrices(1)
    F = F.astype(np.float64)
    gt = sc.gt_depth.numpy().astype(np.float64)
    al = F[0, 0] * xs + F[0, 1] * ys + F[0, 2]
    ga = F[2, 0] * xs + F[2, 1] * ys + F[2, 2]
    u = (al * gt + F[0, 3]) / (ga * gt + F[2, 3])
    delta = np.where((xs + ys) % 2 == 0, 4e-4, -4e-4)
    target = np.floor(u) + 0.5 + delta                       # u(D) = (al D + b0) / (ga D + b2) = target
    D = (F[2, 3] * target - F[0, 3]) / (al - ga * target)
    planes[..., 3] = D.astype(F32)
    return planes


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("box", [11, 19])
@pytest.mark.parametrize("n_best", [1, 2])
@pytest.mark.parametrize("kind", ["gt", "random", "outside", "boundary"])
def test_term_is_the_restatement_bit_for_bit(strict, box, n_best, kind):
    sc = synth.make_scene(64, 48, 3, seed=61, all_gt=True)
    imgs = _u8(sc)
    m = _matcher(sc, imgs, box=box, n_best=n_best, strict=strict)
    maps = _gt_maps(sc)
    maps[0] = None
    planes = _test_planes(sc, m, maps, kind)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    cost, bv, rt = m.pm_cost_planes(planes)
    orc = _oracle(sc, imgs, box, n_best, strict, m)
    ec, ebv, ert = expected_cost_planes(orc, [None] + [m.get_geom_matrices(v) for v in range(1, len(maps))], maps, planes, n_best, 0.2, 3.0)
    assert _bits_equal(cost, ec), (kind, int((cost.view(np.uint32) != ec.view(np.uint32)).sum()))
    assert np.array_equal(bv, ebv)
    assert _bits_equal(rt, ert)
    # the term is not idle: the same planes score differently without it
    m.clear_geom()
    c0, _, _ = m.pm_cost_planes(planes)
    assert not _bits_equal(c0, cost)
    m.close()


def _run(sc, maps, weight, strict, iters=4, env=None, per_call=False, timing=False):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m = _matcher(sc, _u8(sc), strict=strict, seed=9)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if timing:
        m.enable_kernel_timing(True)
    if maps is not None:
        m.set_geom_depths(maps, weight=weight)
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


def _same(a, b):
    for u, v in zip(a, b):
        assert _bits_equal(u, v)


@pytest.mark.parametrize("strict", [True, False])
def test_weight_zero_is_the_photometric_path(strict):
    sc = synth.make_scene(160, 120, 3, seed=62, all_gt=True)
    maps = _gt_maps(sc)
    a, _ = _run(sc, None, 0.0, strict)
    b, t = _run(sc, maps, 0.0, strict, timing=True)
    _same(a, b)
    assert "pm_sweep_geom" in t and "pm_sweep" not in t       # (every sweep ran the kernels with the term)


@pytest.mark.parametrize("strict", [True, False])
def test_memo_and_packed_form_change_no_bit_under_geometry(strict):
    sc = synth.make_scene(333, 251, 4, seed=63, all_gt=True)
    maps = _gt_maps(sc)
    iters = 6
    plain, t = _run(sc, maps, 0.2, strict, iters, {"TSAR_MEMO": "0"}, timing=True)
    assert "pm_sweep_packed" not in t                           # (no memo: no packed form either)
    early, t = _run(sc, maps, 0.2, strict, iters, {"TSAR_COMPACT_FROM": "2"}, timing=True)
    assert "pm_sweep_packed" in t
    rolled, t = _run(sc, maps, 0.2, strict, iters, {"TSAR_COMPACT_FROM": "-1"}, timing=True)
    assert "pm_sweep_packed" not in t
    calls, _ = _run(sc, maps, 0.2, strict, iters, {}, per_call=True)
    _same(plain, early)
    _same(plain, rolled)
    _same(plain, calls)
    photometric, _ = _run(sc, None, 0.2, strict, iters)
    assert not _bits_equal(plain[0], photometric[0])           # the term changed the result


@pytest.mark.parametrize("strict", [True, False])
def test_stored_cost_is_the_planes_score_after_rescore(strict):
    sc = synth.make_scene(160, 120, 3, seed=64, all_gt=True)
    m = _matcher(sc, _u8(sc), strict=strict, seed=11)
    m.enable_kernel_timing(True)
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[40:60, 50:90] = 0                                    # no estimate here: rescore must draw valid hypotheses
    R0 = np.asarray(sc.R[0], np.float64)
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ R0).astype(F32)    # camera -> world: R^T n
    m.load_planes(depth, normal_world)
    m.set_geom_depths(_gt_maps(sc), weight=0.2)
    m.rescore()
    planes, c, bv, rt = m.get_plane()
    cc, cbv, crt = m.pm_cost_planes(planes)
    assert _bits_equal(c, cc) and np.array_equal(bv, cbv) and _bits_equal(rt, crt)
    orc = ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max)
    for y in range(40, 60, 3):
        for x in range(50, 90, 3):
            d = orc.depth_from_plane(planes[y, x], x, y)
            assert sc.depth_min <= d <= sc.depth_max, (x, y, d)
    m.pm_iterate(3)
    planes, c, _, _ = m.get_plane()
    cc, _, _ = m.pm_cost_planes(planes)
    assert _bits_equal(c, cc)
    t = m.kernel_timing()
    assert "pm_rescore" in t and "pm_sweep_geom" in t
    m.close()


def _reorder(sc, imgs, k):
    order = [k] + [v for v in range(len(imgs)) if v != k]
    return [imgs[v] for v in order], sc.K[order], sc.R[order], sc.t[order], order


def test_geometric_pass_does_what_it_is_for():
    """Phase 1 (photometric) on every view of a textureless scene, phase 2 on view 0.  Bars stated before measuring: the share of
    view-0 pixels that reproject within 1 px onto >= 2 sources' phase-1 maps rises; the textured pixels' share within 1e-3 relative
    depth of ground truth drops by at most 0.5 points."""
    sc = synth.make_scene(192, 144, 5, seed=65, all_gt=True, textureless=True)
    imgs = _u8(sc)
    n = len(imgs)
    depth1, normal1 = [], []
    for k in range(n):
        iv, K, R, t, _ = _reorder(sc, imgs, k)
        m = _matcher(sc, iv, strict=False, seed=13, K=K, R=R, t=t)
        m.pm_init()
        m.pm_iterate(6)
        m.compute_disp()
        r = m.get_result(("depth", "normal"))
        depth1.append(r["depth"].copy())
        normal1.append(r["normal"].copy())
        m.close()
    m = _matcher(sc, imgs, strict=False, seed=13)
    api.run_geom_pass(m, depth1[0], normal1[0], [None] + depth1[1:], 2)
    depth2 = m.get_result(("depth",))["depth"].copy()
    h, w = depth2.shape
    ys, xs = np.mgrid[0:h, 0:w]

    def agree(D):
        cnt = np.zeros((h, w), np.int32)
        for v in range(1, n):
            F, B = m.get_geom_matrices(v)
            cnt += geom_term(F, B, depth1[v], xs, ys, D.astype(F32), 1.0, 3.0) < 1.0
        return float(((cnt >= 2) & (D > 0)).mean())

    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()
    rel = lambda D: np.abs(D - gt) / gt
    a1, a2 = agree(depth1[0]), agree(depth2)
    t1, t2 = float((rel(depth1[0])[tex] < 1e-3).mean()), float((rel(depth2)[tex] < 1e-3).mean())
    med1, med2 = float(np.median(rel(depth1[0])[~tex])), float(np.median(rel(depth2)[~tex]))
    print(f"reprojection agreement {a1:.4f} -> {a2:.4f}; textured within 1e-3 {t1:.4f} -> {t2:.4f}; textureless median rel. error "
          f"{med1:.4f} -> {med2:.4f}")
    assert a2 > a1
    assert t2 >= t1 - 0.005
    m.close()


@pytest.mark.parametrize("strict", [True, False])
def test_device_matrices_are_the_float64_geometry(strict):
    """the matrices the kernels read (derive_cameras) against the independent float64 formation of test_geom_cpu.py, each entry
    rounded once to float32: within one float32 ulp, or 1e-7 of the row's largest entry for entries that come out of cancellation
    (the two float64 formations differ in their last bits); a transposed rotation or a wrong sign is off by far more"""
    from test_geom_cpu import matrices64
    sc = synth.make_scene(64, 48, 3, seed=67)
    m = _matcher(sc, _u8(sc), strict=strict)
    for v in range(3):
        F, B = m.get_geom_matrices(v)
        F64, B64 = matrices64(sc.K, sc.R, sc.t, v)
        for got, want in ((F, F64), (B, B64)):
            ref = want.astype(F32)
            tol = np.maximum(np.spacing(np.abs(ref)), 1e-7 * np.abs(ref).max(axis=1, keepdims=True))
            assert np.all(np.abs(got.astype(np.float64) - ref) <= tol), (v, got, ref)
    m.close()


def test_error_paths():
    sc = synth.make_scene(64, 48, 2, seed=66, all_gt=True)
    imgs = _u8(sc)
    maps = _gt_maps(sc)
    m = _matcher(sc, imgs)
    for kw in ({"weight": -0.1}, {"clip": 0.0}, {"clip": -1.0}, {"weight": float("nan")}):
        with pytest.raises(api.TsarError) as e:
            m.set_geom_depths(maps, **kw)
        assert e.value.code == api.TSAR_ERR_INVALID
    rc = m.L.tsar_set_geom_depths(m._ctx, 2, None, api.MEM_HOST, 0.2, 3.0)   # wrong number of views / NULL
    assert rc != api.TSAR_OK
    m.set_geom_depths(maps)
    c = api.Matcher()
    with pytest.raises(api.TsarError) as e:
        c.pyramid_from(m)                                        # coarse-to-fine with the term: refused
    assert e.value.code == api.TSAR_ERR_STATE
    m.clear_geom()
    c.pyramid_from(m)
    c.pm_init()
    m.set_geom_depths(maps)
    with pytest.raises(api.TsarError) as e:
        m.upsample_planes(c)
    assert e.value.code == api.TSAR_ERR_STATE
    m.clear_geom()
    m.upsample_planes(c)
    c.close()
    m.close()
    only = _matcher(sc, imgs[:1], K=sc.K[:1], R=sc.R[:1], t=sc.t[:1])
    with pytest.raises(api.TsarError) as e:
        only.set_geom_depths([None])
    assert e.value.code == api.TSAR_ERR_STATE
    only.close()


# ---- the CLI: tsar_gipuma --all --geom_consistency, tsar_fusion --geom ------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")
FUSION = os.path.join(ROOT, "tsar-mvs_amd", "tsar_fusion")


def _cli(*args, ok=True):
    import subprocess
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    if ok:
        assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_cli_geom_consistency(tmp_path):
    from tsar_mvs_amd import io as tio
    sc = synth.make_scene(128, 96, 3, seed=68, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    common = ["-mslp_folder", root, "-images_folder", root + "images/", "--iterations=3", "--blocksize=11", "--n_best=1", "--seed=7"]
    geom = ["--all", "--gpus=1", *common, "--geom_consistency", "--geom_iterations=2"]
    first = _cli(CLI, *geom)
    assert first.stdout.count("(geom): ok") == n
    vd = lambda k: root + f"APD/{k:08d}/"
    for k in range(n):
        for f in ("TSAR_geom_disp.dmb", "TSAR_geom_normals.dmb", "TSAR_geom.txt", "TSAR_disp.dmb"):
            assert os.path.exists(vd(k) + f), f
    # bit for bit against api.run_geom_pass on the same files, the same seed (the CLI's seed + view id) and settings
    for k in range(n):
        ids = [k] + [s for s in range(n) if s != k]
        imgs = [tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views(imgs, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), np.stack([c[2] for c in cams]), u8=True)
        src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
        api.run_geom_pass(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, 2)
        r = m.get_result(("depth", "normal"))
        m.close()
        assert _bits_equal(r["depth"], tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb")), k
        assert _bits_equal(r["normal"], tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb")), k
    # resume: nothing is recomputed; a changed --geom_weight recomputes phase 2 only; --force recomputes both phases
    again = _cli(CLI, *geom)
    assert again.stdout.count("geom outputs present, skipped") == n and again.stdout.count("outputs present, skipped") == 2 * n
    other = _cli(CLI, *geom, "--geom_weight=0.3")
    assert "geom outputs present" not in other.stdout and other.stdout.count("(geom): ok") == n
    assert "geom_weight=0.3" in open(vd(0) + "TSAR_geom.txt").read()
    forced = _cli(CLI, *geom, "--geom_weight=0.3", "--force")
    assert "skipped" not in forced.stdout and forced.stdout.count("(geom): ok") == n
    # a newer phase-1 map of a source voids the views that read it
    os.utime(vd(1) + "TSAR_disp.dmb")
    newer = _cli(CLI, *geom, "--geom_weight=0.3")
    assert newer.stdout.count("(geom): ok") == n                     # (every view has view 1 among its sources)
    # refusals
    names = [f"{k:08d}.pgm" for k in range(n)]
    assert _cli(CLI, *names, *common, "--geom_consistency", ok=False).returncode != 0                      # without --all
    assert _cli(CLI, "--all", *common, "--geom_consistency", "--mode=tsar", ok=False).returncode != 0      # with --mode=tsar
    assert _cli(CLI, "--all", *common, "--geom_consistency", "--geom_clip=0", ok=False).returncode != 0
    # fusion of the geom maps: tsar_fusion --geom, and tsar_gipuma --fuse with the pass
    ply = root + "APD/APD_TSAR.ply"
    _cli(FUSION, root, "--geom")
    geom_cloud = open(ply, "rb").read()
    _cli(FUSION, root)
    assert open(ply, "rb").read() != geom_cloud                      # (the photometric maps make another cloud)
    _cli(CLI, *geom, "--geom_weight=0.3", "--fuse")
    assert open(ply, "rb").read() == geom_cloud
    os.rename(vd(2) + "TSAR_geom_disp.dmb", vd(2) + "moved.dmb")
    assert _cli(FUSION, root, "--geom", ok=False).returncode != 0     # --geom reads the geom maps, not the others

"""The geometric-consistency check on the GPU (include/tsar.h tsar_geom_check, Matcher.geom_check, tsar_gipuma --consistency_filter): count,
filtered depth and mask bit for bit against the numpy float32 restatement (test_geom_check_cpu.geom_check_ref), in host and device memory,
in strict and fast contexts; depth=None; the call moves nothing else in the context; the error codes; the check does what it is for on
a textureless scene; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_geom_check_cpu import geom_check_ref
from test_gpu_geom import _bits_equal, _gt_maps, _matcher, _reorder, _test_planes, _u8
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")

SHAPES = [(64, 48, 3), (101, 67, 4)]        # the second: odd in both directions, partial tiles in x and in y, two blocks along x
_CASES = {}


def _case(shape):
    """per shape, built once: the scene, a strict and a fast context holding its views, the ground-truth maps with their holes, and the
    matrices the kernels read"""
    if shape not in _CASES:
        sc = synth.make_scene(*shape, seed=94, all_gt=True)
        imgs = _u8(sc)
        ms = {strict: _matcher(sc, imgs, strict=strict) for strict in (True, False)}
        maps = _gt_maps(sc)
        maps[0] = None
        n = len(maps)
        FB = [ms[True].get_geom_matrices(v) for v in range(n)]
        for v in range(n):                                      # both contexts hold the same matrices
            assert all(_bits_equal(a, b) for a, b in zip(FB[v], ms[False].get_geom_matrices(v)))
        _CASES[shape] = (sc, ms, maps, [fb[0] for fb in FB], [fb[1] for fb in FB])
    return _CASES[shape]


def _depths(sc, m, maps, kind):
    """the reference view's map to check, of one kind"""
    gt = sc.gt_depth.numpy().astype(F32)
    h, w = gt.shape
    ys, xs = np.mgrid[0:h, 0:w]
    if kind in ("gt", "no_map"):
        return gt.copy()
    if kind in ("boundary", "outside"):                         # fronto-parallel planes n = (0, 0, -1): the depth is d at every pixel
        return np.ascontiguousarray(_test_planes(sc, m, maps, kind)[..., 3])
    if kind == "depth_diff_edge":                               # around the depth_diff = 0.01 edge, both ways, side by side
        scale = np.choose((xs + 2 * ys) % 4, [F32(1.009), F32(0.991), F32(1.011), F32(0.989)]).astype(F32)
        return (gt * scale).astype(F32)
    assert kind == "non_candidates"
    rng = np.random.default_rng(7)
    d = gt.copy()
    pick = rng.integers(0, 12, (h, w))
    for k, val in enumerate([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf]):
        d[pick == k] = val
    return d


KINDS = ["gt", "no_map", "boundary", "outside", "depth_diff_edge", "non_candidates"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_n%d" % s)
def test_check_is_the_restatement_bit_for_bit(shape, kind):
    import torch
    sc, ms, maps, F, B = _case(shape)
    n = len(maps)
    maps = list(maps)
    if kind == "no_map":
        maps[2] = None
    depth = _depths(sc, ms[True], maps, kind)
    for m in ms.values():
        m.set_geom_depths(maps, weight=0.0)                     # installed for checking only
    seen = set()
    for k in (1, 2, n):                                         # (n: more than the n - 1 sources can give: nothing is kept)
        params = (2.0, 0.01, k)
        count, filtered, mask = geom_check_ref(F, B, maps, depth, params)
        seen.update(np.unique(count).tolist())
        for strict, m in ms.items():
            r = m.geom_check(depth, *params)
            assert r["count"].dtype == np.uint8 and np.array_equal(r["count"], count), (kind, k, strict, int((r["count"] != count).sum()))
            assert _bits_equal(r["depth"], filtered), (kind, k, strict)
            assert _bits_equal(m.get_reliable_mask(), mask), (kind, k, strict)
            dev = m.geom_check(torch.from_numpy(depth).cuda(), *params)
            assert dev["count"].is_cuda and dev["depth"].is_cuda and dev["count"].dtype == torch.uint8
            assert np.array_equal(dev["count"].cpu().numpy(), count) and _bits_equal(dev["depth"].cpu().numpy(), filtered)
            assert _bits_equal(m.get_reliable_mask(), mask)
            only = m.geom_check(depth, *params, want=("count",))
            assert set(only) == {"count"} and np.array_equal(only["count"], count)
        if k == n:
            assert not mask.any() and not filtered.any()
    # the inputs exercise what they are there for
    if kind == "gt":
        assert max(seen) == n - 1 and 0 in seen                  # every source agrees somewhere; the holes and the borders drop some
    if kind == "no_map":
        assert max(seen) == n - 2
    if kind == "outside":
        assert seen == {0}
    if kind in ("boundary", "depth_diff_edge"):
        assert len(seen) >= 2
    if kind == "non_candidates":
        bad = ~((depth > 0) & np.isfinite(depth))
        assert bad.mean() > 0.3 and np.all(geom_check_ref(F, B, maps, depth, (2.0, 0.01, 1))[0][bad] == 0)


def test_other_thresholds_bit_for_bit():
    """reproj_error and depth_diff away from their defaults, down to where they cut into ground truth (the nearest-pixel rounding of
    the chain leaves up to ~0.7 px of reprojection error on true depths)"""
    sc, ms, maps, F, B = _case(SHAPES[1])
    depth = _depths(sc, ms[True], maps, "gt")
    for m in ms.values():
        m.set_geom_depths(maps, weight=0.0)
    kept = []
    for params in ((0.3, 0.01, 1), (0.5, 0.001, 2), (1048576.0, 0.5, 3), (2.0, 1e-4, 1)):
        count, filtered, mask = geom_check_ref(F, B, maps, depth, params)
        kept.append(float(mask.mean()))
        for m in ms.values():
            r = m.geom_check(depth, *params)
            assert np.array_equal(r["count"], count) and _bits_equal(r["depth"], filtered) and _bits_equal(m.get_reliable_mask(), mask)
    # (the tighter bounds cut into ground truth: they are not idle)
    loose = float(geom_check_ref(F, B, maps, depth, (2.0, 0.01, 1))[2].mean())
    assert 0 < kept[0] < loose and 0 < kept[3] < loose


def test_depth_none_is_the_contexts_own_result():
    sc, ms, maps, F, B = _case(SHAPES[1])
    m = _matcher(sc, _u8(sc), strict=False, seed=21)
    m.pm_init()
    m.pm_iterate(1)
    m.set_geom_depths(maps, weight=0.0)
    with pytest.raises(api.TsarError) as e:                       # no result yet
        m.geom_check()
    assert e.value.code == api.TSAR_ERR_STATE
    m.compute_disp()
    own = m.get_result(("depth",))["depth"]
    a = m.geom_check()
    mask_a = m.get_reliable_mask()
    b = m.geom_check(own)
    assert np.array_equal(a["count"], b["count"]) and _bits_equal(a["depth"], b["depth"]) and _bits_equal(mask_a, m.get_reliable_mask())
    count, filtered, mask = geom_check_ref(F, B, maps, own, (2.0, 0.01, 2))
    assert np.array_equal(a["count"], count) and _bits_equal(a["depth"], filtered) and _bits_equal(mask_a, mask)
    m.close()


def test_filtering_a_device_map_in_place():
    """depth_out may be `depth` itself (include/tsar.h): a map on the device filtered where it lies, host memory too"""
    import torch
    sc, ms, maps, F, B = _case(SHAPES[1])
    depth = _depths(sc, ms[True], maps, "depth_diff_edge")
    m = ms[False]
    m.set_geom_depths(maps, weight=0.0)
    count, filtered, mask = geom_check_ref(F, B, maps, depth, (2.0, 0.01, 2))
    assert 0 < mask.mean() < 1
    p = api.GeomCheckParams(2.0, 0.01, 2)
    d = torch.from_numpy(depth.copy()).cuda()
    m._chk(m.L.tsar_geom_check(m._ctx, C.c_void_p(d.data_ptr()), C.byref(p), None, C.c_void_p(d.data_ptr()), api.MEM_DEVICE))
    assert _bits_equal(d.cpu().numpy(), filtered) and _bits_equal(m.get_reliable_mask(), mask)
    hd = depth.copy()
    m._chk(m.L.tsar_geom_check(m._ctx, hd.ctypes.data_as(C.c_void_p), C.byref(p), None, hd.ctypes.data_as(C.c_void_p), api.MEM_HOST))
    assert _bits_equal(hd, filtered)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("env,form", [({"TSAR_COMPACT_FROM": "-1"}, "memo"), ({"TSAR_COMPACT_FROM": "2"}, "packed"), ({"TSAR_BLOCK": "256"}, "block256")])
def test_nothing_else_moves(env, form):
    """planes, costs, best views, ratios and the result are bit-identical before and after the call, and the sweeps that follow it — the
    memo, the packed form, the sweep counter and the term they read — equal those of a context that never made it"""
    sc, _, maps, _, _ = _case(SHAPES[1])
    gt = sc.gt_depth.numpy().astype(F32)

    def run(check):
        # (the knobs are read by tsar_create; the forced workgroup shape applies to the two-best-views kernels)
        m = _with_env(env, lambda: _matcher(sc, _u8(sc), n_best=2 if form == "block256" else 1, strict=False, seed=9))
        m.enable_kernel_timing(True)
        m.set_geom_depths(maps, weight=0.2)
        m.pm_init()
        m.pm_iterate(2)
        m.compute_disp()
        if check:
            before, res0 = m.get_plane(), m.get_result()
            m.geom_check(gt)
            m.geom_check()
            after, res1 = m.get_plane(), m.get_result()
            assert all(_bits_equal(a, b) for a, b in zip(before, after))
            assert all(_bits_equal(res0[k], res1[k]) for k in res0)
            assert m.kernel_timing()["geom_check"][0] == 2
        m.pm_iterate(2)
        state, t = m.get_plane(), m.kernel_timing()
        m.close()
        return state, t

    (with_check, t1), (without, t0) = run(True), run(False)
    assert all(_bits_equal(a, b) for a, b in zip(with_check, without))
    assert ("pm_sweep_packed" in t1) == (form == "packed") and "geom_check" not in t0
    # (the check launched no sweep and no rescore of its own)
    sweeps = lambda t: {k: v[0] for k, v in t.items() if k.startswith("pm_")}
    assert sweeps(t1) == sweeps(t0) and sweeps(t0)["pm_sweep_geom"] == 8


def test_error_codes():
    sc, ms, maps, _, _ = _case(SHAPES[0])
    gt = sc.gt_depth.numpy().astype(F32)
    m = ms[True]
    m.clear_geom()
    with pytest.raises(api.TsarError) as e:
        m.geom_check(gt)
    assert e.value.code == api.TSAR_ERR_STATE                   # no term installed
    m.set_geom_depths(maps, weight=0.0)
    out = np.empty_like(gt)
    assert m.L.tsar_geom_check(m._ctx, gt.ctypes.data_as(C.c_void_p), None, None, out.ctypes.data_as(C.c_void_p), api.MEM_HOST) == api.TSAR_ERR_INVALID
    bad = [{"reproj_error": 0.0}, {"reproj_error": -1.0}, {"reproj_error": float("nan")}, {"reproj_error": float("inf")}, {"reproj_error": 2.0 ** 20 + 1},
           {"depth_diff": 0.0}, {"depth_diff": -0.01}, {"depth_diff": float("nan")}, {"depth_diff": float("inf")},
           {"min_consistent": 0}, {"min_consistent": 32}, {"min_consistent": -2}]
    for kw in bad:
        with pytest.raises(api.TsarError) as e:
            m.geom_check(gt, **kw)
        assert e.value.code == api.TSAR_ERR_INVALID, kw
    m.geom_check(gt, reproj_error=2.0 ** 20, min_consistent=31)  # the ends of the ranges are inside
    m.geom_check(gt, min_consistent=1)
    p = api.GeomCheckParams()
    m.L.tsar_default_geom_check_params(C.byref(p))
    assert (p.reproj_error, p.min_consistent) == (2.0, 2) and F32(p.depth_diff) == F32(0.01)
    f = api.FusionParams()
    m.L.tsar_default_fusion_params(C.byref(f))
    assert (p.reproj_error, p.depth_diff) == (f.reproj_error, f.depth_diff)
    with pytest.raises(api.TsarError) as e:                       # depth = NULL without a result
        m.geom_check()
    assert e.value.code == api.TSAR_ERR_STATE


def test_check_does_what_it_is_for():
    """Phase 1 on every view of a textureless scene in strict arithmetic, then view 0 checked against the three sources' maps at the
    defaults.  Bars from the CPU oracle in strict arithmetic, which the strict kernels reproduce bit for bit (measured there: 99.67 %,
    93.1 %, 1.8 %, 11.8 %)."""
    sc = synth.make_scene(800, 576, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True)
    imgs = _u8(sc)
    n = len(imgs)
    depth1 = []
    for k in range(n):
        iv, K, R, t, _ = _reorder(sc, imgs, k)
        m = _matcher(sc, iv, box=11, n_best=1, strict=True, seed=41 + k, K=K, R=R, t=t)
        m.pm_init()
        m.pm_iterate(3)
        m.compute_disp()
        depth1.append(m.get_result(("depth",))["depth"].copy())
        m.close()
    m = _matcher(sc, imgs, strict=True, seed=41)
    m.set_geom_depths([None] + depth1[1:], weight=0.0)
    r = m.geom_check(depth1[0])
    keep = m.get_reliable_mask() == 1
    m.close()
    assert np.array_equal(keep, r["count"] >= 2) and np.array_equal(keep, r["depth"] > 0)
    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()
    good = np.abs(depth1[0] - gt) / gt < 1e-2
    kept_good = float(good[keep].mean())
    tex_kept = float(keep[tex].mean())
    flat_kept = float(keep[~tex].mean())
    dropped_good = float(good[~keep].mean())
    print(f"kept pixels within 1e-2 of ground truth {kept_good:.4f}; textured pixels kept {tex_kept:.4f}; constant-albedo pixels kept "
          f"{flat_kept:.4f}; dropped pixels within 1e-2 of ground truth {dropped_good:.4f}")
    assert kept_good >= 0.99
    assert tex_kept >= 0.90
    assert flat_kept <= 0.05
    assert dropped_good <= 0.25


# ---- the command line: tsar_gipuma --all --consistency_filter ------------------------------------------------------------------------
def _cli(*args):
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_cli_consistency_filter(tmp_path):
    sc = synth.make_scene(96, 72, 2, seed=69, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    pairs = tio.read_pairs(root + "pair.txt")
    vd = lambda k: root + f"APD/{k:08d}/"
    base = [CLI, "--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=2", "--blocksize=11", "--n_best=1", "--seed=7"]

    def expect(k, maps_name, min_consistent):
        """Matcher.geom_check on the files the CLI read for view k"""
        ids = [k] + [s for s, _ in pairs[k]]
        cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
        m.set_views([tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids], np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]),
                    np.stack([c[2] for c in cams]), u8=True)
        m.set_geom_depths([None] + [tio.read_dmb(vd(i) + maps_name) for i in ids[1:]], weight=0.0)
        r = m.geom_check(tio.read_dmb(vd(k) + maps_name), min_consistent=min_consistent)
        mask = m.get_reliable_mask()
        m.close()
        return r["depth"], mask

    def compare(maps_name, min_consistent):
        total = 0
        for k in range(n):
            want, mask = expect(k, maps_name, min_consistent)
            assert _bits_equal(tio.read_dmb(vd(k) + "TSAR_filtered_disp.dmb"), want), k
            ones = int((mask == 1).sum())
            chk = _cli(CLI, "--check-mask=" + vd(k) + "TSAR_consistent.png")
            checksum = int((np.flatnonzero(mask.ravel() == 1) % 9973).sum())
            assert chk.stdout.strip() == f"mask {sc.w} x {sc.h} reliable {ones} checksum {checksum}", k
            rec = open(vd(k) + "TSAR_filter.txt").read()
            assert f"min_consistent={min_consistent} reproj_error=2 depth_diff=0.00999999978 " in rec and f"checked={maps_name} " in rec
            total += ones
        return total

    first = _cli(*base, "--consistency_filter")
    assert first.stdout.count("(filter): ok") == n and "(geom)" not in first.stdout
    kept2 = compare("TSAR_disp.dmb", 2)
    # a rerun skips every view of both phases; another K recomputes the filter only
    again = _cli(*base, "--consistency_filter")
    assert again.stdout.count("filter outputs present, skipped") == n and again.stdout.count("outputs present, skipped") == 2 * n
    other = _cli(*base, "--consistency_filter=1")
    assert "filter outputs present" not in other.stdout and other.stdout.count("(filter): ok") == n
    kept1 = compare("TSAR_disp.dmb", 1)
    assert kept1 >= kept2 > 0
    # with the geometric-consistency pass the filter checks that pass's maps against its sources' maps of that pass
    geom = _cli(*base, "--geom_consistency", "--geom_iterations=1", "--consistency_filter=1")
    assert geom.stdout.count("(geom): ok") == n and geom.stdout.count("(filter): ok") == n
    compare("TSAR_geom_disp.dmb", 1)
    # a newer input map voids the views that read it
    os.utime(vd(1) + "TSAR_geom_disp.dmb")
    newer = _cli(*base, "--geom_consistency", "--geom_iterations=1", "--consistency_filter=1")
    assert newer.stdout.count("(filter): ok") == n               # (every view has view 1 among its maps)

"""The cross-view depth render and its offer to the matcher on the GPU (include/tsar.h tsar_geom_reproject / tsar_pm_merge_depths,
Matcher.geom_reproject / merge_depths, run_geom_pass(cross_view=), tsar_gipuma --geom_cross_view): the render bit for bit against the numpy
float32 restatement (test_geom_reproject_cpu.reproject_ref) in host and device memory, strict and fast contexts; the call moves nothing in
the context; the error codes; the merge bit for bit against the composition of existing entries it is defined as; a merge that offers
nothing is rescore(); the Python pass; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from test_geom_reproject_cpu import layered, reproject_ref, support_edge
from test_gpu_geom import _bits_equal, _gt_maps, _matcher, _reorder, _u8
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
    back-projections the kernels read"""
    if shape not in _CASES:
        sc = synth.make_scene(*shape, seed=94, all_gt=True)
        imgs = _u8(sc)
        ms = {strict: _matcher(sc, imgs, strict=strict) for strict in (True, False)}
        maps = _gt_maps(sc)
        maps[0] = None
        n = len(maps)
        B = [ms[True].get_geom_matrices(v)[1] for v in range(n)]
        for v in range(n):                                      # both contexts hold the same matrices
            assert _bits_equal(B[v], ms[False].get_geom_matrices(v)[1])
        _CASES[shape] = (sc, ms, maps, B)
    return _CASES[shape]


def _source_maps(maps, kind, sc=None):
    maps = list(maps)
    if kind == "gt":
        return maps
    if kind == "no_map":
        maps[2] = None
        return maps
    if kind == "layered":                                       # on the maps without holes: the share of pixels with two landings is stated for those
        return [None] + layered(_gt_maps(sc, hole=False))[1:]
    if kind == "support_edge":
        return [None] + support_edge(maps)[1:]
    assert kind == "non_candidates"
    rng = np.random.default_rng(7)
    out = [None]
    for m in maps[1:]:
        d = m.copy()
        pick = rng.integers(0, 18, d.shape)
        for k, val in enumerate([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf]):
            d[pick == k] = val
        out.append(d)
    return out


KINDS = ["gt", "no_map", "layered", "support_edge", "non_candidates"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_n%d" % s)
def test_render_is_the_restatement_bit_for_bit(shape, kind):
    sc, ms, maps, B = _case(shape)
    n = len(maps)
    maps = _source_maps(maps, kind, sc)
    for m in ms.values():
        m.set_geom_depths(maps, weight=0.0)                     # installed for this call only
    seen = set()
    for k in (1, 2, n):                                         # (n: more than the n - 1 sources can give: nothing is kept)
        depth, count = reproject_ref(B, maps, 0.01, k)
        seen.update(np.unique(count).tolist())
        for strict, m in ms.items():
            r = m.geom_reproject(0.01, k)
            assert r["count"].dtype == np.uint8 and np.array_equal(r["count"], count), (kind, k, strict, int((r["count"] != count).sum()))
            assert _bits_equal(r["depth"], depth), (kind, k, strict, int((r["depth"].view(np.uint32) != depth.view(np.uint32)).sum()))
            dev = m.geom_reproject(0.01, k, device=True)
            assert dev["count"].is_cuda and dev["depth"].is_cuda and str(dev["count"].dtype) == "torch.uint8"
            assert np.array_equal(dev["count"].cpu().numpy(), count) and _bits_equal(dev["depth"].cpu().numpy(), depth)
            only = m.geom_reproject(0.01, k, want=("count",))
            assert set(only) == {"count"} and np.array_equal(only["count"], count)
            again = m.geom_reproject(0.01, k)                    # a minimum and a set: no dependence on the order of arrival
            assert _bits_equal(again["depth"], r["depth"]) and np.array_equal(again["count"], r["count"])
        if k == n:
            assert not depth.any()
    # the inputs exercise what they are there for
    if kind == "gt":
        assert max(seen) == n - 1 and 0 in seen
    if kind == "no_map":
        assert max(seen) == n - 2
    if kind == "support_edge":
        assert len(seen) >= 3
    if kind == "layered":
        hits = reproject_ref(B, maps, 0.01, 1, want_landings=True)[2]
        assert (hits >= 2).mean() >= 0.90
    if kind == "non_candidates":
        bad = np.mean([~((d > 0) & np.isfinite(d)) for d in maps[1:]])
        assert bad > 0.3


def test_other_depth_diffs_bit_for_bit():
    sc, ms, maps, B = _case(SHAPES[1])
    maps = _source_maps(maps, "support_edge")
    for m in ms.values():
        m.set_geom_depths(maps, weight=0.0)
    means = []
    for dd in (1e-4, 0.0095, 0.0205, 0.5):
        depth, count = reproject_ref(B, maps, dd, 2)
        means.append(float(count.mean()))
        for m in ms.values():
            r = m.geom_reproject(dd, 2)
            assert np.array_equal(r["count"], count) and _bits_equal(r["depth"], depth), dd
    assert means[0] < means[1] < means[2] <= means[3]            # (the bound is not idle)


def test_nothing_else_moves():
    """planes, costs, best views, ratios, the result and the reliable mask are bit-identical before and after the call, and the sweeps that
    follow it equal those of a context that never made it"""
    sc, _, maps, _ = _case(SHAPES[1])
    rng = np.random.default_rng(2)
    mask = (rng.random((sc.h, sc.w)) < 0.5).astype(F32)

    def run(call):
        m = _matcher(sc, _u8(sc), strict=False, seed=9)
        m.enable_kernel_timing(True)
        m.set_geom_depths(maps, weight=0.2)
        m.pm_init()
        m.pm_iterate(2)
        m.compute_disp()
        m.set_reliable_mask(mask)
        if call:
            before, res0 = m.get_plane(), m.get_result()
            m.geom_reproject()
            m.geom_reproject(0.02, 2, device=True)
            after, res1 = m.get_plane(), m.get_result()
            assert all(_bits_equal(a, b) for a, b in zip(before, after))
            assert all(_bits_equal(res0[k], res1[k]) for k in res0)
            assert _bits_equal(m.get_reliable_mask(), mask)
            assert m.kernel_timing()["geom_reproject"][0] == 6   # three launches per call
        m.pm_iterate(2)
        state, t = m.get_plane(), m.kernel_timing()
        m.close()
        return state, t

    (with_call, t1), (without, t0) = run(True), run(False)
    assert all(_bits_equal(a, b) for a, b in zip(with_call, without))
    assert "geom_reproject" not in t0
    sweeps = lambda t: {k: v[0] for k, v in t.items() if k.startswith("pm_")}
    assert sweeps(t1) == sweeps(t0) and sweeps(t0)["pm_sweep_geom"] == 8


def test_error_codes():
    sc, ms, maps, _ = _case(SHAPES[0])
    m = ms[True]
    m.clear_geom()
    with pytest.raises(api.TsarError) as e:
        m.geom_reproject()
    assert e.value.code == api.TSAR_ERR_STATE                   # no term installed
    m.set_geom_depths(maps, weight=0.0)
    out = np.empty((sc.h, sc.w), F32)
    outp = out.ctypes.data_as(C.c_void_p)
    p = api.GeomReprojectParams(0.01, 1)
    assert m.L.tsar_geom_reproject(m._ctx, None, outp, None, api.MEM_HOST) == api.TSAR_ERR_INVALID            # p NULL
    assert m.L.tsar_geom_reproject(m._ctx, C.byref(p), None, None, api.MEM_HOST) == api.TSAR_ERR_INVALID      # both outputs NULL
    assert m.L.tsar_geom_reproject(m._ctx, C.byref(p), outp, None, 7) == api.TSAR_ERR_INVALID                 # mem unknown
    assert m.L.tsar_geom_reproject(m._ctx, C.byref(p), outp, None, api.MEM_HOST) == api.TSAR_OK
    bad = [{"depth_diff": 0.0}, {"depth_diff": -0.01}, {"depth_diff": float("nan")}, {"depth_diff": float("inf")},
           {"min_views": 0}, {"min_views": 64}, {"min_views": -2}]
    for kw in bad:
        with pytest.raises(api.TsarError) as e:
            m.geom_reproject(**kw)
        assert e.value.code == api.TSAR_ERR_INVALID, kw
    m.geom_reproject(min_views=1)                               # the ends of the range are inside
    assert not m.geom_reproject(min_views=63)["depth"].any()
    d = api.GeomReprojectParams()
    m.L.tsar_default_geom_reproject_params(C.byref(d))
    assert d.min_views == 1 and F32(d.depth_diff) == F32(0.01)
    # tsar_pm_merge_depths: NULL depth, unknown mem; no plane state
    f = ms[False]
    f.pm_init()
    assert f.L.tsar_pm_merge_depths(f._ctx, None, api.MEM_HOST, None) == api.TSAR_ERR_INVALID
    assert f.L.tsar_pm_merge_depths(f._ctx, outp, 7, None) == api.TSAR_ERR_INVALID
    fresh = _matcher(sc, _u8(sc), strict=False)
    with pytest.raises(api.TsarError) as e:
        fresh.merge_depths(np.zeros((sc.h, sc.w), F32))
    assert e.value.code == api.TSAR_ERR_STATE
    fresh.close()
    only = _matcher(sc, _u8(sc)[:1], K=sc.K[:1], R=sc.R[:1], t=sc.t[:1])
    with pytest.raises(api.TsarError) as e:                      # the reference view alone: nothing to score against
        only.merge_depths(np.zeros((sc.h, sc.w), F32))
    assert e.value.code == api.TSAR_ERR_STATE
    only.close()


def _offered_depth(sc, B, maps):
    """the ground-truth render with unusable values sprinkled in"""
    depth = reproject_ref(B, maps, 0.01, 1)[0].copy()
    rng = np.random.default_rng(11)
    pick = rng.integers(0, 20, depth.shape)
    for k, val in enumerate([0.0, np.nan, np.inf, F32(sc.depth_min) * F32(0.5), F32(sc.depth_max) * F32(2.0)]):
        depth[pick == k] = val
    return depth


@pytest.mark.parametrize("strict", [True, False])
def test_merge_is_the_composition_bit_for_bit(strict):
    import torch
    sc, _, maps, B = _case(SHAPES[1])
    imgs = _u8(sc)
    depth = _offered_depth(sc, B, maps)

    def start():
        m = _matcher(sc, imgs, strict=strict, seed=11)
        m.set_geom_depths(maps, weight=0.2)
        m.pm_init()
        m.pm_iterate(1)
        return m

    # the expected state, from existing entries
    e = start()
    e.rescore()
    P, Cst, bv, rt = e.get_plane()
    orc = ol.Oracle([np.asarray(i, F32) for i in imgs], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=11,
                    flags=0 if strict else ol.FLAGS_FAST_8BIT_IMAGERY)
    with np.errstate(all="ignore"):
        usable = np.isfinite(depth) & (depth >= F32(sc.depth_min)) & (depth <= F32(sc.depth_max))
    assert 0.05 < (~usable).mean() < 0.6
    Q = P.copy()
    for y, x in zip(*np.nonzero(usable)):
        Q[y, x, 3] = orc.getD(P[y, x, :3], int(x), int(y), float(depth[y, x]))
    cq, bq, rq = e.pm_cost_planes(Q)
    take = cq < Cst
    want = (np.where(take[..., None], Q, P), np.where(take, cq, Cst), np.where(take, bq, bv), np.where(take, rq, rt))
    e.close()
    assert take.sum() > 0 and not take[~usable].any()
    for where in ("host", "device"):
        m = start()
        m.enable_kernel_timing(True)
        n_taken = m.merge_depths(depth if where == "host" else torch.from_numpy(depth).cuda())
        got = m.get_plane()
        assert n_taken == int(take.sum()), (n_taken, int(take.sum()))
        for name, g, w_ in zip(("planes", "cost", "best view", "ratio"), got, want):
            assert _bits_equal(g, w_), (where, name, int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w_).view(np.uint32)).sum()))
        # every stored cost is its plane's score
        cc, cbv, crt = m.pm_cost_planes(got[0])
        assert _bits_equal(cc, got[1]) and np.array_equal(cbv, got[2]) and _bits_equal(crt, got[3])
        t = m.kernel_timing()
        assert t["pm_merge_depths"][0] == 2 and t["pm_rescore"][0] == 1
        with pytest.raises(api.TsarError) as err:                # the result is void
            m.get_result()
        assert err.value.code == api.TSAR_ERR_STATE
        m.close()


def test_a_merge_that_offers_nothing_is_rescore():
    sc, _, maps, _ = _case(SHAPES[1])
    imgs = _u8(sc)
    R0 = np.asarray(sc.R[0], np.float64)
    own = sc.gt_depth.numpy().astype(F32).copy()
    own[20:30, 30:60] = 0                                       # rescore draws here
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ R0).astype(F32)

    def run(merge):
        m = _matcher(sc, imgs, strict=False, seed=9)
        m.load_planes(own, normal_world)
        m.set_geom_depths(maps, weight=0.2)
        taken = m.merge_depths(np.zeros((sc.h, sc.w), F32)) if merge else m.rescore()
        first = m.get_plane()
        m.pm_iterate(2)
        second = m.get_plane()
        m.close()
        return taken, first, second

    (taken, a1, a2), (_, b1, b2) = run(True), run(False)
    assert taken == 0
    assert all(_bits_equal(a, b) for a, b in zip(a1, b1))
    assert all(_bits_equal(a, b) for a, b in zip(a2, b2))


def test_python_pass_with_cross_view():
    sc, _, maps, _ = _case(SHAPES[1])
    imgs = _u8(sc)
    p1 = _matcher(sc, imgs, strict=False, seed=9)
    p1.pm_init()
    p1.pm_iterate(1)
    p1.compute_disp()
    own = p1.get_result(("depth", "normal"))
    p1.close()

    def result(fn):
        m = _matcher(sc, imgs, strict=False, seed=9)
        fn(m)
        out = (m.get_plane(), m.get_result())
        m.close()
        return out

    def manual(m):
        m.load_planes(own["depth"], own["normal"])
        m.set_geom_depths(maps, weight=0.2, clip=3.0)
        r = m.geom_reproject(0.01, 2, want=("depth",), device=True)
        assert m.merge_depths(r["depth"]) > 0
        m.pm_iterate(1)
        m.compute_disp()

    def same(a, b):
        return all(_bits_equal(x, y) for x, y in zip(a[0], b[0])) and all(_bits_equal(a[1][k], b[1][k]) for k in a[1])

    cross = result(lambda m: api.run_geom_pass(m, own["depth"], own["normal"], maps, 1, cross_view=2))
    assert same(cross, result(manual))
    plain = result(lambda m: api.run_geom_pass(m, own["depth"], own["normal"], maps, 1))
    assert same(plain, result(lambda m: api.run_geom_pass(m, own["depth"], own["normal"], maps, 1, cross_view=0)))
    assert not same(plain, cross)                               # (the switch is not idle)
    # coarse to fine: levels = 0 is the single-scale pass; one level down runs
    ms0 = result(lambda m: api.run_geom_pass_multiscale(m, own["depth"], own["normal"], maps, 0, 1, 1, cross_view=2))
    assert same(ms0, cross)
    with pytest.raises(ValueError):
        api.run_geom_pass(None, None, None, None, 1, cross_view=64)
    with pytest.raises(ValueError):
        api.run_geom_pass(None, None, None, None, 1, cross_view=1, cross_view_depth_diff=0.0)


def test_python_pass_multiscale_with_cross_view():
    """one level down: the merge runs on the full-resolution matcher right after its term is installed, before the chain is carried down"""
    sc = synth.make_scene(128, 96, 3, seed=94, all_gt=True)
    imgs = _u8(sc)
    maps = _gt_maps(sc)
    maps[0] = None
    p1 = _matcher(sc, imgs, strict=False, seed=9)
    p1.pm_init()
    p1.pm_iterate(1)
    p1.compute_disp()
    own = p1.get_result(("depth", "normal"))
    p1.close()

    def manual(m, c):
        m.clear_geom()
        c.clear_geom()
        c.pyramid_from(m)
        m.load_planes(own["depth"], own["normal"])
        m.set_geom_depths(maps, weight=0.2, clip=3.0)
        m.merge_depths(m.geom_reproject(0.01, 2, want=("depth",), device=True)["depth"])
        c.geom_pyramid_from(m)
        c.pyramid_planes_from(m)
        c.pm_iterate(1)
        m.upsample_merge(c)
        m.pm_iterate(1)
        m.compute_disp()

    a, ca = _matcher(sc, imgs, strict=False, seed=9), api.Matcher()
    manual(a, ca)
    b = _matcher(sc, imgs, strict=False, seed=9)
    cb = api.run_geom_pass_multiscale(b, own["depth"], own["normal"], maps, 1, 1, 1, cross_view=2)
    assert all(_bits_equal(x, y) for x, y in zip(a.get_plane(), b.get_plane()))
    assert _bits_equal(a.get_result(("depth",))["depth"], b.get_result(("depth",))["depth"])
    for m in (a, ca, b, *cb):
        m.close()


def test_cross_view_does_what_it_is_for():
    """Phase 1 (3 iterations) on every view of test_check_does_what_it_is_for's textureless scene in strict arithmetic, then phase 2 of
    view 0 (2 iterations) three ways with one seed: without the merge, with K = 1 and with K = 2; and the control again with another seed,
    whose distance from the first is the run-to-run noise of reseeding.  Shares of pixels within 1e-2 of ground truth over all pixels /
    textured / constant-albedo / recoverable pixels (phase-1 depth off by more than 1e-2 while the K = 2 render of the sources' phase-1
    maps is within 1e-2: 0.98 % of the image).  Bars from the CPU oracle in strict arithmetic, which the strict kernels reproduce bit for
    bit (tools/cross_view_oracle_bars.py, 800 x 576; measured there:
        control           0.7449 / 0.9674 / 0.0515 / 0.2976
        K = 1             0.7431 / 0.9679 / 0.0426 / 0.3315     (37.5 % of the pixels took the offered depth)
        K = 2             0.7450 / 0.9678 / 0.0511 / 0.3317     (18.4 %)
        control, reseeded 0.7447 / 0.9673 / 0.0511 / 0.2974 ).
    The merge recovers 3.4 points more of the recoverable pixels than propagation alone and leaves the rest where it was: a small gain.
    The figures are printed before they are asserted; GPU-observed values have not been recorded yet."""
    sc = synth.make_scene(800, 576, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True)
    imgs = _u8(sc)
    n = len(imgs)
    depth1, normal1 = [], []
    for k in range(n):
        iv, K, R, t, _ = _reorder(sc, imgs, k)
        m = _matcher(sc, iv, box=11, n_best=1, strict=True, seed=41 + k, K=K, R=R, t=t)
        m.pm_init()
        m.pm_iterate(3)
        m.compute_disp()
        r = m.get_result(("depth", "normal"))
        depth1.append(r["depth"].copy())
        normal1.append(r["normal"].copy())
        m.close()
    maps = [None] + depth1[1:]
    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()
    good = lambda D: np.abs(D - gt) / gt < 1e-2

    def phase2(seed, K):
        m = _matcher(sc, imgs, strict=True, seed=seed)
        m.load_planes(depth1[0], normal1[0])
        m.set_geom_depths(maps, weight=0.2, clip=3.0)
        render2 = m.geom_reproject(0.01, 2, want=("depth",))["depth"]
        m.rescore()
        taken = None
        if K:
            rescored = m.get_plane()[1]
            taken = m.merge_depths(m.geom_reproject(0.01, K, want=("depth",), device=True)["depth"])
            assert taken > 0
            assert np.all(m.get_plane()[1] <= rescored)          # right after the merge no pixel's cost is above its rescored cost
        m.pm_iterate(2)
        m.compute_disp()
        D = m.get_result(("depth",))["depth"].copy()
        m.close()
        return D, render2, taken

    runs = {"control": phase2(41, 0), "K=1": phase2(41, 1), "K=2": phase2(41, 2), "control, reseeded": phase2(43, 0)}
    recoverable = ~good(depth1[0]) & good(runs["control"][1])
    share = {}
    for name, (D, _, taken) in runs.items():
        g = good(D)
        share[name] = (float(g.mean()), float(g[tex].mean()), float(g[~tex].mean()), float(g[recoverable].mean()))
        print("%-18s all %.4f textured %.4f constant-albedo %.4f recoverable %.4f%s" % ((name,) + share[name] + ("" if taken is None else "  taken %.4f" % (taken / g.size),)))
    print("recoverable pixels: %.4f of the image" % recoverable.mean())
    noise = abs(share["control"][1] - share["control, reseeded"][1])
    for name in ("K=1", "K=2"):
        assert share[name][1] >= share["control"][1] - noise, (name, share[name][1], share["control"][1], noise)
        assert share[name][3] >= 0.31, (name, share[name][3])    # measured 0.3315 / 0.3317
        assert share[name][3] > share["control"][3]
    for name in runs:
        assert share[name][0] >= 0.73 and share[name][1] >= 0.96 and share[name][2] >= 0.03, (name, share[name])
    assert share["control"][3] >= 0.28                           # measured 0.2976
    assert 0.005 <= recoverable.mean() <= 0.02                   # measured 0.0098


# ---- the command line: tsar_gipuma --all --geom_consistency --geom_cross_view ------------------------------------------------------
def _cli(*args):
    out = subprocess.run(list(args), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_cli_geom_cross_view(tmp_path):
    sc = synth.make_scene(96, 72, 2, seed=69, textureless=True)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    n = len(sc.images)
    pairs = tio.read_pairs(root + "pair.txt")
    vd = lambda k: root + f"APD/{k:08d}/"
    base = [CLI, "--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=2", "--blocksize=11", "--n_best=1", "--seed=7",
            "--geom_consistency", "--geom_iterations=1"]

    def compare(K):
        """api.run_geom_pass(..., cross_view=K) on the files the CLI read for each view"""
        for k in range(n):
            ids = [k] + [s for s, _ in pairs[k]]
            cams = [tio.read_cam(root + f"cams/{i:08d}_cam.txt") for i in ids]
            m = api.Matcher()
            m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=cams[0][3], depth_max=cams[0][4], flags=0, seed=7 + k))
            m.set_views([tio.read_pgm(root + f"images/{i:08d}.pgm") for i in ids], np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]),
                        np.stack([c[2] for c in cams]), u8=True)
            src = [None] + [tio.read_dmb(vd(i) + "TSAR_disp.dmb") for i in ids[1:]]
            api.run_geom_pass(m, tio.read_dmb(vd(k) + "TSAR_disp.dmb"), tio.read_dmb(vd(k) + "TSAR_normals.dmb"), src, 1, cross_view=K)
            r = m.get_result(("depth", "normal"))
            m.close()
            assert _bits_equal(r["depth"], tio.read_dmb(vd(k) + "TSAR_geom_disp.dmb")), (K, k)
            assert _bits_equal(r["normal"], tio.read_dmb(vd(k) + "TSAR_geom_normals.dmb")), (K, k)
            rec = open(vd(k) + "TSAR_geom.txt").read()
            if K:
                assert f"\ngeom_cross_view={K} geom_cross_view_depth_diff=0.00999999978\n" in rec
            else:
                assert "geom_cross_view" not in rec

    first = _cli(*base, "--geom_cross_view")
    assert first.stdout.count("(geom): ok") == n
    compare(2)
    # a rerun skips every view of both phases; another K recomputes phase 2 only; without the switch the record does not name it
    again = _cli(*base, "--geom_cross_view")
    assert again.stdout.count("geom outputs present, skipped") == n and again.stdout.count("outputs present, skipped") == 2 * n
    other = _cli(*base, "--geom_cross_view=1")
    assert "geom outputs present" not in other.stdout and other.stdout.count("(geom): ok") == n
    assert other.stdout.count("outputs present, skipped") == n   # (phase 1 stands)
    compare(1)
    plain = _cli(*base)
    assert plain.stdout.count("(geom): ok") == n
    compare(0)

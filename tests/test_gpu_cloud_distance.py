"""tsar_cloud_distance on the GPU against the numpy restatement (tests/cloud_distance_ref.py): dist2 bit for bit; index, within,
n_valid_query and pairs exactly (pairs against the numpy count of the 27-cell candidates) — in host and device memory, with strides 3, 4
and 9 (the extra columns hold NaN: they must not be read as coordinates), through a strict and a fast context; determinism, the
shuffled-target invariance, the context left as it was, the refusals, evaluate_cloud on a fused ground-truth cloud and on a PatchMatch
cloud, and the tsar_evaluate tool."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from cloud_distance_ref import cell_edge, cloud_distance_ref, evaluate_ref, pairs_per_query, pairs_ref
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctxs(small_scene):
    """a strict and a fast context, each holding views and a plane state: the operator must run on them and leave them alone"""
    ms = {}
    for name, flags in (("strict", api.FLAG_STRICT_DIV), ("fast", 0)):
        m = api.matcher_from_scene(small_scene, seed=5, flags=flags)
        m.pm_init()
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


def padded(a, stride):
    out = np.full((len(a), stride), np.nan, F)
    out[:, :3] = a
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def check(ctxs, q, t, R, tol=None, modes=(("strict", False, 3, 3), ("fast", True, 9, 4))):
    """the operator against the restatement: (context, device memory, query stride, target stride) per mode"""
    tol = [R, 0.5 * R, 0.1 * R] if tol is None else tol
    ref = cloud_distance_ref(q, t, R, tol)
    pairs = pairs_ref(q, t, R)
    for name, on_device, qs, ts in modes:
        qq, tt = padded(q, qs), padded(t, ts)
        if on_device:
            qq, tt = torch.from_numpy(qq).cuda(), torch.from_numpy(tt).cuda()
        r = api.cloud_distance(qq, tt, R, tol, matcher=ctxs[name])
        d2, idx = (r["dist2"].cpu().numpy(), r["index"].cpu().numpy()) if on_device else (r["dist2"], r["index"])
        assert d2.dtype == F and idx.dtype == np.int32 and d2.shape == (len(q),) and idx.shape == (len(q),)
        assert same_bits(d2, ref["dist2"]), "dist2 differs in %d of %d" % (np.count_nonzero(d2.view(np.uint32) != ref["dist2"].view(np.uint32)), len(q))
        assert np.array_equal(idx, ref["index"])
        assert r["within"].tolist() == ref["within"].tolist() and r["n_valid_query"] == ref["n_valid_query"]
        assert r["pairs"] == pairs
    return ref


@pytest.mark.parametrize("n_target", [0, 1, 65, 3000])
@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 257, 5000])
def test_uniform_box_sizes(ctxs, n_query, n_target):
    rng = np.random.default_rng(1000 * n_query + n_target)
    q, t = rng.random((n_query, 3), dtype=F), rng.random((n_target, 3), dtype=F)
    hits = 0
    for R in (0.05, 0.2, 2.0):          # at 2.0 the whole cloud sits in one cell
        hits += np.count_nonzero(check(ctxs, q, t, R)["index"] >= 0)
    assert (hits > 0) == (n_target > 0)


def test_many_points_in_one_cell(ctxs):
    rng = np.random.default_rng(2)
    t = (rng.random((4096, 3), dtype=F) * F(0.9)).astype(F)
    q = (rng.random((300, 3), dtype=F) * F(1.5) - F(0.3)).astype(F)
    assert pairs_ref(t[:1], t, 1.0) == 4096
    ref = check(ctxs, q, t, 1.0)
    assert 0 < np.count_nonzero(ref["index"] >= 0)


def test_a_plane_is_one_layer_of_cells(ctxs):
    rng = np.random.default_rng(3)
    t = rng.random((3000, 3), dtype=F)
    t[:, 2] = F(0.625)
    q = rng.random((1000, 3), dtype=F)
    q[:, 2] = (F(0.625) + (rng.random(1000, dtype=F) - F(0.5)) * F(0.2)).astype(F)
    ref = check(ctxs, q, t, 0.06)
    assert 0 < np.count_nonzero(ref["index"] >= 0) < 1000


@pytest.mark.parametrize("R", [0.125, 0.37])
def test_points_on_cell_borders(ctxs, R):
    """coordinates that are float32 roundings of whole multiples of the cell edge (the origin is 0: a target sits there), and their
    float32 neighbours on either side"""
    rng = np.random.default_rng(4)
    e = cell_edge(R)
    base = (rng.integers(0, 12, size=(1500, 3)) * e).astype(F)
    t = np.nextafter(base, (base + rng.integers(-1, 2, size=base.shape)).astype(F)).astype(F)
    t = np.abs(t)
    t[0] = 0
    qb = (rng.integers(-1, 13, size=(1200, 3)) * e).astype(F)
    q = np.nextafter(qb, (qb + rng.integers(-1, 2, size=qb.shape)).astype(F)).astype(F)
    ref = check(ctxs, q, t, R)
    assert 0 < np.count_nonzero(ref["index"] >= 0)


def test_negative_coordinates_and_an_offset_cloud(ctxs):
    rng = np.random.default_rng(5)
    t = (rng.random((2000, 3), dtype=F) - F(0.5)) * F(3.0)
    q = (rng.random((1500, 3), dtype=F) - F(0.5)) * F(3.4)
    ref = check(ctxs, (q - F(7.0)).astype(F), (t - F(7.0)).astype(F), 0.2)
    assert 0 < np.count_nonzero(ref["index"] >= 0) < 1500
    # offset by 1e4: the coordinates keep about 1e-3 of resolution, dx cancels, and many distances tie
    off = np.array([1e4, -1e4, 1e4], F)
    ref = check(ctxs, (q + off).astype(F), (t + off).astype(F), 0.2)
    assert 0 < np.count_nonzero(ref["index"] >= 0) < 1500


def test_duplicated_points_give_the_smallest_index(ctxs):
    rng = np.random.default_rng(6)
    base = rng.random((300, 3), dtype=F)
    t = np.concatenate([base, base[::-1], base[100:200], base])          # every point three or four times, in mixed order
    q = np.concatenate([base[:150], rng.random((150, 3), dtype=F)])
    ref = check(ctxs, q, t, 0.1)
    assert np.array_equal(ref["index"][:150], np.arange(150)) and (ref["dist2"][:150] == 0).all()


def test_non_finite_records(ctxs):
    rng = np.random.default_rng(7)
    q, t = rng.random((700, 3), dtype=F), rng.random((900, 3), dtype=F)
    for a in (q, t):
        a[5] = np.nan
        a[17, 1] = np.inf
        a[64, 2] = -np.inf
        a[len(a) - 1, 0] = np.nan
        a[200:230] = np.nan
    ref = check(ctxs, q, t, 0.1)
    assert ref["n_valid_query"] == 700 - 34 and not np.isin(ref["index"], [5, 17, 64, 899] + list(range(200, 230))).any()
    # no candidate on one side or the other
    check(ctxs, q, np.full((40, 3), np.nan, F), 0.1)
    check(ctxs, np.full((40, 3), np.inf, F), t, 0.1)


def test_query_is_target(ctxs):
    rng = np.random.default_rng(8)
    a = rng.random((2500, 3), dtype=F)
    ref = check(ctxs, a, a, 0.03)
    assert np.array_equal(ref["index"], np.arange(2500))
    d = torch.from_numpy(padded(a, 9)).cuda()                             # the same device buffer on both sides
    r = api.cloud_distance(d, d, 0.03, [0.03], matcher=ctxs["fast"])
    assert np.array_equal(r["index"].cpu().numpy(), np.arange(2500)) and r["within"].tolist() == [2500]


def test_two_calls_give_the_same_bits_and_a_shuffled_target_the_same_distances(ctxs):
    rng = np.random.default_rng(9)
    q, t = rng.random((4000, 3), dtype=F), rng.random((3500, 3), dtype=F)   # random points: no two targets at one distance
    a = api.cloud_distance(q, t, 0.08, [0.08, 0.02], matcher=ctxs["fast"])
    b = api.cloud_distance(q, t, 0.08, [0.08, 0.02], matcher=ctxs["fast"])
    c = api.cloud_distance(q, t, 0.08, [0.08, 0.02])                        # a context of the call's own
    for r in (b, c):
        assert same_bits(a["dist2"], r["dist2"]) and np.array_equal(a["index"], r["index"]) and a["within"].tolist() == r["within"].tolist()
        assert (a["pairs"], a["n_valid_query"]) == (r["pairs"], r["n_valid_query"])
    perm = rng.permutation(len(t))
    s = api.cloud_distance(q, t[perm], 0.08, [0.08, 0.02], matcher=ctxs["strict"])
    assert same_bits(a["dist2"], s["dist2"]) and a["within"].tolist() == s["within"].tolist() and a["pairs"] == s["pairs"]
    hit = a["index"] >= 0
    assert 0 < hit.sum() < len(q) and np.array_equal(hit, s["index"] >= 0) and np.array_equal(perm[s["index"][hit]], a["index"][hit])


def test_want_names_the_outputs(ctxs):
    q = np.random.default_rng(10).random((100, 3), dtype=F)
    r = api.cloud_distance(q, q, 0.5, want=(), matcher=ctxs["fast"])
    assert "dist2" not in r and "index" not in r and r["within"].shape == (0,) and r["n_valid_query"] == 100
    r = api.cloud_distance(q, q, 0.5, want=("index",), matcher=ctxs["fast"])
    assert "dist2" not in r and np.array_equal(r["index"], np.arange(100))


def test_the_context_is_left_as_it_was(ctxs, small_scene):
    """get_plane before and after is bit-equal, and a fuse on the same context afterwards gives what it gave before"""
    sc = synth.make_scene(64, 48, 2, seed=8, all_gt=True)
    n = len(sc.images)
    depths = [d.numpy() for d, _ in sc.meta["gt_all"]]
    normals = [np.ascontiguousarray((nc.numpy() @ sc.R[v]).astype(F)) for v, (_, nc) in enumerate(sc.meta["gt_all"])]
    fuse = lambda m: api.fuse(depths, normals, [im.numpy() for im in sc.images], sc.K, sc.R, sc.t, {v: [s for s in range(n) if s != v] for v in range(n)},
                              api.FusionParams(1, 2.0, 0.01, 15.0, 1), matcher=m)
    rng = np.random.default_rng(11)
    q, t = rng.random((3000, 3), dtype=F), rng.random((3000, 3), dtype=F)
    for m in ctxs.values():
        before = m.get_plane()
        cloud_before = fuse(m)
        api.cloud_distance(q, t, 0.1, [0.05], matcher=m)
        with pytest.raises(api.TsarError):
            api.cloud_distance(q, t, 0.1, [0.5], matcher=m)              # a refused call leaves it alone too
        after = m.get_plane()
        assert all(same_bits(a, b) for a, b in zip(before, after))
        assert same_bits(cloud_before, fuse(m)) and len(cloud_before) > 0
        m.pm_iterate(1)                                                   # and the matcher goes on


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(fn, *fragments):
    with pytest.raises(api.TsarError) as e:
        fn()
    assert e.value.code == api.TSAR_ERR_INVALID
    for s in fragments:
        assert s in str(e.value), str(e.value)
    return e.value


def test_refusals(ctxs):
    m = ctxs["strict"]
    rng = np.random.default_rng(12)
    q, t = rng.random((500, 3), dtype=F), rng.random((400, 3), dtype=F)
    far = np.array([[0, 0, 0], [3e6, 0, 0]], F)
    refused(lambda: api.cloud_distance(q, far, 1.0, matcher=m), "max_dist", "2^20 cells")
    one_cell = (rng.random((4096, 3), dtype=F) * F(0.9)).astype(F)
    e = refused(lambda: api.cloud_distance(one_cell, one_cell, 1.0, [0.5], max_pairs=10 ** 6, matcher=m), "max_pairs", str(4096 * 4096))
    assert e.pairs == 4096 * 4096
    d = torch.from_numpy(one_cell).cuda()                                 # device outputs of a refused call are not written
    d2 = torch.full((4096,), -7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((4096,), -7, dtype=torch.int32, device="cuda")
    prm = api.CloudDistanceParams(1.0, 10 ** 6)
    pairs, within = C.c_int64(-1), (C.c_int64 * 1)(-5)
    tol = (C.c_float * 1)(0.5)
    torch.cuda.synchronize()
    rc = m.L.tsar_cloud_distance_ctx(m._ctx, d.data_ptr(), 4096, 3, d.data_ptr(), 4096, 3, C.byref(prm), 1, tol, d2.data_ptr(), idx.data_ptr(), within, None,
                                     C.byref(pairs), api.MEM_DEVICE)
    assert rc == api.TSAR_ERR_INVALID and pairs.value == 4096 * 4096 and within[0] == -5
    assert (d2 == -7.0).all().item() and (idx == -7).all().item()
    assert api.cloud_distance(one_cell, one_cell, 1.0, [0.5], max_pairs=4096 * 4096, matcher=m)["pairs"] == 4096 * 4096   # the bound itself passes
    refused(lambda: api.cloud_distance(q, t, 0.1, [0.05, 0.11], matcher=m), "tolerance")
    refused(lambda: api.cloud_distance(q, t, 0.1, [0.0], matcher=m), "tolerance")
    refused(lambda: api.cloud_distance(q, t, 0.1, [np.nan], matcher=m), "tolerance")
    for R in (0.0, -1.0, np.inf, np.nan, 1e-30, 1e30):                   # fl(R * R) is 0 or inf at the last two
        refused(lambda: api.cloud_distance(q, t, R, matcher=m), "max_dist")
    # a stride of 2 through the C entry (the binding asserts k >= 3 before it calls)
    prm = api.CloudDistanceParams(0.5, 1 << 40)
    for qs, ts in ((2, 3), (3, 2)):
        rc = m.L.tsar_cloud_distance_ctx(m._ctx, q.ctypes.data_as(C.c_void_p), 100, qs, t.ctypes.data_as(C.c_void_p), 100, ts, C.byref(prm), 0, None, None, None, None,
                                         None, None, api.MEM_HOST)
        assert rc == api.TSAR_ERR_INVALID and "stride" in m.L.tsar_last_error(m._ctx).decode()
    with pytest.raises(AssertionError):
        api.cloud_distance(q[:, :2], t, 0.5, matcher=m)
    check(ctxs, q, t, 0.1)                                                # and the context still works


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_clouds():
    """the fused ground-truth cloud of a 160 x 120 scene with three sources, and the fused cloud of a strict PatchMatch run on it"""
    sc = synth.make_scene(160, 120, 3, all_gt=True)
    n = len(sc.images)
    pairs = {v: [s for s in range(n) if s != v] for v in range(n)}
    grays = [im.numpy() for im in sc.images]
    depths = [d.numpy() for d, _ in sc.meta["gt_all"]]
    normals = [np.ascontiguousarray((nc.numpy() @ sc.R[v]).astype(F)) for v, (_, nc) in enumerate(sc.meta["gt_all"])]
    prm = api.FusionParams(1, 2.0, 0.01, 15.0, 1)
    gt = api.fuse(depths, normals, grays, sc.K, sc.R, sc.t, pairs, prm)
    pd, pn = [], []
    for ref in range(n):
        order = [ref] + [v for v in range(n) if v != ref]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, seed=3 + ref, flags=api.FLAG_STRICT_DIV))
        m.set_views([sc.images[v] for v in order], sc.K[order], sc.R[order], sc.t[order])
        m.pm_init()
        m.pm_iterate(3)
        m.compute_disp()
        res = m.get_result(("depth", "normal"))
        pd.append(res["depth"])
        pn.append(res["normal"])
        m.close()
    pm = api.fuse(pd, pn, grays, sc.K, sc.R, sc.t, pairs, prm)
    footprint = float(sc.depth_min) / float(sc.K[0][0, 0])               # no two pixels of one view are nearer to each other than this
    return gt, pm, footprint


def test_evaluate_a_cloud_against_itself_and_against_a_shifted_copy(scene_clouds):
    gt, _, footprint = scene_clouds
    tau = F(0.05 * footprint)
    # keep the points with no other point in the 27 cells of edge 3.5 tau around them (fusion leaves a few near-duplicates across views):
    # every other point is then more than 3.5 tau away
    gt = gt[pairs_per_query(gt, gt, F(3.5) * tau) == 1]
    assert len(gt) > 5000 and gt.shape[1] == 9                           # the 9-float records go in as they are
    r = api.evaluate_cloud(gt, gt, [tau, F(3) * tau])
    assert r["accuracy"].tolist() == [1.0, 1.0] and r["completeness"].tolist() == [1.0, 1.0] and r["f1"].tolist() == [1.0, 1.0]
    assert r["n_accurate"].tolist() == [len(gt)] * 2 and r["n_recon_valid"] == r["n_gt_valid"] == len(gt)
    assert r["accuracy"].dtype == np.float64
    # shifted by 2 tau along x: a point's own original is 2 tau away (too far for tau, near enough for 3 tau), every other one more than 1.5 tau
    shifted = gt.copy()
    shifted[:, 0] += F(2) * tau
    r = api.evaluate_cloud(torch.from_numpy(shifted).cuda(), torch.from_numpy(gt).cuda(), [tau, F(3) * tau])
    assert r["accuracy"].tolist() == [0.0, 1.0] and r["completeness"].tolist() == [0.0, 1.0] and r["f1"].tolist() == [0.0, 1.0]
    assert r["n_accurate"].tolist() == [0, len(gt)]


def test_evaluate_a_patchmatch_cloud_equals_the_restatement(scene_clouds):
    gt, pm, footprint = scene_clouds
    assert len(gt) > 10000 and len(pm) > 5000
    gt, pm = gt[::7], pm[::5]                                             # every cloud thinned so that the brute-force restatement takes a second
    tol = [F(0.5 * footprint), F(2 * footprint), F(8 * footprint)]
    ref = evaluate_ref(pm, gt, tol)
    r = api.evaluate_cloud(pm, gt, tol)
    assert r["n_accurate"].tolist() == ref["n_accurate"].tolist() and r["n_complete"].tolist() == ref["n_complete"].tolist()
    assert (r["n_recon_valid"], r["n_gt_valid"]) == (ref["n_recon_valid"], ref["n_gt_valid"]) == (len(pm), len(gt))
    for k in ("accuracy", "completeness", "f1"):
        assert r[k].tolist() == ref[k].tolist()
    assert 0 < ref["n_accurate"][0] < ref["n_accurate"][2] and 0 < ref["n_complete"][0] < ref["n_complete"][2]      # the tolerances separate something
    assert r["pairs_accuracy"] == pairs_ref(pm, gt, max(tol)) and r["pairs_completeness"] == pairs_ref(gt, pm, max(tol))


def test_the_tool(scene_clouds, tmp_path):
    gt, pm, footprint = scene_clouds
    gt, pm = gt[::7], pm[::5]
    a, b = str(tmp_path / "pm.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, pm)
    tio.write_ply(b, gt, binary=False)
    tol = [F(0.5 * footprint), F(4 * footprint)]
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate")
    out = subprocess.run([tool, a, b, "--tolerances=%.9g,%.9g" % tuple(tol), "--json=" + str(tmp_path / "r.json")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    ref = evaluate_ref(pm, gt, tol)
    assert rec["n_accurate"] == ref["n_accurate"].tolist() and rec["n_complete"] == ref["n_complete"].tolist()
    assert (rec["n_recon"], rec["n_gt"], rec["n_recon_valid"], rec["n_gt_valid"]) == (len(pm), len(gt), len(pm), len(gt))
    assert rec["accuracy"] == ref["accuracy"].tolist() and rec["completeness"] == ref["completeness"].tolist() and rec["f1"] == ref["f1"].tolist()
    assert rec["pairs_accuracy"] == pairs_ref(pm, gt, max(tol)) and rec["pairs_completeness"] == pairs_ref(gt, pm, max(tol))
    # a radius as large as the scene is refused, with the library's reason
    out = subprocess.run([tool, a, b, "--tolerances=1000", "--max_pairs=1000"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "max_pairs" in out.stderr and out.stdout == ""

"""tsar_cloud_voxels on the GPU against the numpy restatement (tests/cloud_voxels_ref.py): rank, rep, count, within, n_voxels and n_valid
exactly, every element — in host and device memory, with strides 3, 4 and 9 (the extra columns hold NaN), through a strict and a fast
context that hold views and a plane state; runs of one voxel that straddle waves, borders, ties, non-finite records and distances, a cap
below the number of voxels, determinism, the shuffled cloud, every refusal; evaluate_cloud(voxel=, crop=), voxel_downsample, tsar_fusion
--voxel and tsar_evaluate --voxel."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from cloud_voxels_ref import cloud_voxels_ref, density_case, evaluate_voxel_ref
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("strict", False, 3), ("fast", True, 9), ("fast", False, 4))       # (context, device memory, stride)


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
    out[:, :3] = a[:, :3]
    return out


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def check(ctxs, cloud, V, dist2=None, tol=None, modes=MODES):
    """the operator against the restatement, every output, every element"""
    ref = cloud_voxels_ref(cloud, V, dist2, tol)
    for name, on_device, stride in modes:
        c, d2 = padded(cloud, stride), dist2
        if on_device:
            c = torch.from_numpy(c).cuda()
            d2 = None if dist2 is None else torch.from_numpy(np.ascontiguousarray(dist2, F)).cuda()
        r = api.cloud_voxels(c, V, d2, tol, matcher=ctxs[name])
        assert (r["n_voxels"], r["n_valid"]) == (ref["n_voxels"], ref["n_valid"])
        for k in ("rank", "rep", "count") + (("within",) if tol is not None else ()):
            got = host(r[k])
            assert got.dtype == np.int32 and got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
            assert np.array_equal(got, ref[k]), "%s differs in %d of %d (%s, device %s, stride %d)" % (k, np.count_nonzero(got != ref[k]), got.size, name, on_device, stride)
        assert ("within" in r) == (tol is not None)
    return ref


def some_dist2(rng, n):
    """distances of every kind: small, zero, exactly a squared tolerance, +inf, NaN"""
    d = (rng.random(n, dtype=F) * F(0.02)).astype(F)
    kind = rng.integers(0, 10, size=n)
    d[kind == 0] = 0
    d[kind == 1] = np.inf
    d[kind == 2] = np.nan
    d[kind == 3] = F(0.1) * F(0.1)
    return d


TOL = [0.1, 0.05, 0.12]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_uniform_box_sizes(ctxs, n):
    rng = np.random.default_rng(100 + n)
    c = rng.random((n, 3), dtype=F)
    d2 = some_dist2(rng, n)
    one = check(ctxs, c, 2.0, d2, TOL)                                       # one voxel: at n = 5000 one run crosses 79 waves
    assert one["n_voxels"] == min(n, 1)
    alone = check(ctxs, c, 0.001, d2, TOL)                                   # nearly every point alone
    assert alone["n_voxels"] >= n - 2
    mid = check(ctxs, c, 0.13, d2, TOL)
    if n == 5000:
        assert 300 < mid["n_voxels"] < 600 and mid["count"].max() > 10 and 0 < mid["within"][:, 1].sum() < mid["within"][:, 2].sum()
    check(ctxs, c, 0.13)                                                     # without dist2: no "within"


@pytest.mark.parametrize("per_voxel", [3, 65])
def test_runs_that_straddle_wave_boundaries(ctxs, per_voxel):
    rng = np.random.default_rng(per_voxel)
    c = (rng.random((200, per_voxel, 3), dtype=F) * F(0.8) + F(0.1)).astype(F)
    c[:, :, 0] += np.arange(200, dtype=F)[:, None]
    c[0, 0] = 0                                                              # the origin: the cells are the unit cells
    c = c.reshape(-1, 3)[rng.permutation(200 * per_voxel)]
    ref = check(ctxs, c, 1.0, some_dist2(rng, len(c)), TOL)
    assert ref["n_voxels"] == 200 and (ref["count"] == per_voxel).all()


def test_a_plane_is_one_layer_of_cells(ctxs):
    rng = np.random.default_rng(3)
    c = rng.random((3000, 3), dtype=F)
    c[:, 2] = F(0.625)
    ref = check(ctxs, c, 0.06, some_dist2(rng, 3000), TOL)
    assert (ref["keys"] >> 42 == 0).all() and 200 < ref["n_voxels"] < 300
    c[:, 1] = F(-3.0)                                                        # a line
    assert check(ctxs, c, 0.06)["n_voxels"] == 17


@pytest.mark.parametrize("V", [0.125, 0.37])
def test_points_on_voxel_borders(ctxs, V):
    """coordinates that are float32 roundings of whole multiples of V (the origin is 0: a point sits there), and their float32 neighbours
    on either side"""
    rng = np.random.default_rng(4)
    base = (rng.integers(0, 12, size=(3000, 3)) * np.float64(F(V))).astype(F)
    c = np.abs(np.nextafter(base, (base + rng.integers(-1, 2, size=base.shape)).astype(F)).astype(F))
    c[0] = 0
    ref = check(ctxs, c, V, some_dist2(rng, 3000), TOL)
    assert 1000 < ref["n_voxels"] <= 13 ** 3


def test_negative_coordinates_and_an_offset_cloud(ctxs):
    rng = np.random.default_rng(5)
    c = ((rng.random((3000, 3), dtype=F) - F(0.5)) * F(3.0)).astype(F)
    d2 = some_dist2(rng, 3000)
    assert check(ctxs, (c - F(7.0)).astype(F), 0.2, d2, TOL)["n_voxels"] > 1000
    # offset by 1e4: the coordinates keep about 1e-3 of resolution, and many points coincide or tie
    off = np.array([1e4, -1e4, 1e4], F)
    assert check(ctxs, (c + off).astype(F), 0.2, d2, TOL)["n_voxels"] > 1000
    assert check(ctxs, (c + off).astype(F), 0.004, d2, TOL)["n_voxels"] > 2000


def test_ties_to_the_centre_and_duplicated_points(ctxs):
    rng = np.random.default_rng(6)
    cells = rng.integers(0, 6, size=(400, 3)).astype(F)
    sign = rng.choice(np.array([-0.25, 0.25], F), size=(400, 3))
    c = np.concatenate([np.zeros((1, 3), F), cells + F(0.5) + sign, cells + F(0.5) - sign, cells[::-1] + F(0.5) + sign[::-1]]).astype(F)   # V = 1: all at one d2f per cell
    ref = check(ctxs, c, 1.0, some_dist2(rng, len(c)), TOL)
    occupied = ref["count"] > 1
    assert occupied.sum() > 100 and (np.diff(np.sort(ref["d2f"][1:])) == 0).all()
    first = np.full(ref["n_voxels"], len(c), np.int64)
    np.minimum.at(first, ref["rank"][1:], np.arange(1, len(c)))
    assert np.array_equal(ref["rep"][1:], first[1:])                                # the smallest index of every voxel (voxel 0 holds the origin point too)
    base = rng.random((300, 3), dtype=F)
    dup = np.concatenate([base, base[::-1], base[100:200], base])
    ref = check(ctxs, dup, 0.09, some_dist2(rng, len(dup)), TOL)
    assert (ref["rep"] < 300).all() and (ref["count"] >= 3).all()


def test_non_finite_records_and_non_finite_distances(ctxs):
    rng = np.random.default_rng(7)
    c = rng.random((900, 3), dtype=F)
    c[5] = np.nan
    c[17, 1] = np.inf
    c[64, 2] = -np.inf
    c[899, 0] = np.nan
    c[200:230] = np.nan
    c[0] = [np.inf, np.nan, 0]
    d2 = some_dist2(rng, 900)
    d2[300:330] = [np.nan, np.inf, 0.0] * 10
    ref = check(ctxs, c, 0.1, d2, TOL)
    assert ref["n_valid"] == 900 - 35 and (ref["rank"][[0, 5, 17, 64, 899]] == -1).all() and (ref["rank"][200:230] == -1).all()
    assert not np.isin(ref["rep"], [0, 5, 17, 64, 899] + list(range(200, 230))).any()
    assert check(ctxs, np.full((70, 3), np.nan, F), 0.1, np.zeros(70, F), TOL)["n_voxels"] == 0       # no candidate: every rank -1
    allnan = check(ctxs, c, 0.1, np.full(900, np.nan, F), TOL)
    assert (allnan["within"] == 0).all()


def raw_call(m, cloud, V, cap, tol=None, dist2=None, on_device=False, sentinel=-7):
    """the C entry with buffers of len(cloud) voxels filled with a sentinel -> (rc, n_voxels, n_valid, rank, rep, count, within)"""
    n, n_tol = len(cloud), 0 if tol is None else len(tol)
    bufs = [np.full(n, sentinel, np.int32), np.full(n, sentinel, np.int32), np.full(n, sentinel, np.int32), np.full((n, max(n_tol, 1)), sentinel, np.int32)]
    c, d2 = np.ascontiguousarray(cloud, F), None if dist2 is None else np.ascontiguousarray(dist2, F)
    if on_device:
        bufs = [torch.from_numpy(b).cuda() for b in bufs]
        c, d2 = torch.from_numpy(c).cuda(), None if d2 is None else torch.from_numpy(d2).cuda()
        torch.cuda.synchronize()
    ptr = (lambda a: None if a is None else C.c_void_p(a.data_ptr())) if on_device else (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
    t = None if tol is None else np.ascontiguousarray(tol, F)
    nv, nvalid = C.c_int64(-1), C.c_int64(-1)
    prm = api.CloudVoxelsParams(V)
    rc = m.L.tsar_cloud_voxels_ctx(m._ctx, ptr(c), n, c.shape[1], C.byref(prm), ptr(d2), n_tol, None if t is None else t.ctypes.data_as(C.c_void_p), ptr(bufs[0]), cap,
                                   ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]) if n_tol else None, C.byref(nv), C.byref(nvalid), api.MEM_DEVICE if on_device else api.MEM_HOST)
    return (rc, nv.value, nvalid.value) + tuple(host(b) for b in bufs)


@pytest.mark.parametrize("on_device", [False, True])
def test_a_cap_below_the_number_of_voxels(ctxs, on_device):
    rng = np.random.default_rng(8)
    c = rng.random((4000, 3), dtype=F)
    d2 = some_dist2(rng, 4000)
    ref = cloud_voxels_ref(c, 0.1, d2, TOL)
    assert ref["n_voxels"] > 900
    for cap in (0, 1, 64, 700, ref["n_voxels"], 4000):
        rc, nv, nvalid, rank, rep, count, within = raw_call(ctxs["fast"], c, 0.1, cap, TOL, d2, on_device)
        w = min(cap, ref["n_voxels"])
        assert rc == api.TSAR_OK and nv == ref["n_voxels"] and nvalid == 4000                   # the number found is reported, the call succeeds
        assert np.array_equal(rank, ref["rank"])                                                   # ranks name voxels beyond the cap too
        assert np.array_equal(rep[:w], ref["rep"][:w]) and np.array_equal(count[:w], ref["count"][:w]) and np.array_equal(within[:w], ref["within"][:w])
        assert (rep[w:] == -7).all() and (count[w:] == -7).all() and (within[w:] == -7).all()     # nothing is written behind it


def test_two_calls_give_the_same_bits_and_a_shuffled_cloud_the_same_voxels(ctxs):
    rng = np.random.default_rng(9)
    c = rng.random((6000, 3), dtype=F)
    d2 = some_dist2(rng, 6000)
    want = ("rank", "rep", "count")
    a = api.cloud_voxels(c, 0.07, d2, TOL, want=want, matcher=ctxs["fast"])
    b = api.cloud_voxels(c, 0.07, d2, TOL, want=want, matcher=ctxs["fast"])
    own = api.cloud_voxels(c, 0.07, d2, TOL, want=want)                      # a context of the call's own
    for r in (b, own):
        assert all(np.array_equal(a[k], r[k]) for k in want + ("within",)) and (a["n_voxels"], a["n_valid"]) == (r["n_voxels"], r["n_valid"])
    perm = rng.permutation(6000)
    s = api.cloud_voxels(c[perm], 0.07, d2[perm], TOL, want=want, matcher=ctxs["strict"])
    # the origin and the keys do not depend on the order: the voxels keep their numbers, so (count, within) is unchanged voxel by voxel
    assert s["n_voxels"] == a["n_voxels"] and np.array_equal(s["count"], a["count"]) and np.array_equal(s["within"], a["within"])
    assert np.array_equal(s["rank"], a["rank"][perm])
    ref = cloud_voxels_ref(c, 0.07)
    order = np.lexsort((ref["d2f"], ref["rank"]))                             # per voxel its points by d2f
    rk, dd = ref["rank"][order], ref["d2f"][order]
    start = np.flatnonzero(np.r_[True, rk[1:] != rk[:-1]])
    second_equal = np.zeros(len(start), bool)
    has2 = ref["count"] > 1
    second_equal[has2] = dd[start[has2] + 1] == dd[start[has2]]
    once = ~second_equal                                                      # the minimal d2f is attained once
    assert once.sum() > 0.9 * len(once)
    assert np.array_equal(perm[s["rep"][once]], a["rep"][once])


def test_want_names_the_outputs_and_voxel_downsample(ctxs):
    rng = np.random.default_rng(10)
    c = padded(rng.random((3000, 3), dtype=F), 9)
    c[:, 3:] = rng.random((3000, 6), dtype=F)                                # whole records: normals and colours travel with the point
    c[11, 0] = np.nan
    r = api.cloud_voxels(c, 0.1, want=(), matcher=ctxs["fast"])
    assert not any(k in r for k in ("rank", "rep", "count", "within")) and r["n_valid"] == 2999
    ref = cloud_voxels_ref(c, 0.1)
    r = api.cloud_voxels(c, 0.1, want=("count",), matcher=ctxs["fast"])
    assert "rep" not in r and np.array_equal(r["count"], ref["count"])
    rows = np.sort(ref["rep"])
    thin = api.voxel_downsample(c, 0.1, matcher=ctxs["strict"])
    assert thin.shape == (ref["n_voxels"], 9) and np.array_equal(thin.view(np.uint32), c[rows].view(np.uint32))
    thin_d = api.voxel_downsample(torch.from_numpy(c).cuda(), 0.1)
    assert thin_d.is_cuda and np.array_equal(thin_d.cpu().numpy().view(np.uint32), c[rows].view(np.uint32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_context_works_afterwards(ctxs):
    m = ctxs["strict"]
    L = m.L
    rng = np.random.default_rng(12)
    c = rng.random((500, 3), dtype=F)
    d2 = some_dist2(rng, 500)
    cp, dp = c.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p)
    out = np.full(500, -7, np.int32)
    op = out.ctypes.data_as(C.c_void_p)
    tol = (C.c_float * 2)(0.1, 0.05)
    nv = C.c_int64(-1)

    def call(cloud=cp, n=500, stride=3, prm=api.CloudVoxelsParams(0.1), dist2=None, n_tol=0, t=None, cap=500, within=None, mem=api.MEM_HOST):
        rc = L.tsar_cloud_voxels_ctx(m._ctx, cloud, n, stride, C.byref(prm) if prm is not None else None, dist2, n_tol, t, op, cap, op, op, within, C.byref(nv), None, mem)
        return rc, L.tsar_last_error(m._ctx).decode()

    def refused(fragment, **kw):
        rc, msg = call(**kw)
        assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_voxels:") and fragment in msg, (rc, msg)
        assert (out == -7).all()                                              # a refused call writes nothing

    refused("params is NULL", prm=None)
    refused("mem must be", mem=7)
    refused("stride", stride=2)
    refused("n must be", n=-1)
    refused("n must be", n=1 << 31)
    for V in (0.0, -1.0, np.inf, -np.inf, np.nan):
        refused("voxel must be finite and > 0", prm=api.CloudVoxelsParams(V))
    refused("tolerances without tol or without dist2", n_tol=2, t=tol)                             # dist2 NULL
    refused("tolerances without tol or without dist2", n_tol=2, dist2=dp)                          # tol NULL
    for bad in (0.0, -0.1, np.inf, np.nan):
        refused("every tolerance must be finite and > 0", n_tol=2, dist2=dp, t=(C.c_float * 2)(0.1, bad), within=op)
    refused("within_out needs tolerances", within=op)
    refused("cap must be >= 0", cap=-1)
    far = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [0, 3e5, 0]], F)                                   # 3e5 / 0.1 >= 2^21 cells on y
    refused("2^21 cells or more", cloud=far.ctypes.data_as(C.c_void_p), n=3)
    with pytest.raises(api.TsarError) as e:
        api.cloud_voxels(far, 0.1, matcher=m)
    assert e.value.code == api.TSAR_ERR_INVALID and "2^21 cells" in str(e.value)
    assert api.cloud_voxels(far, 0.2, matcher=m)["n_voxels"] == 3                                  # 1.5e6 cells pass
    with pytest.raises(AssertionError):
        api.cloud_voxels(c[:, :2], 0.1, matcher=m)
    with pytest.raises(AssertionError):
        api.cloud_voxels(c, 0.1, dist2=d2, matcher=m)                                              # dist2 and tolerances go together
    check(ctxs, c, 0.1, d2, TOL)                                                                   # and the contexts still work


def test_the_contexts_are_left_as_they_were(ctxs):
    """get_plane before and after is bit-equal, after calls that succeed and calls that are refused, and the matcher goes on"""
    rng = np.random.default_rng(13)
    c = rng.random((5000, 3), dtype=F)
    d2 = some_dist2(rng, 5000)
    bits = lambda planes: [np.asarray(a).view(np.uint32).copy() for a in planes]
    for m in ctxs.values():
        before = bits(m.get_plane())
        api.cloud_voxels(c, 0.05, d2, TOL, matcher=m)
        api.cloud_voxels(torch.from_numpy(c).cuda(), 0.3, matcher=m)
        with pytest.raises(api.TsarError):
            api.cloud_voxels(c, 1e-8, matcher=m)
        api.evaluate_cloud(c, c[::2], [0.05], voxel=0.1, crop=(0, 0, 0, 0.5, 1, 1), matcher=m)
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(m.get_plane())))
        m.pm_iterate(1)


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_clouds():
    """the fused ground-truth cloud of the small scene and the fused cloud of a strict PatchMatch run on it"""
    sc = synth.make_scene(96, 64, 3, seed=7, all_gt=True)
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
    footprint = float(sc.depth_min) / float(sc.K[0][0, 0])
    assert len(gt) > 5000 and len(pm) > 1500                                 # small enough for the brute-force restatement of the distances as they are
    return gt, pm, footprint


def same_evaluation(r, ref, voxel, crop):
    for k in ("n_accurate", "n_complete"):
        assert r[k].tolist() == ref[k].tolist()
    for k in ("n_recon_valid", "n_gt_valid") + (("n_recon_voxels", "n_gt_voxels") if voxel is not None else ()) + (("n_recon_cropped", "n_gt_cropped") if crop is not None else ()):
        assert r[k] == ref[k], k
    for k in ("accuracy", "completeness", "f1") + (("accuracy_voxel", "completeness_voxel", "f1_voxel") if voxel is not None else ()):
        assert r[k].dtype == np.float64 and r[k].tolist() == ref[k].tolist(), k                   # float64 for float64


def test_evaluate_the_density_case(ctxs):
    recon, gt, tau, voxel = density_case()
    for rr, gg in ((recon, gt), (torch.from_numpy(recon).cuda(), torch.from_numpy(gt).cuda())):
        r = api.evaluate_cloud(rr, gg, [tau], voxel=voxel, matcher=ctxs["fast"])
        assert r["accuracy"].tolist() == [32 / 352] and r["accuracy_voxel"].tolist() == [0.5] and r["n_recon_voxels"] == 64
        assert r["completeness_voxel"].tolist() == [0.5] and r["f1_voxel"].tolist() == [0.5] and r["n_gt_voxels"] == 64
        same_evaluation(r, evaluate_voxel_ref(recon, gt, [tau], voxel=voxel), voxel, None)
        crop = (4, 0, -1, 8, 8, 1)
        r = api.evaluate_cloud(rr, gg, [tau], voxel=voxel, crop=crop)
        assert r["accuracy_voxel"].tolist() == [1.0] and (r["n_recon_cropped"], r["n_gt_cropped"]) == (320, 32)
        same_evaluation(r, evaluate_voxel_ref(recon, gt, [tau], voxel=voxel, crop=crop), voxel, crop)
    plain = api.evaluate_cloud(recon, gt, [tau])
    assert sorted(plain) == sorted(["tolerances", "accuracy", "completeness", "f1", "n_accurate", "n_complete", "n_recon_valid", "n_gt_valid", "pairs_accuracy",
                                    "pairs_completeness"])                                         # without the switches: today's dict
    with pytest.raises(ValueError):
        api.evaluate_cloud(recon, gt, [tau], crop=(1, 0, 0, 0, 1, 1))


def test_evaluate_a_patchmatch_cloud_equals_the_restatement(scene_clouds):
    gt, pm, footprint = scene_clouds
    tol = [F(0.5 * footprint), F(2 * footprint), F(8 * footprint)]
    voxel = F(6 * footprint)
    lo, hi = gt[:, :3].min(axis=0), gt[:, :3].max(axis=0)
    crop = tuple((lo + F(0.1) * (hi - lo)).tolist()) + tuple((hi - F(0.15) * (hi - lo)).tolist())
    for v, cr in ((voxel, None), (voxel, crop), (None, crop)):
        ref = evaluate_voxel_ref(pm, gt, tol, voxel=v, crop=cr)
        r = api.evaluate_cloud(pm, gt, tol, voxel=v, crop=cr)
        same_evaluation(r, ref, v, cr)
        if v is not None:
            assert 100 < ref["n_recon_voxels"] < len(pm) and 0 < ref["accuracy_voxel"][0] < ref["accuracy_voxel"][2] <= 1
            # the integer arrays behind the ratios, through the operator itself (the cropped cloud and its distances are the restatement's)
            got = api.cloud_voxels(ref["recon_cloud"], v, ref["recon_dist2"], tol)
            for k in ("rank", "rep", "count", "within"):
                assert np.array_equal(got[k], ref["recon_voxels"][k]), k
        if cr is not None:
            assert 0 < ref["n_recon_cropped"] < len(pm) and 0 < ref["n_gt_cropped"] < len(gt)
    # a cloud against itself scores 1.0 at every tolerance, point-wise and voxel-averaged
    r = api.evaluate_cloud(torch.from_numpy(pm).cuda(), torch.from_numpy(pm).cuda(), tol, voxel=voxel, crop=crop)
    for k in ("accuracy", "completeness", "f1", "accuracy_voxel", "completeness_voxel", "f1_voxel"):
        assert r[k].tolist() == [1.0] * 3, k


def test_the_evaluate_tool_with_voxel_and_crop(scene_clouds, tmp_path):
    gt, pm, footprint = scene_clouds
    a, b = str(tmp_path / "pm.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, pm)
    tio.write_ply(b, gt, binary=False)
    tol = [F(0.5 * footprint), F(4 * footprint)]
    voxel = F(5 * footprint)
    lo, hi = gt[:, :3].min(axis=0), gt[:, :3].max(axis=0)
    crop = [float(F(v)) for v in (lo + F(0.1) * (hi - lo)).tolist() + (hi - F(0.1) * (hi - lo)).tolist()]
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate")
    out = subprocess.run([tool, a, b, "--tolerances=%.9g,%.9g" % tuple(tol), "--voxel=%.9g" % voxel, "--crop=" + ",".join("%.9g" % v for v in crop)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    r = api.evaluate_cloud(pm, gt, tol, voxel=voxel, crop=crop)
    for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1", "accuracy_voxel", "completeness_voxel", "f1_voxel"):
        assert rec[k] == r[k].tolist(), k
    for k in ("n_recon_valid", "n_gt_valid", "n_recon_voxels", "n_gt_voxels", "n_recon_cropped", "n_gt_cropped", "pairs_accuracy", "pairs_completeness"):
        assert rec[k] == r[k], k
    assert F(rec["voxel"]) == voxel and [F(v) for v in rec["crop"]] == [F(v) for v in crop] and 0 < rec["n_recon_cropped"] < len(pm)
    same_evaluation(r, evaluate_voxel_ref(pm, gt, tol, voxel=voxel, crop=crop), voxel, crop)


def read_fused_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("element vertex")][0].split()[-1])
    assert len(body) == n * 27
    return head.replace(b"element vertex %d" % n, b"element vertex N"), np.frombuffer(body, np.uint8).reshape(n, 27)


def test_tsar_fusion_voxel_writes_the_representatives_rows(small_scene, tmp_path):
    """the PLY with --voxel=V holds exactly the rows sorted(rep) of the PLY the same run writes without it, bit for bit"""
    root = str(tmp_path) + "/"
    tio.export_scene(small_scene, root)
    cli, fusion = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma"), os.path.join(ROOT, "tsar-mvs_amd", "tsar_fusion")
    out = subprocess.run([cli, "--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=2", "--blocksize=11", "--n_best=1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([fusion, root, "--num_consistent=1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    plain_bytes = open(root + "APD/APD_TSAR.ply", "rb").read()
    head, full = read_fused_ply(root + "APD/APD_TSAR.ply")
    shutil.copy(root + "APD/APD_TSAR.ply", root + "full.ply")
    xyz = np.ascontiguousarray(full[:, :12]).view("<f4").reshape(-1, 3)
    assert len(xyz) > 1000
    V = float(F(0.02) * F(np.ptp(xyz[:, 0])))
    out = subprocess.run([fusion, root, "--num_consistent=1", "--voxel=%.9g" % V], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ref = cloud_voxels_ref(xyz, F(V))
    assert 100 < ref["n_voxels"] < 0.9 * len(xyz)                                              # the case thins something, and not to nothing
    head_v, thin = read_fused_ply(root + "APD/APD_TSAR.ply")
    assert head_v == head and np.array_equal(thin, full[np.sort(ref["rep"])])
    assert "%d points -> %d voxels" % (len(xyz), ref["n_voxels"]) in out.stdout                   # the counts before and after
    out = subprocess.run([fusion, root, "--num_consistent=1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and open(root + "APD/APD_TSAR.ply", "rb").read() == plain_bytes and "voxels" not in out.stdout
    for bad in ("0", "-1", "nan", "inf", "x"):
        out = subprocess.run([fusion, root, "--voxel=" + bad], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stderr == "--voxel=V must be a finite number > 0\n"

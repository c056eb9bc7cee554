"""tsar_cloud_neighbors on the GPU against the numpy restatement (tests/cloud_neighbors_ref.py): exact equality of `count`, np.array_equal on
the raw bits of `knn_dist2`, over sizes, strides, memory spaces, list lengths that do and do not fill their template's list, a dense cell,
lattice ties, cell borders, duplicates, non-finite records, a flat cloud and a far point; permutation, repeatability, the contexts left
alone, every refusal; api.remove_outliers and api.evaluate_cloud(clean=) on host and device inputs; the stray scene; tsar_fusion
--outlier_radius=."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from cloud_distance_ref import cloud_distance_ref
from cloud_neighbors_ref import cloud_neighbors_ref, evaluate_clean_ref, remove_outliers_ref, stray_scene
from cloud_voxels_ref import cloud_voxels_ref, evaluate_voxel_ref
from tsar_mvs_amd import api
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("strict", False, 3), ("fast", True, 9), ("fast", False, 9), ("strict", True, 3))       # (context, device memory, stride)
KS = (0, 1, 4, 5, 8, 17, 32)                                              # 5 and 17 do not fill their template's list (8, 32)


@pytest.fixture(scope="module")
def ctxs(small_scene):
    """a strict and a fast context, each holding views, a plane state and a result: the operator must run on them and leave them alone"""
    ms = {}
    for name, flags in (("strict", api.FLAG_STRICT_DIV), ("fast", 0)):
        m = api.matcher_from_scene(small_scene, seed=5, flags=flags)
        m.pm_init()
        m.compute_disp()
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


def padded(a, stride):
    out = np.full((len(a), stride), np.nan, F)                           # (what follows x y z is not read: NaN there changes nothing)
    out[:, :3] = a[:, :3]
    return out


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint32)


def check(ctxs, cloud, R, ks=(0, 8, 32), modes=MODES):
    """the operator against the restatement: every count, every bit of every distance, for each k the first k columns of the reference"""
    cloud = np.ascontiguousarray(cloud, F)
    ref = cloud_neighbors_ref(cloud, R, 32)
    for name, on_device, stride in modes:
        c = padded(cloud, stride)
        if on_device:
            c = torch.from_numpy(c).cuda()
        for k in ks:
            r = api.cloud_neighbors(c, R, k, matcher=ctxs[name])
            where = "(%s, device %s, stride %d, k %d)" % (name, on_device, stride, k)
            assert (r["n_valid"], r["pairs"]) == (ref["n_valid"], ref["pairs"]), where
            got = host(r["count"])
            assert torch.is_tensor(r["count"]) == on_device and got.dtype == np.int32 and got.shape == (len(cloud),)
            assert np.array_equal(got, ref["count"]), "count differs in %d of %d %s" % (np.count_nonzero(got != ref["count"]), got.size, where)
            assert ("knn_dist2" in r) == (k > 0)
            if k:
                got = host(r["knn_dist2"])
                assert got.dtype == F and got.shape == (len(cloud), k)
                want = ref["knn_dist2"][:, :k]
                assert np.array_equal(bits(got), bits(want)), "knn_dist2 differs in %d of %d rows %s" % (np.count_nonzero((bits(got) != bits(want)).any(axis=1)), len(got), where)
    return ref


# ---- sizes, strides, memory, list lengths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 3000])
def test_uniform_box_sizes_and_every_list_length(ctxs, n):
    rng = np.random.default_rng(100 + n)
    cloud = rng.random((n, 3), dtype=F) - F(0.25)                        # (some coordinates negative)
    R = 0.15 if n == 3000 else 0.45                                      # about 40 neighbours in the large cloud: lists of 32 fill for most, not for all
    ref = check(ctxs, cloud, R, ks=KS)
    if n == 3000:
        assert (ref["count"] > 32).sum() > 1000 and (ref["count"] < 17).sum() > 50 and ref["pairs"] < n * n // 2
    if n in (1, 2):
        assert ref["count"].max() <= n - 1


def test_a_dense_cluster_in_one_cell(ctxs):
    """400 points within half a cell edge of each other: more than a wave shares one cell, and every list of 32 overflows many times"""
    rng = np.random.default_rng(1)
    cloud = np.concatenate([F(0.2) + F(0.45) * rng.random((400, 3), dtype=F), F(4) * rng.random((150, 3), dtype=F)])
    ref = check(ctxs, cloud, 1.0, ks=(1, 4, 8, 32))
    assert (ref["count"][:400] >= 399).all() and np.isfinite(ref["knn_dist2"][:400]).all()


@pytest.mark.parametrize("d2", [1, 2, 3])
def test_an_integer_lattice_is_all_ties(ctxs, d2):
    r = F(np.sqrt(F(d2)))
    while F(r * r) < F(d2):
        r = np.nextafter(r, F(np.inf))
    p = np.array([[x, y, z] for z in range(7) for y in range(7) for x in range(7)], F)
    ref = check(ctxs, p, r, ks=(5, 8, 32))
    assert ref["count"][3 + 7 * 3 + 49 * 3] == {1: 6, 2: 18, 3: 26}[d2] and len(np.unique(ref["knn_dist2"][np.isfinite(ref["knn_dist2"])])) == d2


def test_points_on_cell_borders_and_pairs_at_exactly_the_radius(ctxs):
    """R = 0.5: the cell edge R (1 + 2^-10) = 1025 / 2048 is a float32, so multiples of it lie exactly on cell borders, and a shift by
    exactly R gives pairs with d2 == R2"""
    R, e = F(0.5), F(1025.0 / 2048.0)
    assert np.float64(e) == np.float64(R) * (1.0 + 2.0 ** -10)
    steps = np.concatenate([np.arange(5, dtype=F) * e, np.arange(5, dtype=F) * e + R, np.arange(1, 5, dtype=F) * e - R])
    rng = np.random.default_rng(2)
    cloud = np.concatenate([np.zeros((1, 3), F), steps[rng.integers(0, len(steps), (900, 3))]])         # (the origin is a point: the borders are where they seem)
    ref = check(ctxs, cloud, R, ks=(4, 17))
    assert (ref["knn_dist2"] == F(0.25)).sum() > 100 and (ref["knn_dist2"] == 0).sum() > 10            # pairs at exactly R; duplicates


def test_duplicates_count_and_the_point_itself_does_not(ctxs):
    rng = np.random.default_rng(3)
    base = rng.random((150, 3), dtype=F)
    cloud = np.concatenate([base, base, base[:50], np.repeat(base[:1], 40, axis=0)])
    ref = check(ctxs, cloud[rng.permutation(len(cloud))], 0.2, ks=(1, 8, 32))
    assert (ref["knn_dist2"][:, 0] == 0).all() and (ref["knn_dist2"][:, 31] == 0).sum() == 43          # base[0]: 3 + 40 copies, each sees 42 others
    assert not np.signbit(ref["knn_dist2"]).any()


def test_non_finite_records(ctxs):
    rng = np.random.default_rng(4)
    cloud = rng.random((700, 3), dtype=F)
    bad = rng.choice(700, 90, replace=False)
    cloud[bad, rng.integers(0, 3, 90)] = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, 90)]
    ref = check(ctxs, cloud, 0.2, ks=(0, 5, 32))
    assert ref["n_valid"] == 610 and (ref["count"][bad] == -1).all() and np.isposinf(ref["knn_dist2"][bad]).all()
    ref = check(ctxs, cloud[bad], 0.2, ks=(0, 4))                        # no candidate at all
    assert ref["n_valid"] == 0 and ref["pairs"] == 0 and (ref["count"] == -1).all()


def test_a_flat_cloud_a_line_and_one_far_point(ctxs):
    rng = np.random.default_rng(5)
    flat = rng.random((600, 3), dtype=F)
    flat[:, 2] = F(0.25)                                                 # one cell on z
    check(ctxs, flat, 0.08, ks=(8,))
    line = np.zeros((300, 3), F)
    line[:, 1] = rng.random(300, dtype=F)                                # one cell on x and z
    check(ctxs, line, 0.02, ks=(4, 32))
    # alone in its cell, 499 512 cells of edge R (1 + 2^-10) away on every axis: below 2^20, so the call is not refused
    far = np.concatenate([F(0.1) * rng.random((300, 3), dtype=F), np.full((1, 3), 5000, F)])
    ref = check(ctxs, far, 0.01, ks=(0, 8))
    assert ref["count"][-1] == 0 and np.isposinf(ref["knn_dist2"][-1]).all() and 5000 / (0.01 * (1 + 2.0 ** -10)) < (1 << 20)


# ---- the three grid operators in turn on one context ----------------------------------------------------------------------------------------
def test_voxels_distance_neighbors_and_voxels_again_on_one_context(ctxs):
    """The operators share the measuring of a cloud and the sorted index of its cells (cloud_grid.hip), and on one context the same arena:
    nothing of one call may reach the next.  257 points, rows 100..102 a NaN, a +inf and a -inf beside the finite row 103, the last point far
    off (the grid is mostly empty cells): every call counts the same 254 candidates, every array is the restatement's bit for bit, and the
    voxel result after the two searches is the one before them."""
    rng = np.random.default_rng(11)
    cloud = rng.random((257, 3), dtype=F)
    cloud[100, 1], cloud[101, 0], cloud[102, 2] = np.nan, np.inf, -np.inf
    cloud[256] = 300                                                      # 2000 cells of edge R, 3000 voxels away on every axis
    R, V, m = 0.15, 0.1, ctxs["fast"]
    dref, nref, vref = cloud_distance_ref(cloud, cloud, R), cloud_neighbors_ref(cloud, R, 4), cloud_voxels_ref(cloud, V)
    assert dref["n_valid_query"] == nref["n_valid"] == vref["n_valid"] == 254 and vref["n_voxels"] > 100 and vref["rank"][103] >= 0
    for on_device in (False, True):
        c = torch.from_numpy(cloud).cuda() if on_device else cloud
        v1 = api.cloud_voxels(c, V, matcher=m)
        d = api.cloud_distance(c, c, R, matcher=m)
        nb = api.cloud_neighbors(c, R, 4, matcher=m)
        v2 = api.cloud_voxels(c, V, matcher=m)
        assert v1["n_valid"] == d["n_valid_query"] == nb["n_valid"] == v2["n_valid"] == 254, on_device
        assert v1["n_voxels"] == v2["n_voxels"] == vref["n_voxels"] and nb["pairs"] == nref["pairs"], on_device
        for k in ("rank", "rep", "count"):
            assert np.array_equal(host(v1[k]), vref[k]) and np.array_equal(host(v2[k]), host(v1[k])), (k, on_device)
        assert np.array_equal(bits(d["dist2"]), bits(dref["dist2"])) and np.array_equal(host(d["index"]), dref["index"]), on_device
        assert np.array_equal(host(nb["count"]), nref["count"]) and np.array_equal(bits(nb["knn_dist2"]), bits(nref["knn_dist2"])), on_device


# ---- order and repeatability ----------------------------------------------------------------------------------------------------------------
def test_a_shuffled_cloud_gives_the_same_outputs_permuted_and_two_runs_the_same_bits(ctxs):
    rng = np.random.default_rng(6)
    cloud = np.concatenate([rng.random((2500, 3), dtype=F), np.repeat(rng.random((20, 3), dtype=F), 5, axis=0)])
    cloud[17] = np.nan
    m = ctxs["fast"]
    a = api.cloud_neighbors(cloud, 0.12, 32, matcher=m)
    b = api.cloud_neighbors(cloud, 0.12, 32, matcher=m)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(bits(a["knn_dist2"]), bits(b["knn_dist2"])) and a["pairs"] == b["pairs"]
    perm = rng.permutation(len(cloud))
    for dev in (False, True):
        c = cloud[perm]
        s = api.cloud_neighbors(torch.from_numpy(c).cuda() if dev else c, 0.12, 32, matcher=m)
        assert np.array_equal(host(s["count"]), a["count"][perm]) and np.array_equal(bits(s["knn_dist2"]), bits(a["knn_dist2"][perm]))
        assert (s["n_valid"], s["pairs"]) == (a["n_valid"], a["pairs"])


def test_the_first_distance_is_the_nearest_other_point(ctxs):
    """knn_dist2[:, 0] is what tsar_cloud_distance would give for the point against the cloud WITHOUT it.  cloud_distance(cloud, cloud)
    itself finds the point (distance 0), so the check goes through the restatement of that operator, one point against the rest at a time,
    not through api.cloud_distance."""
    rng = np.random.default_rng(7)
    cloud = rng.random((300, 3), dtype=F)
    assert len(np.unique(cloud, axis=0)) == 300                          # duplicate-free
    got = api.cloud_neighbors(cloud, 0.1, 1, matcher=ctxs["strict"])["knn_dist2"][:, 0]
    want = np.array([cloud_distance_ref(cloud[i:i + 1], np.delete(cloud, i, axis=0), 0.1)["dist2"][0] for i in range(300)], F)
    assert np.array_equal(bits(got), bits(want)) and np.isfinite(want).sum() > 100 and np.isposinf(want).sum() > 10


def test_want_names_the_outputs_and_a_context_is_made_when_none_is_given():
    rng = np.random.default_rng(8)
    cloud = rng.random((500, 3), dtype=F)
    ref = cloud_neighbors_ref(cloud, 0.2, 4)
    r = api.cloud_neighbors(cloud, 0.2, 4, want=("knn_dist2",))
    assert "count" not in r and np.array_equal(bits(r["knn_dist2"]), bits(ref["knn_dist2"]))
    r = api.cloud_neighbors(torch.from_numpy(cloud).cuda(), 0.2, 4, want=("count",))
    assert "knn_dist2" not in r and r["count"].is_cuda and np.array_equal(host(r["count"]), ref["count"])
    r = api.cloud_neighbors(cloud, 0.2, want=())
    assert sorted(r) == ["n_valid", "pairs"] and r["pairs"] == ref["pairs"]


def test_the_contexts_are_left_as_they_were(ctxs):
    """get_plane and get_result before and after are bit-equal, after calls that succeed and calls that are refused, and the matcher goes on"""
    rng = np.random.default_rng(9)
    c = rng.random((5000, 3), dtype=F)
    state = lambda m: [np.asarray(a).view(np.uint32).copy() for a in m.get_plane()] + [v.view(np.uint32).copy() for _, v in sorted(m.get_result().items())]
    for m in ctxs.values():
        before = state(m)
        api.cloud_neighbors(c, 0.05, 32, matcher=m)
        api.cloud_neighbors(torch.from_numpy(c).cuda(), 0.1, 0, matcher=m)
        with pytest.raises(api.TsarError):
            api.cloud_neighbors(c, 1e-8, 4, matcher=m)
        with pytest.raises(api.TsarError):
            api.cloud_neighbors(c, 0.5, 4, max_pairs=10, matcher=m)
        api.remove_outliers(c, 0.05, min_neighbors=2, k=3, matcher=m)
        api.evaluate_cloud(c, c[::2], [0.05], clean=dict(radius=0.05, k=4), matcher=m)
        assert all(np.array_equal(a, b) for a, b in zip(before, state(m)))
        m.pm_iterate(1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_context_works_afterwards(ctxs):
    m = ctxs["strict"]
    L = m.L
    rng = np.random.default_rng(10)
    c = rng.random((500, 3), dtype=F)
    cp = c.ctypes.data_as(C.c_void_p)
    cnt, knn = np.full(500, -7, np.int32), np.full((500, 4), -7, F)
    cntp, knnp = cnt.ctypes.data_as(C.c_void_p), knn.ctypes.data_as(C.c_void_p)
    n_valid, pairs = C.c_int64(-1), C.c_int64(-1)
    P = api.CloudNeighborsParams

    def call(cloud=cp, n=500, stride=3, prm=P(0.1, 4, 1 << 40), count=cntp, out=knnp, mem=api.MEM_HOST):
        rc = L.tsar_cloud_neighbors_ctx(m._ctx, cloud, n, stride, C.byref(prm) if prm is not None else None, count, out, C.byref(n_valid), C.byref(pairs), mem)
        return rc, L.tsar_last_error(m._ctx).decode()

    def refused(fragment, **kw):
        rc, msg = call(**kw)
        assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_neighbors:") and fragment in msg, (rc, msg)
        assert (cnt == -7).all() and (knn == -7).all() and n_valid.value == -1                        # a refused call writes nothing

    refused("params is NULL", prm=None)
    refused("mem must be", mem=7)
    refused("stride", stride=2)
    refused("n must be", n=-1)
    refused("n must be", n=1 << 31)
    for R in (0.0, -1.0, np.inf, -np.inf, np.nan, 1e30, 1e-30):                                       # 1e30, 1e-30: fl(R * R) is +inf, 0
        refused("radius must be finite and > 0", prm=P(R, 4, 1 << 40))
    refused("k must be in 0..", prm=P(0.1, -1, 1 << 40))
    refused("k must be in 0..", prm=P(0.1, 33, 1 << 40))
    refused("knn_dist2_out needs k > 0", prm=P(0.1, 0, 1 << 40))
    refused("max_pairs must be >= 0", prm=P(0.1, 4, -1))
    assert pairs.value == -1
    far = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [0, 2e4, 0]], F)                                       # 2e4 / 0.01 >= 2^20 cells on y
    refused("2^20 cells or more", cloud=far.ctypes.data_as(C.c_void_p), n=3, prm=P(0.01, 4, 1 << 40))
    with pytest.raises(api.TsarError) as e:
        api.cloud_neighbors(far, 0.01, 4, matcher=m)
    assert e.value.code == api.TSAR_ERR_INVALID and "2^20 cells" in str(e.value) and e.value.pairs is None
    # more than max_pairs pairs: *pairs_out is filled, nothing else is written
    want_pairs = cloud_neighbors_ref(c, 0.1)["pairs"]
    refused("more than max_pairs", prm=P(0.1, 4, want_pairs - 1))
    assert pairs.value == want_pairs
    with pytest.raises(api.TsarError) as e:
        api.cloud_neighbors(torch.from_numpy(c).cuda(), 0.1, 4, max_pairs=want_pairs - 1, matcher=m)
    assert e.value.code == api.TSAR_ERR_INVALID and e.value.pairs == want_pairs
    assert api.cloud_neighbors(c, 0.1, 4, max_pairs=want_pairs, matcher=m)["pairs"] == want_pairs     # exactly max_pairs pass
    rc, _ = call()
    assert rc == api.TSAR_OK and n_valid.value == 500 and pairs.value == want_pairs and (cnt >= 0).all()
    with pytest.raises(AssertionError):
        api.cloud_neighbors(c[:, :2], 0.1, matcher=m)
    check(ctxs, c, 0.1)                                                                                # and the contexts still work


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
RULES = [dict(min_neighbors=6), dict(k=8, ratio=2.0), dict(min_neighbors=3, k=4, ratio=1.5), dict(k=32, ratio=3.0)]


@pytest.fixture(scope="module")
def scene():
    """the stray scene with a fourth column that rides along and two non-finite records"""
    s = np.concatenate([stray_scene(), np.arange(3200, dtype=F)[:, None]], axis=1)
    s[40, 0] = np.nan
    s[3100, 2] = np.inf
    return s


@pytest.mark.parametrize("rules", RULES, ids=lambda r: "-".join("%s%g" % kv for kv in r.items()))
def test_remove_outliers_equals_the_restatement(ctxs, scene, rules):
    ref_rows, ref_keep = remove_outliers_ref(scene, 0.06, **rules)
    assert 1500 < ref_keep.sum() < 3150                                   # the rule removes something, and not all
    for dev in (False, True):
        c = torch.from_numpy(scene).cuda() if dev else scene
        rows, keep = api.remove_outliers(c, 0.06, return_mask=True, matcher=ctxs["fast"], **rules)
        assert torch.is_tensor(rows) == dev and torch.is_tensor(keep) == dev
        assert host(keep).dtype == bool and np.array_equal(host(keep), ref_keep)                       # the mask
        assert np.array_equal(bits(rows), bits(ref_rows))                                              # whole records, the cloud's own order
        assert np.array_equal(bits(api.remove_outliers(c, 0.06, **rules)), bits(ref_rows))            # a context of its own
    empty = api.remove_outliers(scene, 1e-5, k=2, matcher=ctxs["fast"])                                # no finite k-th distance: nothing passes
    assert empty.shape == (0, 4)
    with pytest.raises(ValueError):
        api.remove_outliers(scene, 0.06)


def test_it_removes_the_strays_and_keeps_the_surface(ctxs):
    """the issue's scene: 3000 surface points, 200 strays.  The restatement's figures (3000 / 177 and 3000 / 178) were worked on the CPU; the GPU
    result equals the restatement exactly, and clears the bars it clears with room."""
    cloud = stray_scene()
    for rules, removed in ((dict(min_neighbors=6), 177), (dict(k=8, ratio=2.0), 178)):
        ref_rows, ref_keep = remove_outliers_ref(cloud, 0.06, **rules)
        assert ref_keep[:3000].sum() == 3000 and (~ref_keep[3000:]).sum() == removed
        for c in (cloud, torch.from_numpy(cloud).cuda()):
            rows, keep = api.remove_outliers(c, 0.06, return_mask=True, matcher=ctxs["strict"], **rules)
            keep = host(keep)
            assert np.array_equal(keep, ref_keep) and np.array_equal(bits(rows), bits(ref_rows))
            assert keep[:3000].mean() >= 0.99 and (~keep[3000:]).mean() >= 0.8
    gt, tol = cloud[:3000], [0.01]
    plain = api.evaluate_cloud(cloud, gt, tol, matcher=ctxs["fast"])
    for clean, removed in ((dict(radius=0.06, min_neighbors=6), 177), (dict(radius=0.06, k=8, ratio=2.0), 178)):
        r = api.evaluate_cloud(cloud, gt, tol, clean=clean, matcher=ctxs["fast"])
        assert r["accuracy"][0] > plain["accuracy"][0] and r["completeness"][0] == plain["completeness"][0] == 1.0      # strictly higher at tau = 0.01
        assert r["n_recon_cleaned"] == removed and r["n_recon_valid"] == 3200 - removed


@pytest.mark.parametrize("more", [{}, {"voxel": 0.1, "crop": (0.1, 0.0, 0.0, 0.9, 1.0, 1.0)}], ids=["plain", "voxel-crop"])
def test_evaluate_cloud_clean_equals_the_restatement(scene, more):
    recon, gt, tol = scene[::2], scene[1:3000:3], [0.01, 0.03]
    plain = api.evaluate_cloud(recon, gt, tol, **more)
    assert "clean" not in plain and "n_recon_cleaned" not in plain                                     # None, the default: the call as it was
    for clean in (dict(radius=0.1, min_neighbors=6), dict(radius=0.1, k=8), dict(radius=0.1, min_neighbors=2, k=3, ratio=1.5)):
        ref = evaluate_clean_ref(recon, gt, tol, clean, **more)
        assert 50 < ref["n_recon_cleaned"] < 800
        for dev in (False, True):
            r = api.evaluate_cloud(*((torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (recon, gt)) if dev else (recon, gt)), tol, clean=clean, **more)
            for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1") + (("accuracy_voxel", "completeness_voxel", "f1_voxel") if more else ()):
                assert r[k].tolist() == ref[k].tolist(), k
            for k in ("n_recon_valid", "n_gt_valid", "n_recon_cleaned") + (("n_recon_voxels", "n_gt_voxels", "n_recon_cropped", "n_gt_cropped") if more else ()):
                assert r[k] == ref[k], k
            assert r["clean"] == {"radius": clean["radius"], "min_neighbors": clean.get("min_neighbors"), "k": clean.get("k"), "ratio": clean.get("ratio", 2.0)}
            assert sorted(set(r) - set(plain)) == ["clean", "n_recon_cleaned"]
    with pytest.raises(ValueError):
        api.evaluate_cloud(recon, gt, tol, clean=dict(radius=0.1))


def test_the_evaluate_tool_cleans_like_the_binding(scene, tmp_path):
    recon, gt = scene[::2, :3], scene[1:3000:3, :3]
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt)
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate")
    out = subprocess.run([tool, a, b, "--tolerances=0.01,0.03", "--clean_radius=0.1", "--clean_min_neighbors=2", "--clean_knn=3", "--clean_ratio=1.5"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    ref = evaluate_clean_ref(recon, gt, [0.01, 0.03], dict(radius=0.1, min_neighbors=2, k=3, ratio=1.5))
    for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1"):
        assert rec[k] == ref[k].tolist(), k
    assert rec["n_recon_cleaned"] == ref["n_recon_cleaned"] > 50 and rec["n_recon_valid"] == ref["n_recon_valid"]
    assert F(rec["clean"].pop("radius")) == F(0.1) and rec["clean"] == {"min_neighbors": 2, "k": 3, "ratio": 1.5}       # (%.9g names the float32)


def read_fused_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("element vertex")][0].split()[-1])
    assert len(body) == n * 27
    return head.replace(b"element vertex %d" % n, b"element vertex N"), np.frombuffer(body, np.uint8).reshape(n, 27)


def test_tsar_fusion_outlier_radius_writes_the_kept_rows(small_scene, tmp_path):
    """the PLY with --outlier_radius= holds exactly the api.remove_outliers rows of the cloud the same run writes without it, bit for bit;
    with --voxel= as well, the cleaning comes first"""
    root = str(tmp_path) + "/"
    tio.export_scene(small_scene, root)
    cli, fusion = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma"), os.path.join(ROOT, "tsar-mvs_amd", "tsar_fusion")
    out = subprocess.run([cli, "--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=2", "--blocksize=11", "--n_best=1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([fusion, root, "--num_consistent=1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--outlier_radius" not in out.stdout, out.stdout + out.stderr
    head, full = read_fused_ply(root + "APD/APD_TSAR.ply")
    xyz = np.ascontiguousarray(full[:, :12]).view("<f4").reshape(-1, 3)
    assert len(xyz) > 1000
    R = float(F(0.02) * F(np.ptp(xyz[:, 0])))
    # both rules (and the reference's "--opt= VALUE" spelling)
    rules = dict(min_neighbors=3, k=6, ratio=1.5)
    out = subprocess.run([fusion, root, "--num_consistent=1", "--outlier_radius=%.9g" % R, "--outlier_min_neighbors=", "3", "--outlier_knn=6", "--outlier_ratio=1.5"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows, keep = api.remove_outliers(xyz, F(R), return_mask=True, **rules)
    assert np.array_equal(keep, remove_outliers_ref(xyz, F(R), **rules)[1]) and 100 < keep.sum() < len(xyz)            # the case removes something, and not all
    head_c, clean = read_fused_ply(root + "APD/APD_TSAR.ply")
    assert head_c == head and np.array_equal(clean, full[keep])
    assert "--outlier_radius=%g: %d points -> %d points" % (F(R), len(xyz), keep.sum()) in out.stdout
    # with --voxel as well: the cleaned cloud is thinned, not the thinned cloud cleaned
    rules, V = dict(min_neighbors=5), float(F(2) * F(R))
    out = subprocess.run([fusion, root, "--num_consistent=1", "--voxel=%.9g" % V, "--outlier_radius=%.9g" % R, "--outlier_min_neighbors=5"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    keep = remove_outliers_ref(xyz, F(R), **rules)[1]
    rep = np.sort(cloud_voxels_ref(xyz[keep], F(V))["rep"])
    _, both = read_fused_ply(root + "APD/APD_TSAR.ply")
    assert np.array_equal(both, full[keep][rep])
    thinned_first = xyz[np.sort(cloud_voxels_ref(xyz, F(V))["rep"])]
    assert len(both) != remove_outliers_ref(thinned_first, F(R), **rules)[1].sum()                    # (the other order gives another cloud here)
    assert out.stdout.index("--outlier_radius=") < out.stdout.index("--voxel=")
    for args, msg in ((["--outlier_radius=0.1"], "--outlier_radius=R needs --outlier_min_neighbors=N, --outlier_knn=K or both"),
                      (["--outlier_radius=0.1", "--outlier_min_neighbors=0"], "--outlier_min_neighbors=N must be an integer >= 1"),
                      (["--outlier_radius=0.1", "--outlier_knn=33"], "--outlier_knn=K must be an integer in 1..32"),
                      (["--outlier_radius=0.1", "--outlier_knn=0"], "--outlier_knn=K must be an integer in 1..32"),
                      (["--outlier_radius=0.1", "--outlier_knn=3", "--outlier_ratio=0"], "--outlier_ratio=Q must be a finite number > 0"),
                      (["--outlier_radius=0.1", "--outlier_knn=3", "--outlier_ratio=nan"], "--outlier_ratio=Q must be a finite number > 0"),
                      (["--outlier_radius=0", "--outlier_knn=3"], "--outlier_radius=R must be a finite number > 0"),
                      (["--outlier_radius=inf", "--outlier_knn=3"], "--outlier_radius=R must be a finite number > 0"),
                      (["--outlier_radius=x", "--outlier_knn=3"], "--outlier_radius=R must be a finite number > 0"),
                      (["--outlier_knn=3"], "--outlier_min_neighbors=, --outlier_knn= and --outlier_ratio= need --outlier_radius=R"),
                      (["--outlier_min_neighbors=3"], "--outlier_min_neighbors=, --outlier_knn= and --outlier_ratio= need --outlier_radius=R"),
                      (["--outlier_ratio=3"], "--outlier_min_neighbors=, --outlier_knn= and --outlier_ratio= need --outlier_radius=R")):
        out = subprocess.run([fusion, root] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stderr == msg + "\n", (args, out.stderr)

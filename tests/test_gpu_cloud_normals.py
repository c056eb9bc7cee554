"""tsar_cloud_normals and tsar_cloud_normal_compare on the GPU against the numpy restatement (tests/cloud_normals_ref.py): exact equality of
the integer outputs, np.array_equal on the raw bits of normal, curvature and cov, over sizes, strides, memory spaces, every list length
and the first k past it, the min_neighbors boundary, lattice ties, a dense cell, cell borders, duplicates, non-finite records, degenerate
clouds, the three orientation modes; permutation, repeatability, the contexts left alone, every refusal; normal_compare's exclusions;
api.evaluate_cloud(normals=) and the built tsar_evaluate --normals= on the stray scene.  Quality bars are held on the CPU (test_cloud_normals_cpu.py): equality carries them over."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from cloud_normals_ref import cloud_normals_ref, evaluate_normals_ref, normal_compare_ref, stray_surface
from tsar_mvs_amd import api
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("strict", False, 3), ("fast", True, 9), ("fast", False, 9), ("none", True, 3))     # (context, device memory, stride); none: a context of the call's own
KS = (3, 8, 9, 16, 17, 32)                                               # each template instance (8, 16, 32) and the first k past it
WANT = ("knn_index", "n_used", "normal", "curvature", "cov")


@pytest.fixture(scope="module")
def ctxs(small_scene):
    """a strict and a fast context, each holding views, a plane state and a result: the operator must run on them and leave them alone"""
    ms = {"none": None}
    for name, flags in (("strict", api.FLAG_STRICT_DIV), ("fast", 0)):
        m = api.matcher_from_scene(small_scene, seed=5, flags=flags)
        m.pm_init()
        m.compute_disp()
        ms[name] = m
    yield ms
    for m in ms.values():
        if m is not None:
            m.close()


def padded(a, stride):
    """the cloud with `stride` columns: its own columns first, NaN after them (what follows x y z is read by orient 2 only)"""
    out = np.full((len(a), max(stride, a.shape[1])), np.nan, F)
    out[:, :a.shape[1]] = a
    return out


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, ref, where):
    """every output of one call against the restatement's, bit for bit"""
    for key in ("n_valid", "n_normals", "pairs"):
        assert got[key] == ref[key], (key, got[key], ref[key], where)
    for key in WANT:
        g, r = host(got[key]), ref[key]
        assert g.dtype == r.dtype and g.shape == r.shape, (key, g.dtype, g.shape, where)
        assert np.array_equal(bits(g), bits(r)), "%s differs in %d of %d rows %s" % (key, np.count_nonzero((bits(g) != bits(r)).reshape(len(r), -1).any(axis=1)), len(r), where)


def check(ctxs, cloud, R, ks=(8, 32), modes=MODES, **kw):
    """the operator against the restatement for each k and mode; orient "record" keeps the cloud's own columns 3 .. 5"""
    cloud = np.ascontiguousarray(cloud, F)
    orient = {None: 0, "viewpoint": 1, "record": 2}[kw.get("orient")]
    refs = {}
    for k in ks:
        kk = dict(kw, min_neighbors=min(kw.get("min_neighbors", 5), k))
        refs[k] = cloud_normals_ref(cloud, R, k, kk["min_neighbors"], orient, kw.get("viewpoint"))
        for name, on_device, stride in modes:
            c = padded(cloud if orient == 2 else cloud[:, :3], stride)
            if on_device:
                c = torch.from_numpy(c).cuda()
            got = api.cloud_normals(c, R, k, want=WANT, matcher=ctxs[name], **kk)
            assert all(torch.is_tensor(got[key]) == on_device for key in WANT)
            same(got, refs[k], "(%s, device %s, stride %d, k %d)" % (name, on_device, c.shape[1], k))
    return refs


# ---- sizes, strides, memory, list lengths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 3000])
def test_uniform_box_sizes_and_every_list_length(ctxs, n):
    rng = np.random.default_rng(200 + n)
    cloud = rng.random((n, 3), dtype=F) - F(0.25)                        # (some coordinates negative)
    R = 0.15 if n == 3000 else 0.45                                      # about 40 neighbours in the large cloud: lists of 32 fill for most, not for all
    refs = check(ctxs, cloud, R, ks=KS)
    if n == 3000:
        assert (refs[32]["n_used"] == 32).sum() > 1000 and (refs[32]["n_used"] < 17).sum() > 50 and refs[32]["n_normals"] > 2900
    if n < 4:
        assert refs[3]["n_normals"] == 0                                 # at most two neighbours: below min_neighbors = 3


def test_the_min_neighbors_boundary(ctxs):
    """clusters of 7 points (every point has m = 6 = min_neighbors: a normal) and of 6 (m = 5: none), far apart"""
    rng = np.random.default_rng(1)
    cloud = np.concatenate([F(c) + F(0.05) * rng.random((7 if c % 2 else 6, 3), dtype=F) for c in range(40)])
    sizes = np.concatenate([np.full(7 if c % 2 else 6, 7 if c % 2 else 6) for c in range(40)])
    ref = check(ctxs, cloud, 0.2, ks=(8, 16), min_neighbors=6)[8]
    assert np.array_equal(ref["n_used"], sizes - 1) and np.array_equal(ref["curvature"] >= 0, sizes == 7) and ref["n_normals"] == 20 * 7
    assert (ref["normal"][sizes == 6] == 0).all() and (ref["cov"][sizes == 6] == 0).all() and (ref["knn_index"][sizes == 6, :5] >= 0).all()


@pytest.mark.parametrize("d2", [1, 2, 3])
def test_an_integer_lattice_is_all_ties(ctxs, d2):
    r = F(np.sqrt(F(d2)))
    while F(r * r) < F(d2):
        r = np.nextafter(r, F(np.inf))
    p = np.array([[x, y, z] for z in range(6) for y in range(6) for x in range(6)], F)
    ref = check(ctxs, p, r, ks=(5, 8, 32))[32]
    mid = 2 + 6 * 2 + 36 * 2
    assert ref["n_used"][mid] == {1: 6, 2: 18, 3: 26}[d2]
    assert ref["knn_index"][mid, :6].tolist() == [mid - 36, mid - 6, mid - 1, mid + 1, mid + 6, mid + 36]      # six at d2 = 1: the index decides


def test_a_dense_cluster_in_one_cell(ctxs):
    """400 points within half a cell edge of each other: more than a wave shares one cell, and every list of 32 overflows many times"""
    rng = np.random.default_rng(2)
    cloud = np.concatenate([F(0.2) + F(0.45) * rng.random((400, 3), dtype=F), F(4) * rng.random((150, 3), dtype=F)])
    ref = check(ctxs, cloud, 1.0, ks=(8, 32))[32]
    assert (ref["n_used"][:400] == 32).all()


def test_points_on_cell_borders_and_pairs_at_exactly_the_radius(ctxs):
    """R = 0.5: the cell edge R (1 + 2^-10) = 1025 / 2048 is a float32, so multiples of it lie exactly on cell borders, and a shift by
    exactly R gives pairs with d2 == R2 (many ties: the index rule decides)"""
    R, e = F(0.5), F(1025.0 / 2048.0)
    steps = np.concatenate([np.arange(5, dtype=F) * e, np.arange(5, dtype=F) * e + R, np.arange(1, 5, dtype=F) * e - R])
    rng = np.random.default_rng(3)
    cloud = np.concatenate([np.zeros((1, 3), F), steps[rng.integers(0, len(steps), (900, 3))]])
    ref = check(ctxs, cloud, R, ks=(17, 32))[32]
    j, ok = ref["knn_index"], ref["knn_index"] >= 0
    d = ((cloud[np.where(ok, j, 0)] - cloud[:, None, :]) ** 2).sum(axis=2)
    assert (ok & (d == F(0.25))).sum() > 100                             # neighbours at exactly R are listed


def test_duplicates_count_and_the_point_itself_does_not(ctxs):
    rng = np.random.default_rng(4)
    base = rng.random((150, 3), dtype=F)
    cloud = np.concatenate([base, base, base[:50], np.repeat(base[:1], 40, axis=0)])
    cloud = cloud[rng.permutation(len(cloud))]
    ref = check(ctxs, cloud, 0.2, ks=(8, 32))[32]
    assert (ref["knn_index"] != np.arange(len(cloud))[:, None]).all()
    assert (cloud[ref["knn_index"][:, 0]] == cloud).all()                # the nearest is a duplicate, at d2 = 0
    heap = (cloud == base[0]).all(axis=1)                                # 43 copies of one point: all 32 slots are duplicates, cov is 0 exactly
    assert heap.sum() == 43 and (ref["cov"][heap] == 0).all() and (ref["curvature"][heap] == 0).all() and (ref["n_used"][heap] == 32).all()


def test_non_finite_records(ctxs):
    rng = np.random.default_rng(5)
    cloud = rng.random((700, 3), dtype=F)
    bad = rng.choice(700, 90, replace=False)
    cloud[bad, rng.integers(0, 3, 90)] = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, 90)]
    ref = check(ctxs, cloud, 0.2, ks=(9, 32))[32]
    assert ref["n_valid"] == 610 and (ref["n_used"][bad] == -1).all() and (ref["knn_index"][bad] == -1).all() and (ref["curvature"][bad] == -1).all()
    assert not np.isin(ref["knn_index"], bad).any()
    ref = check(ctxs, cloud[bad], 0.2, ks=(3,))[3]                       # no candidate at all
    assert ref["n_valid"] == 0 and ref["pairs"] == 0 and ref["n_normals"] == 0


def test_a_flat_cloud_a_line_and_one_far_point(ctxs):
    rng = np.random.default_rng(6)
    flat = rng.random((600, 3), dtype=F)
    flat[:, 2] = F(0.25)                                                 # one cell on z; the normal is +z exactly, curvature 0
    ref = check(ctxs, flat, 0.08, ks=(8,))[8]
    has = ref["curvature"] >= 0
    assert has.sum() > 300 and (ref["normal"][has] == np.array([0, 0, 1], F)).all() and (ref["curvature"][has] == 0).all()
    line = np.zeros((300, 3), F)
    line[:, 1] = rng.random(300, dtype=F)                                # two zero eigenvalues: whatever the procedure defines, but finite
    ref = check(ctxs, line, 0.02, ks=(8, 32))[32]
    assert np.isfinite(ref["normal"]).all() and (ref["n_normals"] > 100)
    far = np.concatenate([F(0.1) * rng.random((300, 3), dtype=F), np.full((1, 3), 5000, F)])
    ref = check(ctxs, far, 0.01, ks=(8,))[8]
    assert ref["n_used"][-1] == 0 and ref["curvature"][-1] == -1


def test_the_three_orientation_modes(ctxs):
    rng = np.random.default_rng(7)
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cloud = np.zeros((1500, 9), F)
    cloud[:, :3] = 0.4 * d + rng.normal(scale=0.002, size=d.shape)       # a noisy sphere about the origin
    cloud[:, 3:6] = -d                                                   # the records' own normals point inwards
    cloud[::50, 4] = np.nan                                              # a NaN there leaves the canonical sign
    cloud[7, 3:6] = 0
    canon = check(ctxs, cloud, 0.08, ks=(16,))[16]
    out = check(ctxs, cloud, 0.08, ks=(16,), orient="viewpoint", viewpoint=(3.0, 0.25, -0.5))[16]
    rec = check(ctxs, cloud, 0.08, ks=(16,), orient="record", modes=MODES[1:3])[16]
    has = canon["curvature"] >= 0
    assert has.sum() > 1400
    big = np.take_along_axis(canon["normal"], np.abs(canon["normal"]).argmax(axis=1)[:, None], axis=1)[:, 0]
    assert (big[has] > 0).all()
    assert (((out["normal"] * (np.array([3.0, 0.25, -0.5]) - cloud[:, :3])).sum(axis=1) >= -1e-6) | ~has).all()   # (d >= 0 in float64, before the normal is rounded)
    inward = (rec["normal"] * d).sum(axis=1) < 0
    plain = has & np.isfinite(cloud[:, 4])
    assert inward[plain].mean() > 0.99 and np.array_equal(bits(rec["normal"][::50]), bits(canon["normal"][::50]))
    assert np.array_equal(bits(np.abs(rec["normal"])), bits(np.abs(canon["normal"]))) and np.array_equal(bits(rec["cov"]), bits(canon["cov"]))


# ---- order and repeatability ----------------------------------------------------------------------------------------------------------------
def test_a_shuffled_cloud_gives_the_same_rows_permuted_and_two_runs_the_same_bits(ctxs):
    """tie-free (random float32 coordinates, no duplicates): ties are broken by index, which a shuffle changes"""
    rng = np.random.default_rng(8)
    cloud = rng.random((2500, 3), dtype=F)
    cloud[17] = np.nan
    m = ctxs["fast"]
    a = api.cloud_normals(cloud, 0.12, 32, want=WANT, matcher=m)
    b = api.cloud_normals(cloud, 0.12, 32, want=WANT, matcher=m)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in WANT) and a["pairs"] == b["pairs"] and a["n_normals"] == b["n_normals"]
    perm = rng.permutation(len(cloud))                                   # row r of the shuffled cloud is row perm[r] of the cloud
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    for dev in (False, True):
        c = cloud[perm]
        s = api.cloud_normals(torch.from_numpy(c).cuda() if dev else c, 0.12, 32, want=WANT, matcher=m)
        for k in ("n_used", "normal", "curvature", "cov"):
            assert np.array_equal(bits(s[k]), bits(a[k][perm])), k
        want = a["knn_index"][perm]
        assert np.array_equal(host(s["knn_index"]), np.where(want >= 0, inv[np.where(want >= 0, want, 0)], -1))
        assert (s["n_valid"], s["n_normals"], s["pairs"]) == (a["n_valid"], a["n_normals"], a["pairs"])


def test_want_names_the_outputs(ctxs):
    rng = np.random.default_rng(9)
    cloud = rng.random((500, 3), dtype=F)
    ref = cloud_normals_ref(cloud, 0.2, 16)
    r = api.cloud_normals(cloud, 0.2)
    assert sorted(r) == ["curvature", "n_normals", "n_valid", "normal", "pairs"] and np.array_equal(bits(r["normal"]), bits(ref["normal"]))
    r = api.cloud_normals(torch.from_numpy(cloud).cuda(), 0.2, want=("cov",), matcher=ctxs["strict"])
    assert r["cov"].is_cuda and np.array_equal(bits(r["cov"]), bits(ref["cov"]))
    r = api.cloud_normals(cloud, 0.2, want=())
    assert sorted(r) == ["n_normals", "n_valid", "pairs"] and (r["n_normals"], r["pairs"]) == (ref["n_normals"], ref["pairs"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_context_is_left_as_it_was(ctxs):
    m = ctxs["strict"]
    L = m.L
    state = lambda: [np.asarray(a).view(np.uint32).copy() for a in m.get_plane()] + [v.view(np.uint32).copy() for _, v in sorted(m.get_result().items())]
    before = state()
    rng = np.random.default_rng(10)
    c = rng.random((500, 3), dtype=F)
    cp = c.ctypes.data_as(C.c_void_p)
    used, nrm = np.full(500, -7, np.int32), np.full((500, 3), -7, F)
    n_valid, n_normals, pairs = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)

    def P(radius=0.1, k=8, min_neighbors=5, orient=0, viewpoint=(0, 0, 0), max_pairs=1 << 40):
        return api.CloudNormalsParams(radius, k, min_neighbors, orient, (C.c_float * 3)(*viewpoint), max_pairs)

    def call(cloud=cp, n=500, stride=3, prm=P(), mem=api.MEM_HOST):
        rc = L.tsar_cloud_normals_ctx(m._ctx, cloud, n, stride, C.byref(prm) if prm is not None else None, None, used.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p),
                                      None, None, C.byref(n_valid), C.byref(n_normals), C.byref(pairs), mem)
        return rc, L.tsar_last_error(m._ctx).decode()

    def refused(fragment, **kw):
        rc, msg = call(**kw)
        assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_normals:") and fragment in msg and "\n" not in msg, (rc, msg)
        assert (used == -7).all() and (nrm == -7).all() and n_valid.value == -1 and n_normals.value == -1       # a refused call writes nothing

    refused("params is NULL", prm=None)
    refused("mem must be", mem=7)
    refused("stride", stride=2)
    refused("n must be", n=-1)
    refused("n must be", n=1 << 31)
    for R in (0.0, -1.0, np.inf, np.nan, 1e30, 1e-30):
        refused("radius must be finite and > 0", prm=P(radius=R))
    for k in (2, 0, -1, 33):
        refused("k must be in 3..", prm=P(k=k, min_neighbors=2))
    for mn in (1, 0, 9):
        refused("min_neighbors must be in 2..k", prm=P(min_neighbors=mn))
    for o in (-1, 3):
        refused("orient must be", prm=P(orient=o))
    refused("the stride must be at least 6", prm=P(orient=2), stride=5)
    for vp in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        refused("finite viewpoint", prm=P(orient=1, viewpoint=vp))
    refused("max_pairs must be >= 0", prm=P(max_pairs=-1))
    assert pairs.value == -1
    far = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [0, 2e4, 0]], F)
    refused("2^20 cells or more", cloud=far.ctypes.data_as(C.c_void_p), n=3, prm=P(radius=0.01))
    want_pairs = cloud_normals_ref(c, 0.1, 8)["pairs"]
    refused("more than max_pairs", prm=P(max_pairs=want_pairs - 1))
    assert pairs.value == want_pairs                                     # *pairs_out is filled, nothing else is written
    with pytest.raises(api.TsarError) as e:
        api.cloud_normals(torch.from_numpy(c).cuda(), 0.1, 8, max_pairs=want_pairs - 1, matcher=m)
    assert e.value.code == api.TSAR_ERR_INVALID and e.value.pairs == want_pairs
    rc, _ = call(prm=P(max_pairs=want_pairs))                            # exactly max_pairs pass; a NaN viewpoint is not read with orient 0
    assert rc == api.TSAR_OK and n_valid.value == 500 and pairs.value == want_pairs and (used >= 0).all() and n_normals.value > 0
    rc, _ = call(prm=P(viewpoint=(np.nan, 0, 0)))
    assert rc == api.TSAR_OK
    assert all(np.array_equal(a, b) for a, b in zip(before, state()))
    check(ctxs, c, 0.1, ks=(8,))                                         # and the contexts still work
    m.pm_iterate(1)


# ---- normal_compare -------------------------------------------------------------------------------------------------------------------------
def compare_case():
    rng = np.random.default_rng(11)
    n, nb = 900, 400
    a = np.full((n, 6), np.nan, F)
    a[:, :3] = rng.normal(size=(n, 3))
    b = rng.normal(size=(nb, 3)).astype(F)
    idx = rng.integers(0, nb, n).astype(np.int32)
    d2 = (rng.random(n, dtype=F) * F(0.02)).astype(F)
    idx[:40] = -1                                                        # every exclusion in turn
    idx[40:60] = nb
    idx[60:70] = -5
    d2[70:100] = F(0.5)
    d2[100:110] = np.nan
    d2[110] = F(F(0.1) * F(0.1))                                         # exactly fl(max_dist * max_dist): compared
    d2[111] = np.nextafter(F(F(0.1) * F(0.1)), F(1))
    a[120:130, 0] = np.nan
    a[130:140, 2] = np.inf
    a[140:150, :3] = 0
    b[:5] = 0
    b[5, 1] = np.nan
    b[6, 0] = -np.inf
    idx[150:157] = np.arange(7)
    a[200, :3], b[10], idx[200] = (1, 0, 0), (1, 1, 0), 10               # 45 degrees
    a[201, :3], b[11], idx[201] = (0, 0, 2), (0, 0, -3), 11              # opposite: |c| = 1, c = -1
    a[202, :3], b[12], idx[202] = (0, 3, 0), (0, 0.5, 0), 12             # parallel: c = 1 exactly
    a[203, :3], b[13], idx[203] = (0, 3, 0), (2, 0, 0), 13               # orthogonal: c = 0 exactly
    d2[200:204] = 0
    return a, b, idx, d2


def test_normal_compare_exclusions_and_a_threshold_met_exactly(ctxs):
    a, b, idx, d2 = compare_case()
    deg = [0.0, 10.0, 45.0, 60.0, 90.0, 180.0]                           # cos(0) = 1 is met exactly by row 202; cos(180) = -1 by row 201 when signed
    mc = api.min_cos_of(deg)
    for signed in (False, True):
        for with_d2 in (True, False):
            ref = normal_compare_ref(a, b, idx, mc, d2 if with_d2 else None, 0.1 if with_d2 else None, signed)
            assert 300 < ref["n_compared"] < 880 and ref["within"][0] >= 1 and ref["within"][-1] == ref["n_compared"]
            for dev, name in ((False, "strict"), (True, "fast"), (True, "none")):
                conv = (lambda x: torch.from_numpy(x).cuda()) if dev else (lambda x: x)
                r = api.normal_compare(conv(a), conv(b), conv(idx), deg, dist2=conv(d2) if with_d2 else None, max_dist=0.1 if with_d2 else None, signed=signed,
                                       want_cos=True, matcher=ctxs[name])
                assert r["n_compared"] == ref["n_compared"] and r["within"].tolist() == ref["within"].tolist(), (signed, with_d2, dev)
                assert torch.is_tensor(r["cos"]) == dev and np.array_equal(bits(r["cos"]), bits(ref["cos"]))
                assert r["accuracy"].tolist() == (ref["within"] / np.float64(ref["n_compared"])).tolist()
            c = ref["cos"]
            assert np.isnan(c[:70]).all() and np.isnan(c[120:157]).all() and np.isnan(c[70:110]).all() == with_d2
            assert (not np.isnan(c[110])) and np.isnan(c[111]) == with_d2
            assert c[201] == (-1 if signed else 1) and c[202] == 1 and c[203] == 0
    r = api.normal_compare(a, b[:0], idx, deg, matcher=ctxs["fast"])     # no row of b: nothing is compared
    assert r["n_compared"] == 0 and r["within"].tolist() == [0] * 6 and r["accuracy"].tolist() == [0.0] * 6
    r = api.normal_compare(a[:0], b, idx[:0], deg)
    assert r["n_compared"] == 0
    m = ctxs["fast"]
    for kw, fragment in ((dict(tolerances_deg=list(range(17))), "n_tol must be in 0..16"), (dict(dist2=d2, max_dist=np.inf), "max_dist must be finite"),
                         (dict(dist2=d2, max_dist=0.0), "max_dist must be finite")):
        with pytest.raises(api.TsarError) as e:
            api.normal_compare(a, b, idx, **dict(dict(tolerances_deg=deg), **kw), matcher=m)
        assert e.value.code == api.TSAR_ERR_INVALID and "tsar_cloud_normal_compare:" in str(e.value) and fragment in str(e.value)
    bad = np.array([1.5], np.float64)
    rc = m.L.tsar_cloud_normal_compare_ctx(m._ctx, a.ctypes.data_as(C.c_void_p), 6, len(a), b.ctypes.data_as(C.c_void_p), 3, len(b), idx.ctypes.data_as(C.c_void_p), None, 0.0,
                                           1, bad.ctypes.data_as(C.c_void_p), 0, None, None, None, api.MEM_HOST)
    assert rc == api.TSAR_ERR_INVALID and "every threshold must be in [-1, 1]" in m.L.tsar_last_error(m._ctx).decode()
    rc = m.L.tsar_cloud_normal_compare_ctx(m._ctx, a.ctypes.data_as(C.c_void_p), 2, len(a), b.ctypes.data_as(C.c_void_p), 3, len(b), idx.ctypes.data_as(C.c_void_p), None, 0.0,
                                           0, None, 0, None, None, None, api.MEM_HOST)
    assert rc == api.TSAR_ERR_INVALID and "a stride must be at least 3" in m.L.tsar_last_error(m._ctx).decode()
    m.pm_iterate(1)


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_cloud_normals_equals_the_restatement(ctxs):
    """the stray scene's surface: every second point, with the analytic normal, is the reconstruction; the rest, without normals, the scan"""
    pts, nrm = stray_surface()
    recon = np.zeros((1500, 6), F)
    recon[:, :3] = pts[::2]
    recon[:, 3:6] = nrm
    recon[::100, 3:6] = 0                                                 # records without a normal are not compared
    gt, tol = pts[1::2], [0.01, 0.03]
    plain = api.evaluate_cloud(recon, gt, tol, matcher=ctxs["fast"])
    for normals, more in ((dict(radius=0.06, k=16), {}), (dict(radius=0.08, k=8, min_neighbors=4, tolerances_deg=(2.0, 5.0, 20.0), signed=True), {"crop": (0.1, 0.0, 0.0, 0.9, 1.0, 1.0)})):
        ref = evaluate_normals_ref(recon, gt, tol, normals, **more)
        assert 1000 < ref["n_normal_compared"] < 1500 and 0 < ref["n_normal_within"][0] < ref["n_normal_within"][-1]
        base = api.evaluate_cloud(recon, gt, tol, matcher=ctxs["fast"], **more)
        for dev in (False, True):
            r = api.evaluate_cloud(*((torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (recon, gt)) if dev else (recon, gt)), tol, normals=normals,
                                   matcher=ctxs["fast"] if dev else None, **more)
            for k in ("n_gt_normals", "n_normal_compared"):
                assert r[k] == ref[k], k
            for k in ("normal_tolerances_deg", "n_normal_within", "normal_accuracy"):
                assert r[k].tolist() == ref[k].tolist(), k
            assert r["normals"] == {"k": normals["k"], "radius": normals["radius"], "min_neighbors": normals.get("min_neighbors", 5), "signed": normals.get("signed", False)}
            assert sorted(set(r) - set(base)) == ["n_gt_normals", "n_normal_compared", "n_normal_within", "normal_accuracy", "normal_tolerances_deg", "normals"]
            for k in base:                                               # and what the call gave before is what it gives now
                assert np.array_equal(r[k], base[k]), k
    assert "normals" not in plain
    with pytest.raises(ValueError):
        api.evaluate_cloud(recon[:, :3], gt, tol, normals=dict(radius=0.06))


def test_the_evaluate_tool_scores_normals_like_the_restatement(tmp_path):
    pts, nrm = stray_surface()
    recon = np.zeros((1500, 6), F)
    recon[:, :3] = pts[::2]
    recon[:, 3:6] = nrm
    recon[::100, 3:6] = 0
    gt = pts[1::2]
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon[:, :3], normals=recon[:, 3:6])
    tio.write_ply(b, gt)
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate")
    plain = subprocess.run([tool, a, b, "--tolerances=0.01,0.03"], capture_output=True, text=True, timeout=120)
    out = subprocess.run([tool, a, b, "--tolerances=0.01,0.03", "--normals=8", "--normal_radius=0.08", "--normal_min_neighbors=4", "--normal_tolerances=2,5,20"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and plain.returncode == 0, out.stderr + plain.stderr
    rec, before = json.loads(out.stdout.splitlines()[-1]), json.loads(plain.stdout.splitlines()[-1])
    ref = evaluate_normals_ref(recon, gt, [0.01, 0.03], dict(radius=0.08, k=8, min_neighbors=4, tolerances_deg=(2.0, 5.0, 20.0)))
    for k in ("n_gt_normals", "n_normal_compared"):
        assert rec[k] == ref[k], k
    for k in ("normal_tolerances_deg", "n_normal_within", "normal_accuracy"):
        assert rec[k] == ref[k].tolist(), k
    assert F(rec["normals"].pop("radius")) == F(0.08) and rec["normals"] == {"k": 8, "min_neighbors": 4, "signed": False}
    assert ref["n_normal_compared"] > 1000 and 0 < ref["n_normal_within"][0] < ref["n_normal_within"][-1]
    assert "normals" not in before and all(rec[k] == before[k] for k in before if not k.startswith("ms_"))        # without the switch: what it was
    r = api.evaluate_cloud(recon, gt, [0.01, 0.03], normals=dict(radius=0.08, k=8, min_neighbors=4, tolerances_deg=(2.0, 5.0, 20.0)))
    assert r["n_normal_within"].tolist() == rec["n_normal_within"] and r["normal_accuracy"].tolist() == rec["normal_accuracy"]

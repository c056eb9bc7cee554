"""The numpy restatement of tsar_cloud_normals / tsar_cloud_normal_compare (tests/cloud_normals_ref.py) held to known answers; no GPU.

Figures of the restatement itself on the scenes below (3000 points each; the plane has 2936 distinct lattice points, 2931 with a normal):
  smallest gap ratio (lambda1 - lambda0) / lambda2:  stray surface k = 16: 0.078, k = 8: 0.028;  sphere: 0.16;  plane: 0.081 -- none below 1e-3
  largest angle of the float64 normal to np.linalg.eigh's, 6 sweeps:  5.5e-16 / 1.2e-15 / 7.3e-16 / 8.6e-16 rad (the same after 4 sweeps);
  3 sweeps leave 2.5e-6 rad on the sphere and 3.2e-9 rad on the plane
  exact plane: largest angle to (-1/2, -1/4, 1) normalised 3.6e-16 rad; largest curvature 1.2e-16
  stray surface, R = 0.06, k = 16: the normals lie a median 1.75 degrees and a 95th percentile 4.21 degrees from the true normal
The bar against LAPACK, 1e-9 rad under the gap condition (lambda1 - lambda0) >= 1e-3 lambda2, is Davis-Kahan's: about 100 eps / 1e-3 = 2e-11,
with 50 x over that."""
import numpy as np
import pytest

from cloud_normals_ref import (canonical_sign, cloud_normals_ref, jacobi_ref, knn_ref, normal_compare_ref, smallest_eigenpair, stray_surface)

F, D = np.float32, np.float64


def sphere():
    rng = np.random.default_rng(1)
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (0.4 * d + rng.normal(scale=0.002, size=d.shape)).astype(F)


def dyadic_plane():
    """z = x / 2 + y / 4 on a 1 / 256 lattice: every coordinate, difference, product and sum below is exact in float64"""
    rng = np.random.default_rng(2)
    xy = np.unique(rng.integers(0, 256, (3000, 2)) / 256.0, axis=0)
    return np.column_stack([xy, xy[:, 0] / 2 + xy[:, 1] / 4]).astype(F)


SCENES = {"stray-k16": (lambda: stray_surface()[0], 0.06, 16), "stray-k8": (lambda: stray_surface()[0], 0.06, 8), "sphere": (sphere, 0.08, 16),
          "plane": (dyadic_plane, 0.05, 16)}


@pytest.fixture(scope="module")
def results():
    return {name: (make(), cloud_normals_ref(make(), R, k, want_v64=True)) for name, (make, R, k) in SCENES.items()}


def full(C6):
    C = np.zeros((len(C6), 3, 3), D)
    for (i, j), col in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        C[:, i, j] = C[:, j, i] = C6[:, col]
    return C


def angle(u, v):
    """the angle between the lines of u and v, in radians (asin of the cross product: exact near 0, where acos of the dot is not)"""
    return np.arcsin(np.clip(np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1)), 0, 1))


@pytest.mark.parametrize("name", list(SCENES))
def test_the_jacobi_normal_is_lapacks(results, name):
    _, r = results[name]
    has = r["n_used"] >= 5
    assert has.sum() > 2900
    w, U = np.linalg.eigh(full(r["cov"][has]))
    assert ((w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]).all()                 # no point of the scene falls outside the condition
    ang = angle(r["v64"][has], U[:, :, 0])
    print(name, "smallest gap ratio %.3g, largest angle to LAPACK %.3g rad" % (((w[:, 1] - w[:, 0]) / w[:, 2]).min(), ang.max()))
    assert ang.max() <= 1e-9
    assert np.abs(np.linalg.norm(r["v64"][has], axis=1) - 1).max() <= 1e-15
    assert np.abs(np.sort(r["eig"][has], axis=1) - w).max() <= 1e-15 * w.max()
    assert np.array_equal(r["normal"][has], r["v64"][has].astype(F))     # rounded once, not renormalised


def test_three_sweeps_would_not_be_enough_and_four_are():
    p = sphere()
    six = cloud_normals_ref(p, 0.08, 16, want_v64=True)
    w, U = np.linalg.eigh(full(six["cov"]))
    a3 = angle(cloud_normals_ref(p, 0.08, 16, sweeps=3, want_v64=True)["v64"], U[:, :, 0]).max()
    a4 = angle(cloud_normals_ref(p, 0.08, 16, sweeps=4, want_v64=True)["v64"], U[:, :, 0]).max()
    print("sphere: 3 sweeps leave %.3g rad, 4 sweeps %.3g rad" % (a3, a4))
    assert a3 > 1e-9 and a4 <= 1e-14


def test_the_exact_plane(results):
    _, r = results["plane"]
    has = r["n_used"] >= 5
    t = np.array([-0.5, -0.25, 1.0])
    ang = angle(r["normal"][has].astype(D), np.broadcast_to(t, (has.sum(), 3)))
    print("plane: largest angle %.3g rad, largest curvature %.3g" % (ang.max(), r["curvature"][has].max()))
    assert ang.max() <= 2.0 ** -22 and (r["curvature"][has] >= 0).all() and r["curvature"][has].max() <= 1e-12
    assert (r["normal"][has, 2] > 0).all()                               # the canonical sign: z is the largest component


def test_quality_on_the_stray_surface(results):
    _, r = results["stray-k16"]
    _, true = stray_surface()
    deg = np.degrees(angle(r["v64"], np.broadcast_to(true, (3000, 3))))
    print("stray surface: median %.3f degrees, 95th percentile %.3f degrees" % (np.median(deg), np.percentile(deg, 95)))
    assert r["n_normals"] == 3000 and np.median(deg) <= 1.8 and np.percentile(deg, 95) <= 4.3      # the prototype's 1.75 and 4.2
    assert 0 < np.median(r["curvature"]) < 0.01


def test_the_tie_rule_on_an_integer_lattice():
    p = np.array([[x, y, z] for z in range(5) for y in range(5) for x in range(5)], F)
    knn, used = knn_ref(p, 1.0, 4)
    mid = 2 + 5 * 2 + 25 * 2
    assert used[mid] == 4 and knn[mid].tolist() == [mid - 25, mid - 5, mid - 1, mid + 1]       # six at d2 = 1: the four smallest indices
    assert used[0] == 3 and knn[0].tolist() == [1, 5, 25, -1]
    knn, used = knn_ref(p, np.sqrt(2.0) * 1.0001, 32)
    assert used[mid] == 18 and knn[mid, :6].tolist() == [mid - 25, mid - 5, mid - 1, mid + 1, mid + 5, mid + 25] and (np.diff(knn[mid, 6:18]) > 0).all()
    dup = np.concatenate([p, p[mid:mid + 1]])                            # a duplicate counts, at d2 = 0, before everything else
    knn, used = knn_ref(dup, 1.0, 4)
    assert knn[mid, 0] == 125 and knn[125, 0] == mid and knn[125, 1:].tolist() == [mid - 25, mid - 5, mid - 1]
    r = cloud_normals_ref(p, 1.0, 8, min_neighbors=6)
    assert r["n_normals"] == 27 and np.isfinite(r["normal"]).all()      # the inner 3 x 3 x 3 have six neighbours; C is a multiple of I there
    assert (r["normal"][mid] == np.array([1, 0, 0], F)).all() and r["curvature"][mid] == F(1 / 3)   # nothing rotates: the lowest index


def test_a_line_has_two_zero_eigenvalues():
    rng = np.random.default_rng(3)
    line = np.zeros((300, 3), F)
    line[:, 1] = rng.random(300, dtype=F)
    r = cloud_normals_ref(line, 0.02, 16, want_v64=True)
    has = r["n_used"] >= 5
    assert has.sum() > 100 and np.isfinite(r["v64"]).all() and np.abs(np.linalg.norm(r["v64"][has], axis=1) - 1).max() <= 1e-15
    assert (r["curvature"][has] == 0).all() and (np.abs(r["v64"][has, 1]) <= 1e-15).all()
    skew = (np.array([[1, 2, 3]], D) * rng.random((300, 1))).astype(F)   # a line off the axes: still finite and of unit length
    r = cloud_normals_ref(skew, 0.1, 16, want_v64=True)
    has = r["n_used"] >= 5
    assert has.sum() > 100 and np.isfinite(r["v64"]).all() and np.abs(np.linalg.norm(r["v64"][has], axis=1) - 1).max() <= 1e-15
    assert np.abs(r["v64"][has] @ np.array([1, 2, 3]) / np.sqrt(14)).max() <= 1e-6 and (r["curvature"][has] <= 1e-12).all()


def test_the_three_orientation_modes():
    p = sphere()
    d = p.astype(D) / np.linalg.norm(p.astype(D), axis=1, keepdims=True)
    rec = np.zeros((3000, 6), F)
    rec[:, :3], rec[:, 3:6] = p, -d
    rec[::50, 4] = np.nan
    canon = cloud_normals_ref(rec, 0.08, 16, want_v64=True)
    v = canon["v64"]
    big = np.take_along_axis(v, np.abs(v).argmax(axis=1)[:, None], axis=1)[:, 0]
    assert canon["n_normals"] == 3000 and (big > 0).all() and np.array_equal(canonical_sign(-v), v)
    vp = (3.0, 0.25, -0.5)
    out = cloud_normals_ref(rec, 0.08, 16, orient=1, viewpoint=vp, want_v64=True)["v64"]
    assert ((out * (np.array(vp) - p.astype(D))).sum(axis=1) >= 0).all() and np.array_equal(np.abs(out), np.abs(v)) and (out != v).any()
    centre = cloud_normals_ref(rec, 0.08, 16, orient=1, viewpoint=(0, 0, 0), want_v64=True)["v64"]
    assert ((centre * d).sum(axis=1) < 0).all()                          # seen from the centre every normal points inwards
    own = cloud_normals_ref(rec, 0.08, 16, orient=2, want_v64=True)["v64"]
    plain = np.isfinite(rec[:, 4])
    assert np.array_equal(own[plain], centre[plain]) and np.array_equal(own[~plain], v[~plain])      # a NaN leaves the canonical sign


def test_every_no_normal_case():
    rng = np.random.default_rng(4)
    p = rng.random((400, 3), dtype=F)
    p[5, 0], p[6, 1], p[7, 2] = np.nan, np.inf, -np.inf
    p[8] = 50                                                            # alone
    r = cloud_normals_ref(p, 0.15, 8, min_neighbors=5)
    few = (r["n_used"] >= 0) & (r["n_used"] < 5)
    assert (r["n_used"][5:8] == -1).all() and (r["knn_index"][5:8] == -1).all() and r["n_used"][8] == 0 and few.sum() > 20
    none = few | (r["n_used"] < 0)
    assert (r["normal"][none] == 0).all() and not np.signbit(r["normal"][none]).any() and (r["curvature"][none] == -1).all() and (r["cov"][none] == 0).all()
    assert (r["knn_index"][few, 0] >= 0).sum() == (r["n_used"][few] > 0).sum()                  # the list is still returned
    assert r["n_valid"] == 397 and r["n_normals"] == 400 - none.sum() and (r["curvature"][~none] >= 0).all()
    assert not np.isin(r["knn_index"], [5, 6, 7]).any()
    empty = cloud_normals_ref(np.zeros((0, 3), F), 0.1, 8)
    assert empty["n_valid"] == empty["n_normals"] == empty["pairs"] == 0 and empty["normal"].shape == (0, 3) and empty["cov"].dtype == D


def test_normal_compare_every_exclusion():
    a = np.array([[1, 0, 0], [0, 0, 2], [0, 3, 0], [0, 3, 0], [1, 1, 0], [np.nan, 0, 1], [0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], F)
    b = np.array([[1, 1, 0], [0, 0, -3], [0, 0.5, 0], [2, 0, 0], [0, 0, 0], [np.inf, 0, 0]], F)
    idx = np.array([0, 1, 2, 3, 0, 0, 0, 4, 5, -1, 6, 0], np.int32)
    d2 = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], F)
    mc = np.cos(np.deg2rad(np.array([0.0, 45.0, 46.0, 90.0, 180.0])))
    r = normal_compare_ref(a, b, idx, mc, d2, 0.5)
    assert r["n_compared"] == 5 and np.isnan(r["cos"][5:]).all()         # a NaN; a zero a; a zero b; an inf b; -1; past n_b; too far
    assert r["cos"][:5].tolist() == [F(1.0 / np.sqrt(2.0)), 1.0, 1.0, 0.0, 1.0]
    assert r["within"].tolist() == [3, 3 + int(1.0 / np.sqrt(2.0) >= mc[1]), 4, 4, 5]                     # 1 >= cos(0) is met exactly; 0 < cos(90 degrees) = 6e-17
    s = normal_compare_ref(a, b, idx, mc, d2, 0.5, signed=True)
    assert s["cos"][1] == -1 and s["within"].tolist() == [2, 2 + int(1.0 / np.sqrt(2.0) >= mc[1]), 3, 3, 5]
    assert normal_compare_ref(a, b, idx, mc)["n_compared"] == 6          # without dist2 the last row counts
    assert normal_compare_ref(a, b, idx, mc, np.full(12, np.nan, F), 0.5)["n_compared"] == 0
    assert normal_compare_ref(a, b, idx, mc, np.full(12, F(F(0.5) * F(0.5))), 0.5)["n_compared"] == 6      # dist2 == fl(max_dist * max_dist) passes

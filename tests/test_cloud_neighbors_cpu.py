"""The numpy restatement of tsar_cloud_neighbors and of the remove_outliers rules (tests/cloud_neighbors_ref.py) against answers worked by
hand.  The GPU tests hold the kernels to this restatement bit for bit; this file holds the restatement to the definition in include/tsar.h."""
import numpy as np
import pytest

from cloud_neighbors_ref import clean_ref, cloud_neighbors_ref, keep_mask_ref, lower_median, remove_outliers_ref

F = np.float32
INF = F(np.inf)


def radius_for(d2):
    """the smallest float32 R whose float32 square reaches d2 (fl(sqrt(2))^2 rounds to just below 2: one ulp up is needed there)"""
    r = F(np.sqrt(F(d2)))
    while F(r * r) < F(d2):
        r = np.nextafter(r, INF)
    assert F(np.nextafter(r, F(0)) * np.nextafter(r, F(0))) < F(d2) <= F(r * r)
    return r


def lattice(m=3):
    return np.array([[x, y, z] for z in range(m) for y in range(m) for x in range(m)], F)


@pytest.mark.parametrize("d2,centre,corner,edge_mid,face_mid", [(1, 6, 3, 4, 5), (2, 18, 6, 9, 13), (3, 26, 7, 11, 17)])
def test_integer_lattice_counts(d2, centre, corner, edge_mid, face_mid):
    """3 x 3 x 3 points on integer coordinates: 6 neighbours at d2 = 1, 12 at 2 and 8 at 3 around the centre; fewer at the border"""
    p = lattice()
    r = cloud_neighbors_ref(p, radius_for(d2))
    at = lambda x, y, z: r["count"][x + 3 * y + 9 * z]
    assert (at(1, 1, 1), at(0, 0, 0), at(1, 0, 0), at(1, 1, 0)) == (centre, corner, edge_mid, face_mid)
    assert r["n_valid"] == 27 and r["pairs"] == 27 * 27 and r["knn_dist2"].shape == (27, 0)          # radius >= 1: every cell touches every other
    if d2 == 2:                                                                                       # the rounded root itself misses the diagonal
        assert cloud_neighbors_ref(p, F(np.sqrt(F(2))))["count"][13] == 6


def test_integer_lattice_ties_in_knn_dist2():
    r = cloud_neighbors_ref(lattice(), radius_for(3), k=8)["knn_dist2"]
    assert r[13].tolist() == [1, 1, 1, 1, 1, 1, 2, 2]                    # the centre: six at 1, then two of the twelve at 2
    assert r[0].tolist() == [1, 1, 1, 2, 2, 2, 3, np.inf]                # a corner: 3 + 3 + 1 within sqrt(3), then the padding
    r = cloud_neighbors_ref(lattice(), radius_for(1), k=8)["knn_dist2"]
    assert r[13].tolist() == [1] * 6 + [np.inf] * 2 and r[0].tolist() == [1] * 3 + [np.inf] * 5


def test_a_pair_at_exactly_the_radius_counts_and_one_ulp_beyond_does_not():
    R = F(0.75)                                                          # R * R = 0.5625 exactly
    beyond = np.nextafter(R, INF)
    assert F(beyond * beyond) > F(R * R)
    p = np.array([[0, 0, 0], [R, 0, 0], [5, 0, 0], [5, beyond, 0]], F)      # (the second pair differs on an axis where one coordinate is 0: exact)
    r = cloud_neighbors_ref(p, R, k=1)
    assert r["count"].tolist() == [1, 1, 0, 0]
    assert r["knn_dist2"][:, 0].tolist() == [0.5625, 0.5625, np.inf, np.inf]


def test_duplicates_count_at_distance_zero_and_the_point_itself_does_not():
    p = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [11, 2, 3]], F)
    r = cloud_neighbors_ref(p, 1.0, k=3)
    assert r["count"].tolist() == [2, 2, 2, 0]
    assert r["knn_dist2"][:3].tolist() == [[0, 0, np.inf]] * 3 and r["knn_dist2"][3].tolist() == [np.inf] * 3
    assert np.signbit(r["knn_dist2"][:3, :2]).sum() == 0                 # +0
    assert r["pairs"] == 3 * 3 + 1                                       # per candidate the candidates of its 27 cells, itself included


def test_non_finite_records_take_no_part():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0.5, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0.5, 0]], F)
    r = cloud_neighbors_ref(p, 1.0, k=2)
    assert r["count"].tolist() == [2, -1, 2, -1, -1, 2] and r["n_valid"] == 3
    assert np.isposinf(r["knn_dist2"][[1, 3, 4]]).all()
    assert r["knn_dist2"][0].tolist() == [0.25, 0.25] and r["knn_dist2"][2].tolist() == [0.25, 0.5]
    r = cloud_neighbors_ref(p[[1, 3]], 1.0, k=1)                         # no candidate at all
    assert r["count"].tolist() == [-1, -1] and r["n_valid"] == 0 and r["pairs"] == 0
    r = cloud_neighbors_ref(np.zeros((0, 3), F), 1.0, k=4)
    assert r["count"].shape == (0,) and r["knn_dist2"].shape == (0, 4) and r["n_valid"] == 0 and r["pairs"] == 0


def test_fewer_than_k_neighbours_are_padded_with_inf():
    p = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F)
    r = cloud_neighbors_ref(p, 2.0, k=4)
    assert r["knn_dist2"].tolist() == [[1, np.inf, np.inf, np.inf], [1, 4, np.inf, np.inf], [4, np.inf, np.inf, np.inf]]
    assert r["count"].tolist() == [1, 2, 1]


def test_lower_median():
    assert lower_median(np.array([5, 1, 4, 2], F)) == 2                  # m even: element 1 of (1, 2, 4, 5)
    assert lower_median(np.array([5, 1, 4, 2, 9], F)) == 4               # m odd: element 2 of (1, 2, 4, 5, 9)
    assert lower_median(np.array([7], F)) == 7 and lower_median(np.zeros(0, F)) is None


def test_remove_outliers_rules():
    p = np.array([[0, 0, 0, 7], [1, 0, 0, 8], [2, 0, 0, 9], [3, 0, 0, 10], [10, 0, 0, 11], [np.nan, 0, 0, 12]], F)
    rows, keep = remove_outliers_ref(p, 1.5, min_neighbors=1)
    assert keep.tolist() == [True, True, True, True, False, False] and np.array_equal(rows, p[:4])      # whole records, the cloud's order
    assert keep_mask_ref(p, 1.5, min_neighbors=2).tolist() == [False, True, True, False, False, False]
    # k = 1 within R = 20: s = (1, 1, 1, 1, 49), m = 5, med = 1;  T = fl(fl(Q * Q) * 1)
    assert keep_mask_ref(p, 20.0, k=1, ratio=2.0).tolist() == [True] * 4 + [False, False]               # 49 > 4
    assert keep_mask_ref(p, 20.0, k=1, ratio=7.0).tolist() == [True] * 5 + [False]                      # 49 <= 49
    assert keep_mask_ref(p, 20.0, k=1, ratio=np.nextafter(F(7), F(0))).tolist() == [True] * 4 + [False, False]
    # k = 2 within R = 1.5: s = (inf, 1, 1, inf, inf): m = 2, the lower median is 1
    assert keep_mask_ref(p, 1.5, k=2, ratio=1.0).tolist() == [False, True, True, False, False, False]
    # both rules: each must pass
    assert keep_mask_ref(p, 20.0, min_neighbors=5, k=1).tolist() == [False] * 6 and keep_mask_ref(p, 20.0, min_neighbors=4, k=1).tolist() == [True] * 4 + [False] * 2
    # m = 0: no finite k-th distance, nothing passes
    assert not keep_mask_ref(p, 0.5, k=1).any()
    c, removed = clean_ref(p, radius=1.5, min_neighbors=1)
    assert removed == 1 and np.isnan(c[4:, :3]).all() and np.array_equal(c[:4], p[:4]) and c[4, 3] == 11


def test_the_two_products_of_the_threshold_are_float32():
    """a ratio whose square rounds in float32: T = fl(fl(Q * Q) * med), not the float64 product"""
    q = F(1.6)                                                           # fl(Q * Q) lies above the exact square
    q2 = F(q * q)
    assert np.float64(q2) != np.float64(q) * np.float64(q)
    # s = (1, 1, x, x, 1, 1) with x = fl(Q * Q): med = 1, T = x, so the pair at x stays; the float64 product Q * Q lies below x and would drop it
    d = F(np.sqrt(np.float64(q2)))
    assert F(d * d) == q2 and np.float64(q) * np.float64(q) < np.float64(q2)
    p = np.array([[0, 0, 0], [1, 0, 0], [100, 0, 0], [100, d, 0], [200, 0, 0], [200, 1, 0]], F)
    s = cloud_neighbors_ref(p, 2.0, k=1)["knn_dist2"][:, 0]
    assert s.tolist() == [1, 1, q2, q2, 1, 1] and lower_median(s) == 1
    assert keep_mask_ref(p, 2.0, k=1, ratio=q).all() and not keep_mask_ref(p, 2.0, k=1, ratio=np.nextafter(q, F(0)))[2:4].any()

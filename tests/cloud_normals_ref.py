"""numpy restatement of tsar_cloud_normals and tsar_cloud_normal_compare (include/tsar.h): the brute-force definition.  Neighbours from an
n x n float32 d2 (as cloud_neighbors_ref.py) ordered with np.lexsort on (index, d2); moments and Jacobi in float64, one numpy operation
per operation of the header, vectorised over the points with np.where for the skipped rotation.  Shared by test_cloud_normals_cpu.py,
test_api_normals_marshal_cpu.py and test_gpu_cloud_normals.py; nothing here reads the library."""
import numpy as np

from cloud_distance_ref import candidates, cloud_distance_ref, pairs_per_query

KNN_MAX = 32
F, D = np.float32, np.float64
ROTATIONS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))


def knn_ref(cloud, radius, k, chunk_elems=1 << 22):
    """-> (knn_index [n, k] int32, -1 padded; n_used [n] int32, -1 for a non-candidate): per candidate the other candidates with
    d2 <= fl(R * R), the smallest d2 first, then the smallest index, cut at k"""
    p = np.asarray(cloud, F)[:, :3]
    n = len(p)
    r = F(radius)
    r2 = F(r * r)
    ci = np.flatnonzero(candidates(p))
    pc = p[ci]
    knn = np.full((n, k), -1, np.int32)
    used = np.full(n, -1, np.int32)
    rows = max(1, chunk_elems // max(1, len(ci)))
    with np.errstate(over="ignore"):
        for s in range(0, len(ci), rows):
            qq = pc[s:s + rows]
            dx = qq[:, None, 0] - pc[None, :, 0]
            dy = qq[:, None, 1] - pc[None, :, 1]
            dz = qq[:, None, 2] - pc[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            d2 = np.where(d2 <= r2, d2, F(np.inf))
            d2[np.arange(len(qq)), s + np.arange(len(qq))] = np.inf               # j != i, by index
            for a in range(len(qq)):
                order = np.lexsort((ci, d2[a]))                                   # by d2, then by the index in the cloud
                order = order[np.isfinite(d2[a][order])][:k]
                knn[ci[s + a], :len(order)] = ci[order]
                used[ci[s + a]] = len(order)
    return knn, used


def jacobi_ref(C6, sweeps=6):
    """C6 [n, 6] float64 (xx xy xz yy yz zz) -> (a [n, 3, 3] after the sweeps, V [n, 3, 3]): the header's cyclic Jacobi, every rotation one
    numpy operation per operation, a rotation with a_pq == 0 skipped through np.where"""
    n = len(C6)
    a = np.zeros((n, 3, 3), D)
    for (i, j), col in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        a[:, i, j] = a[:, j, i] = C6[:, col]
    V = np.zeros((n, 3, 3), D)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in ROTATIONS:
                apq = a[:, p, q].copy()
                skip = apq == 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                a[:, p, p] = np.where(skip, a[:, p, p], a[:, p, p] - h)
                a[:, q, q] = np.where(skip, a[:, q, q], a[:, q, q] + h)
                a[:, p, q] = a[:, q, p] = np.where(skip, apq, 0.0)
                x, y = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, r, p] = a[:, p, r] = np.where(skip, x, c * x - s * y)
                a[:, r, q] = a[:, q, r] = np.where(skip, y, s * x + c * y)
                for k in range(3):
                    x, y = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(skip, x, c * x - s * y)
                    V[:, k, q] = np.where(skip, y, s * x + c * y)
    return a, V


def smallest_eigenpair(a, V):
    """-> (lambda0 [n], v [n, 3] float64): the smallest diagonal entry, the lowest index on ties, and that column of V"""
    l0, v = a[:, 0, 0].copy(), V[:, :, 0].copy()
    for i in (1, 2):
        less = a[:, i, i] < l0
        l0 = np.where(less, a[:, i, i], l0)
        v = np.where(less[:, None], V[:, :, i], v)
    return l0, v


def canonical_sign(v):
    """v negated where its component of largest magnitude (the lowest index on ties) is < 0"""
    big = v[:, 0].copy()
    for i in (1, 2):
        big = np.where(np.abs(v[:, i]) > np.abs(big), v[:, i], big)
    return np.where((big < 0.0)[:, None], -v, v)


def cloud_normals_ref(cloud, radius, k=16, min_neighbors=5, orient=0, viewpoint=None, sweeps=6, want_v64=False):
    """-> dict(knn_index, n_used, normal [n, 3] float32, curvature [n] float32, cov [n, 6] float64, n_valid, n_normals, pairs); with
    want_v64 also "v64" (the float64 normal before it is rounded) and "eig" (the diagonal after the sweeps), for the CPU tests"""
    c = np.asarray(cloud, F)
    assert c.ndim == 2 and c.shape[1] >= 3 and 3 <= k <= KNN_MAX and 2 <= min_neighbors <= k and orient in (0, 1, 2)
    p = c[:, :3]
    n = len(p)
    knn, used = knn_ref(c, radius, k)
    pd = p.astype(D)
    S = np.zeros((n, 3), D)
    Q = np.zeros((n, 6), D)
    with np.errstate(all="ignore"):
        for s in range(k):                                                        # list order: one product and one sum per slot and moment
            on = s < used
            j = np.where(on, knn[:, s], 0)
            u = np.where(on[:, None], pd[j] - pd, 0.0) if n else np.zeros((0, 3), D)
            S = np.where(on[:, None], S + u, S)
            for col, (x, y) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                Q[:, col] = np.where(on, Q[:, col] + u[:, x] * u[:, y], Q[:, col])
        has = used >= min_neighbors
        M = (used + 1).astype(D)
        mu = S / M[:, None]
        C6 = np.stack([Q[:, col] / M - mu[:, x] * mu[:, y] for col, (x, y) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))], axis=1) if n else np.zeros((0, 6), D)
        C6 = np.where(has[:, None], C6, 0.0)
        a, V = jacobi_ref(C6, sweeps)
        l0, v = smallest_eigenpair(a, V)
        v = canonical_sign(v)
        if orient:
            w = (np.asarray(viewpoint, F).astype(D)[None, :] - pd) if orient == 1 else c[:, 3:6].astype(D)
            d = (v[:, 0] * w[:, 0] + v[:, 1] * w[:, 1]) + v[:, 2] * w[:, 2]
            v = np.where((d < 0.0)[:, None], -v, v)
        tot = (a[:, 0, 0] + a[:, 1, 1]) + a[:, 2, 2]
        curv = np.where(tot > 0.0, (np.where(l0 > 0.0, l0, 0.0) / np.where(tot > 0.0, tot, 1.0)).astype(F), F(0))
    normal = np.where(has[:, None], v.astype(F), F(0))
    res = {"knn_index": knn, "n_used": used, "normal": normal.astype(F), "curvature": np.where(has, curv, F(-1)).astype(F), "cov": C6,
           "n_valid": int(candidates(p).sum()), "n_normals": int(has.sum()), "pairs": int(pairs_per_query(p, p, F(radius)).sum()) if (used >= 0).any() else 0}
    if want_v64:
        res["v64"] = np.where(has[:, None], v, 0.0)
        res["eig"] = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    return res


def normal_compare_ref(normal_a, normal_b, index, min_cos, dist2=None, max_dist=None, signed=False):
    """-> dict(cos [n] float32, NaN where not compared; within [n_tol] int64; n_compared)"""
    a, b = np.asarray(normal_a, F)[:, :3], np.asarray(normal_b, F)[:, :3]
    idx = np.asarray(index, np.int32)
    n = len(a)
    cmp = (idx >= 0) & (idx < len(b))
    if dist2 is not None:
        md = F(max_dist)
        with np.errstate(invalid="ignore"):
            cmp &= np.asarray(dist2, F) <= F(md * md)
    bj = b[np.where(cmp, idx, 0)] if len(b) else np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        cmp &= np.isfinite(a).all(axis=1) & np.isfinite(bj).all(axis=1)
        ad, bd = a.astype(D), bj.astype(D)
        aa = (ad[:, 0] * ad[:, 0] + ad[:, 1] * ad[:, 1]) + ad[:, 2] * ad[:, 2]
        bb = (bd[:, 0] * bd[:, 0] + bd[:, 1] * bd[:, 1]) + bd[:, 2] * bd[:, 2]
        cmp &= (aa > 0.0) & (bb > 0.0)
        c = ((ad[:, 0] * bd[:, 0] + ad[:, 1] * bd[:, 1]) + ad[:, 2] * bd[:, 2]) / np.sqrt(aa * bb)
        if not signed:
            c = np.abs(c)
        mc = np.asarray(min_cos, D).reshape(-1)
        within = np.array([np.count_nonzero(cmp & (c >= t)) for t in mc], np.int64)
        cos = np.where(cmp, c.astype(F), F(np.nan)).astype(F)
    return {"cos": cos, "within": within, "n_compared": int(cmp.sum())}


def evaluate_normals_ref(recon, gt, tolerances, normals, crop=None):
    """the record of api.evaluate_cloud(..., normals=) / tsar_evaluate --normals=: the new fields only"""
    recon, gt = np.array(recon, F), np.array(gt, F)
    if crop is not None:
        for c in (recon, gt):
            with np.errstate(invalid="ignore"):
                inside = ((c[:, :3] >= np.asarray(crop[:3], F)) & (c[:, :3] <= np.asarray(crop[3:], F))).all(axis=1)
            c[~inside, :3] = np.nan
    tol = np.asarray(tolerances, F).reshape(-1)
    r = tol.max()
    acc = cloud_distance_ref(recon, gt, r)
    k, mn = normals.get("k", 16), normals.get("min_neighbors", 5)
    g = cloud_normals_ref(gt, normals["radius"], k, mn)
    deg = np.asarray(normals.get("tolerances_deg", (10.0, 30.0)), D).reshape(-1)
    s = normal_compare_ref(recon[:, 3:6], g["normal"], acc["index"], np.cos(np.deg2rad(deg)), acc["dist2"], r, normals.get("signed", False))
    nc = s["n_compared"]
    return {"normal_tolerances_deg": deg, "n_gt_normals": g["n_normals"], "n_normal_compared": nc, "n_normal_within": s["within"],
            "normal_accuracy": s["within"] / D(nc) if nc else np.zeros(len(deg), D)}


def stray_surface():
    """the 3000 surface points of cloud_neighbors_ref.stray_scene (z = 0.5 + 0.1 x + noise) and the surface's true unit normal"""
    from cloud_neighbors_ref import stray_scene
    nrm = np.array([-0.1, 0.0, 1.0]) / np.sqrt(1.01)
    return stray_scene()[:3000], nrm

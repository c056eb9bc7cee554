"""numpy restatement of tsar_cloud_neighbors (include/tsar.h) and of the rules of api.remove_outliers: the brute-force definition, an
n x n float32 d2 written operation for operation, chunked over the rows.  Shared by test_cloud_neighbors_cpu.py, test_outlier_cli_cpu.py
and test_gpu_cloud_neighbors.py; nothing here reads the library."""
import numpy as np

from cloud_distance_ref import candidates, pairs_per_query
from cloud_voxels_ref import evaluate_voxel_ref

KNN_MAX = 32


def cloud_neighbors_ref(cloud, radius, k=0, chunk_elems=1 << 22):
    """-> dict(count [n] int32, knn_dist2 [n, k] float32, n_valid, pairs).  Every operation is one float32 numpy operation (numpy fuses
    nothing): d2 = (dx * dx + dy * dy) + dz * dz over every pair of candidates; the point itself is left out by its index; a value above
    fl(R * R) enters as +inf; a row's k smallest values are the first k of the row sorted (a multiset: ties need no rule)."""
    p = np.asarray(cloud, np.float32)
    assert p.ndim == 2 and p.shape[1] >= 3 and 0 <= k <= KNN_MAX
    p = p[:, :3]
    n = len(p)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    cand = candidates(p)
    ci = np.flatnonzero(cand)
    pc = p[ci]
    count = np.full(n, -1, np.int32)
    knn = np.full((n, k), np.inf, np.float32)
    rows = max(1, chunk_elems // max(1, len(ci)))
    with np.errstate(over="ignore"):
        for s in range(0, len(ci), rows):
            qq = pc[s:s + rows]
            dx = qq[:, None, 0] - pc[None, :, 0]
            dy = qq[:, None, 1] - pc[None, :, 1]
            dz = qq[:, None, 2] - pc[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            d2 = np.where(d2 <= r2, d2, np.float32(np.inf))
            d2[np.arange(len(qq)), s + np.arange(len(qq))] = np.inf               # j != i, by index
            count[ci[s:s + rows]] = np.count_nonzero(d2 < np.inf, axis=1)
            if k:
                srt = np.sort(d2, axis=1)[:, :k]
                knn[ci[s:s + rows], :srt.shape[1]] = srt
    return {"count": count, "knn_dist2": knn, "n_valid": int(cand.sum()), "pairs": int(pairs_per_query(p, p, r).sum()) if len(ci) else 0}


def lower_median(values):
    """element (m - 1) // 2 of the m values sorted ascending; None when m = 0"""
    v = np.sort(np.asarray(values, np.float32).reshape(-1))
    return v[(len(v) - 1) // 2] if len(v) else None


def keep_mask_ref(cloud, radius, min_neighbors=None, k=None, ratio=2.0):
    """the boolean keep mask of api.remove_outliers: a candidate that passes every rule given"""
    assert min_neighbors is not None or k is not None
    res = cloud_neighbors_ref(cloud, radius, k or 0)
    keep = res["count"] >= 0
    if min_neighbors is not None:
        keep &= res["count"] >= min_neighbors
    if k is not None:
        s = res["knn_dist2"][:, k - 1]
        med = lower_median(s[np.isfinite(s)])
        if med is None:
            keep &= False
        else:
            q = np.float32(ratio)
            T = np.float32(np.float32(q * q) * med)
            keep &= s <= T
    return keep


def remove_outliers_ref(cloud, radius, min_neighbors=None, k=None, ratio=2.0):
    """-> (the kept rows, whole records in the cloud's order; the keep mask)"""
    c = np.asarray(cloud, np.float32)
    keep = keep_mask_ref(c, radius, min_neighbors, k, ratio)
    return c[keep].copy(), keep


def clean_ref(cloud, **clean):
    """-> (a copy with x y z of every record the rules remove set to NaN, the number of candidate records so removed)"""
    c = np.array(cloud, np.float32)
    keep = keep_mask_ref(c, clean["radius"], clean.get("min_neighbors"), clean.get("k"), clean.get("ratio", 2.0))
    removed = int(np.count_nonzero(candidates(c) & ~keep))
    c[~keep, :3] = np.nan
    return c, removed


def evaluate_clean_ref(recon, gt, tolerances, clean, voxel=None, crop=None):
    """the counts and float64 ratios of api.evaluate_cloud(..., clean=) / tsar_evaluate --clean_*: recon cleaned first, then the call as it was"""
    recon, removed = clean_ref(recon, **clean)
    res = evaluate_voxel_ref(recon, gt, tolerances, voxel=voxel, crop=crop)
    res["n_recon_cleaned"] = removed
    return res


def stray_scene():
    """the issue's scene: 3000 points on a slanted noisy surface, then 200 strays in the unit cube -> [3200, 3] float32"""
    rng = np.random.default_rng(0)
    xy = rng.random((3000, 2))
    z = 0.5 + 0.1 * xy[:, 0] + rng.normal(scale=0.002, size=3000)
    return np.concatenate([np.column_stack([xy, z]), rng.random((200, 3))]).astype(np.float32)

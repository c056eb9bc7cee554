"""numpy restatement of tsar_cloud_voxels (include/tsar.h) and of the voxel-averaged figures of api.evaluate_cloud / tsar_evaluate.  Shared by
test_cloud_voxels_cpu.py, test_voxel_cli_cpu.py and test_gpu_cloud_voxels.py; nothing here reads the library."""
import numpy as np

from cloud_distance_ref import candidates, cloud_distance_ref

MAX_EXTENT = 1 << 21


def voxel_cells(pts, origin, voxel):
    """floor(((double)p - (double)o) / (double)V) per axis, as float64"""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    return np.floor((p - np.asarray(origin, np.float32).astype(np.float64)[None, :]) / np.float64(np.float32(voxel)))


def cloud_voxels_ref(cloud, voxel, dist2=None, tolerances=None):
    """-> dict(rank [n] int32, rep / count [n_voxels] int32, keys [n_voxels] int64, d2f [n] float32 (NaN for a non-candidate), n_voxels, n_valid,
    and with dist2 and tolerances within [n_voxels, n_tol] int32).  Every operation is one numpy operation in the stated type."""
    c = np.asarray(cloud, np.float32)
    n = len(c)
    V = np.float64(np.float32(voxel))
    assert np.isfinite(V) and V > 0
    cand = candidates(c)
    idx = np.flatnonzero(cand)
    rank = np.full(n, -1, np.int32)
    d2f_all = np.full(n, np.nan, np.float32)
    n_tol = 0 if tolerances is None else len(np.asarray(tolerances).reshape(-1))
    out = {"rank": rank, "rep": np.zeros(0, np.int32), "count": np.zeros(0, np.int32), "keys": np.zeros(0, np.int64), "d2f": d2f_all, "n_voxels": 0,
           "n_valid": int(len(idx))}
    if tolerances is not None:
        out["within"] = np.zeros((0, n_tol), np.int32)
    if not len(idx):
        return out
    p = c[idx, :3]
    origin = p.min(axis=0)                                                # float32 minimum per axis
    cell = voxel_cells(p, origin, voxel)
    assert (cell >= 0).all() and (cell.max(axis=0) + 1 < MAX_EXTENT).all(), "2^21 cells or more on an axis: the library refuses this"
    ci = cell.astype(np.int64)
    key = (ci[:, 2] << 42) | (ci[:, 1] << 21) | ci[:, 0]
    keys, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    rank[idx] = inv.astype(np.int32)
    centre = origin.astype(np.float64)[None, :] + (cell + 0.5) * V       # one product, then one sum
    d = p.astype(np.float64) - centre
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d2f = d2.astype(np.float32)
    d2f_all[idx] = d2f
    code = (d2f.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    best = np.full(len(keys), np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, inv, code)
    out.update(rep=(best & np.uint64(0xffffffff)).astype(np.int32), count=count.astype(np.int32), keys=keys, n_voxels=int(len(keys)))
    if tolerances is not None:
        tol = np.asarray(tolerances, np.float32).reshape(-1)
        dd = np.asarray(dist2, np.float32)[idx]
        within = np.zeros((len(keys), n_tol), np.int32)
        with np.errstate(invalid="ignore"):
            for k, t in enumerate(tol):
                np.add.at(within[:, k], inv, (dd <= np.float32(t * t)).astype(np.int32))      # NaN and +inf never pass
        out["within"] = within
    return out


def voxel_share(within, count):
    """per tolerance (sum_v within[v][k] / count[v]) / n_voxels: one float64 division per term, the terms added one after another in ascending voxel
    order (np.cumsum is sequential; np.sum adds pairwise and is not the definition); 0 without voxels"""
    within = np.asarray(within, np.float64)
    count = np.asarray(count, np.float64)
    if len(count) == 0:
        return np.zeros(within.shape[1], np.float64)
    return np.cumsum(within / count[:, None], axis=0)[-1] / np.float64(len(count))


def crop_ref(cloud, crop):
    """-> (a copy with x y z of every record outside the closed box set to NaN, the number of candidate records so removed)"""
    c = np.array(cloud, np.float32)
    lo, hi = np.asarray(crop[:3], np.float32), np.asarray(crop[3:], np.float32)
    cand = candidates(c)
    with np.errstate(invalid="ignore"):
        inside = ((c[:, :3] >= lo) & (c[:, :3] <= hi)).all(axis=1) if len(c) else np.zeros(0, bool)
    c[~(cand & inside), :3] = np.nan
    return c, int(np.count_nonzero(cand & ~inside))


def evaluate_voxel_ref(recon, gt, tolerances, voxel=None, crop=None):
    """the counts and float64 ratios of api.evaluate_cloud(..., voxel=, crop=) / tsar_evaluate --voxel= --crop="""
    tol = np.asarray(tolerances, np.float32).reshape(-1)
    res = {}
    if crop is not None:
        (recon, res["n_recon_cropped"]), (gt, res["n_gt_cropped"]) = crop_ref(recon, crop), crop_ref(gt, crop)
    r = tol.max()
    a = cloud_distance_ref(recon, gt, r, tol)
    c = cloud_distance_ref(gt, recon, r, tol)
    acc = a["within"] / np.float64(a["n_valid_query"]) if a["n_valid_query"] else np.zeros(len(tol))
    com = c["within"] / np.float64(c["n_valid_query"]) if c["n_valid_query"] else np.zeros(len(tol))
    s = acc + com
    res.update({"n_accurate": a["within"], "n_complete": c["within"], "n_recon_valid": a["n_valid_query"], "n_gt_valid": c["n_valid_query"],
                "accuracy": acc, "completeness": com, "f1": np.where(s > 0, 2.0 * acc * com / np.where(s > 0, s, 1.0), 0.0)})
    if voxel is not None:
        va = cloud_voxels_ref(recon, voxel, a["dist2"], tol)
        vc = cloud_voxels_ref(gt, voxel, c["dist2"], tol)
        av, cv = voxel_share(va["within"], va["count"]), voxel_share(vc["within"], vc["count"])
        sv = av + cv
        res.update({"accuracy_voxel": av, "completeness_voxel": cv, "f1_voxel": np.where(sv > 0, 2.0 * av * cv / np.where(sv > 0, sv, 1.0), 0.0),
                    "n_recon_voxels": va["n_voxels"], "n_gt_voxels": vc["n_voxels"], "recon_voxels": va, "gt_voxels": vc,
                    "recon_cloud": np.asarray(recon, np.float32), "recon_dist2": a["dist2"]})       # what recon_voxels was computed from
    return res


def density_case():
    """-> (recon, gt, tau, voxel): a surface of 8 x 8 voxels of edge 1 (one layer), every coordinate a multiple of 1/16 so that cells and distances
    are exact.  gt holds one point per voxel.  recon's half x < 4 carries 10 points per voxel, all 2 tau off the surface; its half x >= 4 carries 1
    point per voxel, on the gt point.  Point-wise accuracy is 32 / 352 = 1 / 11; averaged over recon's 64 voxels it is exactly 0.5.  recon's
    voxel (x, y) has the number 8 y + x; its first 320 records are the dense half, voxel by voxel (x fastest), ten each."""
    tau, voxel = np.float32(1.0 / 32.0), np.float32(1.0)
    gt = np.array([[x + 0.5, y + 0.5, 0.0] for y in range(8) for x in range(8)], np.float32)
    dense = np.array([[x + (j + 1) / 16.0, y + 0.5, 1.0 / 16.0] for y in range(8) for x in range(4) for j in range(10)], np.float32)
    sparse = np.array([[x + 0.5, y + 0.5, 0.0] for y in range(8) for x in range(4, 8)], np.float32)
    return np.concatenate([dense, sparse]), gt, tau, voxel

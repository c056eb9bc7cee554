"""numpy restatement of tsar_cloud_distance (include/tsar.h): the brute-force definition in float32, chunked, and the float64 cell
function with the count of the pairs the 27-cell search looks at.  Shared by test_cloud_distance_cpu.py, test_evaluate_cli_cpu.py and
test_gpu_cloud_distance.py; nothing here reads the library."""
import numpy as np

CELL_FACTOR = 1.0 + 2.0 ** -10
MAX_EXTENT = 1 << 20


def _xyz(pts):
    p = np.asarray(pts, np.float32)
    assert p.ndim == 2 and p.shape[1] >= 3
    return p[:, :3]


def candidates(pts):
    """records whose x, y and z are all finite"""
    p = np.asarray(pts, np.float32)
    return np.isfinite(p[:, :3]).all(axis=1) if len(p) else np.zeros(0, bool)


def cloud_distance_ref(query, target, max_dist, tolerances=(), chunk_elems=1 << 22):
    """-> dict(dist2 [nq] float32, index [nq] int32, within [n_tol] int64, n_valid_query).  Every operation is one float32 numpy
    operation (numpy fuses nothing): d2 = (dx * dx + dy * dy) + dz * dz; the minimum over the candidate targets, kept when <= fl(R * R);
    the smallest index among equal minima (argmin returns the first, and the candidates are visited in index order)."""
    q = _xyz(query)
    t = _xyz(target)
    r = np.float32(max_dist)
    r2 = np.float32(r * r)
    qc, tc = candidates(q), candidates(t)
    tj = np.flatnonzero(tc)
    tt = t[tj]
    dist2 = np.full(len(q), np.inf, np.float32)
    index = np.full(len(q), -1, np.int32)
    qi = np.flatnonzero(qc)
    if len(tj) and len(qi):
        rows = max(1, chunk_elems // len(tj))
        with np.errstate(over="ignore"):
            for s in range(0, len(qi), rows):
                sel = qi[s:s + rows]
                qq = q[sel]
                dx = qq[:, None, 0] - tt[None, :, 0]
                dy = qq[:, None, 1] - tt[None, :, 1]
                dz = qq[:, None, 2] - tt[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                k = d2.argmin(axis=1)
                m = d2[np.arange(len(sel)), k]
                keep = m <= r2
                dist2[sel[keep]] = m[keep]
                index[sel[keep]] = tj[k[keep]]
    tol = np.asarray(tolerances, np.float32).reshape(-1)
    within = np.array([int(np.count_nonzero(dist2 <= np.float32(v * v))) for v in tol], np.int64)
    return {"dist2": dist2, "index": index, "within": within, "n_valid_query": int(qc.sum())}


def cell_edge(max_dist):
    return np.float64(np.float32(max_dist)) * CELL_FACTOR


def cell_coords(pts, origin, max_dist):
    """floor(((double)p - (double)o) / e) per axis, as float64 (a far query's coordinate may exceed any integer type's range)"""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    return np.floor((p - np.asarray(origin, np.float32).astype(np.float64)[None, :]) / cell_edge(max_dist))


def grid_of(target, max_dist):
    """(origin [3] float32, extent [3] int) of the candidate targets' grid, or None without a candidate"""
    t = _xyz(target)
    tt = t[candidates(t)]
    if not len(tt):
        return None
    origin = tt.min(axis=0)
    extent = cell_coords(tt.max(axis=0)[None, :], origin, max_dist)[0] + 1
    return origin, extent


def pairs_per_query(query, target, max_dist):
    """per query the number of candidate targets in the 27 cells around its own (0 for a query that is no candidate)"""
    q = _xyz(query)
    t = _xyz(target)
    g = grid_of(t, max_dist)
    qc = candidates(q)
    out = np.zeros(len(q), np.int64)
    if g is None or not qc.any():
        return out
    origin, extent = g
    assert (extent < MAX_EXTENT).all()
    dims = extent.astype(np.int64) + 4                           # cells -2 .. extent + 1, shifted by 2
    ct = cell_coords(t[candidates(t)], origin, max_dist).astype(np.int64) + 2
    cq = np.clip(cell_coords(q[qc], origin, max_dist), -2, extent[None, :] + 1).astype(np.int64) + 2
    key = lambda c: (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    cells, counts = np.unique(key(ct), return_counts=True)
    total = np.zeros(len(cq), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                c = cq + np.array([dx, dy, dz], np.int64)[None, :]
                ok = ((c >= 0) & (c < dims[None, :])).all(axis=1)
                k = key(c)
                pos = np.searchsorted(cells, k)
                pos[pos == len(cells)] = 0
                total += np.where(ok & (cells[pos] == k), counts[pos], 0)
    out[qc] = total
    return out


def pairs_ref(query, target, max_dist):
    """the number of (candidate query, candidate target) pairs with the target in one of the 27 cells around the query's"""
    return int(pairs_per_query(query, target, max_dist).sum())


def evaluate_ref(recon, gt, tolerances):
    """the counts and float64 ratios of api.evaluate_cloud / tsar_evaluate"""
    tol = np.asarray(tolerances, np.float32).reshape(-1)
    r = tol.max()
    a = cloud_distance_ref(recon, gt, r, tol)
    c = cloud_distance_ref(gt, recon, r, tol)
    acc = a["within"] / np.float64(a["n_valid_query"]) if a["n_valid_query"] else np.zeros(len(tol))
    com = c["within"] / np.float64(c["n_valid_query"]) if c["n_valid_query"] else np.zeros(len(tol))
    s = acc + com
    f1 = np.where(s > 0, 2.0 * acc * com / np.where(s > 0, s, 1.0), 0.0)
    return {"n_accurate": a["within"], "n_complete": c["within"], "n_recon_valid": a["n_valid_query"], "n_gt_valid": c["n_valid_query"],
            "accuracy": acc, "completeness": com, "f1": f1}

"""numpy restatement of tsar_cloud_render and tsar_depth_compare from the text of include/tsar.h, and the scene the render's tests share.
Used by test_cloud_render_cpu.py and test_gpu_cloud_render.py; nothing here reads the library.  Every operation is one numpy operation in
the stated type (numpy contracts nothing into a fused multiply-add)."""
import functools

import numpy as np

F = np.float32
EMPTY32 = np.uint32(0xFFFFFFFF)
EMPTY64 = np.uint64(0xFFFFFFFFFFFFFFFF)
THIN_SEED = 11          # the seed of the quarter the scene's cloud is thinned to (thinned_cloud)


def projection(K, R, t):
    """P = K [R | t]: float64 products and sums of the float32 elements, in the header's order, rounded once to float32 -> [3, 4] float32"""
    K = np.asarray(K, F).reshape(3, 3).astype(np.float64)
    Rt = np.concatenate([np.asarray(R, F).reshape(3, 3), np.asarray(t, F).reshape(3, 1)], axis=1).astype(np.float64)
    P = np.empty((3, 4), np.float64)
    for k in range(3):
        for j in range(4):
            P[k, j] = (K[k, 0] * Rt[0, j] + K[k, 1] * Rt[1, j]) + K[k, 2] * Rt[2, j]
    return P.astype(F)


def landings(cloud, K, R, t, w, h, radius=0.0, max_px=8):
    """-> (lands [n] bool, xi, yi [n] int64, p2 [n] float32, s [n] int64); xi, yi and s are 0 where the point does not land"""
    c = np.asarray(cloud, F)
    P = projection(K, R, t)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(all="ignore"):
        cand = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        p = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        assert all(q.dtype == F for q in p)
        xq, yq = p[0] / p[2], p[1] / p[2]
        xf, yf = np.floor(xq + F(0.5)), np.floor(yq + F(0.5))
        lands = cand & (p[2] > 0) & (p[2] < np.inf) & (xf >= 0) & (xf <= F(w - 1)) & (yf >= 0) & (yf <= F(h - 1))
        fr = F(np.asarray(K, F).reshape(3, 3)[0, 0]) * F(radius)
        assert fr.dtype == F and np.isfinite(fr) and fr >= 0
        if float(radius) > 0:
            sf = np.minimum(np.floor(fr / p[2] + F(0.5)), F(max_px))
        else:
            sf = np.zeros(len(c), F)
    xi = np.where(lands, xf, 0).astype(np.int64)
    yi = np.where(lands, yf, 0).astype(np.int64)
    s = np.where(lands, sf, 0).astype(np.int64)
    return lands, xi, yi, p[2].astype(F), s


def cloud_render_ref(cloud, K, R, t, w, h, radius=0.0, max_px=8, occlusion_diff=0.02, depth_diff=0.01, min_points=1, max_splats=1 << 34):
    """-> dict(depth [h, w] float32, count [h, w] uint8, index [h, w] int32, n_splats, refused) and the intermediate planes Zc, Zo (float32, NaN
    where there is none), landed, visible (bool) and support (int64).  refused: n_splats > max_splats, and then no plane is in the dict."""
    c = np.asarray(cloud, F)
    n = len(c)
    lands, xi, yi, p2, s = landings(c, K, R, t, w, h, radius, max_px)
    x0, x1 = np.maximum(xi - s, 0), np.minimum(xi + s, w - 1)
    y0, y1 = np.maximum(yi - s, 0), np.minimum(yi + s, h - 1)
    n_splats = int(((x1 - x0 + 1) * (y1 - y0 + 1))[lands].sum())
    if n_splats > max_splats:
        return {"n_splats": n_splats, "refused": True}
    idx = np.flatnonzero(lands)
    at = yi[idx] * w + xi[idx]
    bits = p2[idx].view(np.uint32)
    # centre buffer: the minimal code bits(p_2) << 32 | i
    zc = np.full(w * h, EMPTY64, np.uint64)
    np.minimum.at(zc, at, (bits.astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64))
    landed = zc != EMPTY64
    # occluder buffer: the minimal bits(p_2) over the clipped footprints
    zo = np.full(w * h, EMPTY32, np.uint32)
    S = int(s[idx].max()) if len(idx) else 0
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            xx, yy = xi[idx] + dx, yi[idx] + dy
            m = (s[idx] >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            np.minimum.at(zo, (yy * w + xx)[m], bits[m])
    with np.errstate(all="ignore"):
        Zc = np.where(landed, (zc >> np.uint64(32)).astype(np.uint32).view(F), F(np.nan)).astype(F)
        Zo = np.where(zo != EMPTY32, zo.view(F), F(np.nan)).astype(F)
        assert not (landed & ~(Zo <= Zc)).any()                              # the centre pixel is covered
        visible = landed & (Zc - Zo <= F(occlusion_diff) * Zo)
        near = np.abs(p2[idx] - Zc[at]) <= F(depth_diff) * Zc[at]
    support = np.zeros(w * h, np.int64)
    np.add.at(support, at[near], 1)
    kept = visible & (support >= int(min_points))
    winner = (zc & np.uint64(0xFFFFFFFF)).astype(np.int64)
    shape = (h, w)
    return {"depth": np.where(kept, Zc, F(0)).astype(F).reshape(shape), "count": np.minimum(support, 255).astype(np.uint8).reshape(shape),
            "index": np.where(kept, winner, -1).astype(np.int32).reshape(shape), "n_splats": n_splats, "refused": False,
            "Zc": Zc.reshape(shape), "Zo": Zo.reshape(shape), "landed": landed.reshape(shape), "visible": visible.reshape(shape), "support": support.reshape(shape),
            "n": n}


def depth_compare_ref(depth, gt, tolerances, mask=None):
    """-> dict(n_gt, n_both, within [n_tol] int64, n_front, n_behind, error [same shape] float32 with NaN off the n_both pixels)"""
    D, G = np.asarray(depth, F).reshape(-1), np.asarray(gt, F).reshape(-1)
    tol = np.asarray(tolerances, F).reshape(-1)
    with np.errstate(all="ignore"):
        is_gt = (G > 0) & (G < np.inf)
        if mask is not None:
            is_gt &= np.asarray(mask).reshape(-1) != 0
        both = is_gt & (D > 0) & (D < np.inf)
        diff = D - G
        assert diff.dtype == F
        within = np.array([np.count_nonzero(both & (np.abs(diff) <= tk * G)) for tk in tol], np.int64)
        t0 = tol[0] * G
        err = np.where(both, diff / G, F(np.nan)).astype(F)
    return {"n_gt": int(np.count_nonzero(is_gt)), "n_both": int(np.count_nonzero(both)), "within": within, "n_front": int(np.count_nonzero(both & (diff < -t0))),
            "n_behind": int(np.count_nonzero(both & (diff > t0))), "error": err.reshape(np.asarray(depth).shape)}


def ratios(counts):
    """the float64 ratios a caller forms from the counts (0 where a denominator is 0)"""
    nb, ng = np.float64(counts["n_both"]), np.float64(counts["n_gt"])
    w = np.asarray(counts["within"], np.int64).astype(np.float64)
    return {"accuracy": w / nb if nb else np.zeros(len(w)), "completeness": w / ng if ng else np.zeros(len(w)), "cover": float(nb / ng) if ng else 0.0}


def evaluate_depth_maps_ref(depths, cloud, K, R, t, tolerances, radius, masks=None, **render_kw):
    """the composition api.evaluate_depth_maps states: per view a render at the map's size and a comparison; the total adds the counts first"""
    views = []
    for v, d in enumerate(depths):
        d = np.asarray(d, F)
        h, w = d.shape
        r = cloud_render_ref(cloud, K[v], R[v], t[v], w, h, radius, **render_kw)
        c = depth_compare_ref(d, r["depth"], tolerances, None if masks is None else masks[v])
        c["n_splats"] = r["n_splats"]
        views.append(c)
    total = {k: sum(c[k] for c in views) for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats")}
    total["within"] = np.sum([c["within"] for c in views], axis=0).astype(np.int64)
    return views, total


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
def back_project(depth, K, R, t):
    """the world points of a depth map's pixels with a depth, float64 -> [m, 3] float32: X = R^T (d K^-1 (u, v, 1) - t)"""
    d = np.asarray(depth, np.float64)
    h, w = d.shape
    v, u = np.mgrid[0:h, 0:w]
    ok = (d > 0) & np.isfinite(d)
    pix = np.stack([u[ok], v[ok], np.ones(ok.sum())], 0).astype(np.float64)
    cam = np.linalg.inv(np.asarray(K, np.float64)) @ pix * d[ok][None, :]
    return (np.asarray(R, np.float64).T @ (cam - np.asarray(t, np.float64).reshape(3, 1))).T.astype(F)


@functools.lru_cache(maxsize=None)
def scene():
    """synth.make_scene(160, 120, 3, seed=5, textureless=True, all_gt=True, step=0.2) and the cloud of its three source views' ground-truth maps
    back-projected (57 600 points; the render's target is view 0) -> (scene, cloud [n, 3] float32, spacing = 5 / f)"""
    from tsar_mvs_amd import synth
    sc = synth.make_scene(160, 120, 3, seed=5, textureless=True, all_gt=True, step=0.2)
    cloud = np.concatenate([back_project(sc.meta["gt_all"][v][0].numpy(), sc.K[v], sc.R[v], sc.t[v]) for v in (1, 2, 3)])
    return sc, np.ascontiguousarray(cloud), float(5.0 / float(sc.K[0][0, 0]))


@functools.lru_cache(maxsize=None)
def thinned_cloud():
    """a quarter of scene()'s cloud, drawn at random with THIN_SEED, in the cloud's order"""
    _, cloud, _ = scene()
    keep = np.sort(np.random.default_rng(THIN_SEED).permutation(len(cloud))[: len(cloud) // 4])
    return np.ascontiguousarray(cloud[keep])

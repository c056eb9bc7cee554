"""numpy restatement of tsar_cloud_render_oriented from the text of include/tsar.h, and the slanted scene its tests share.  Used by
test_cloud_splat_cpu.py and test_gpu_cloud_splat.py; nothing here reads the library.  Every operation is one numpy operation in the stated
type (numpy contracts nothing into a fused multiply-add).  The landing and P are cloud_render_ref's."""
import functools

import numpy as np

from cloud_render_ref import EMPTY32, EMPTY64, F, landings, projection


def splat_view(K, R, t):
    """the host side: A = K R (P's first three columns, float32), M = A^-1 by cofactors and C = -R^T t in float64, each element rounded once
    -> (M [3, 3] float32, C [3] float32), or None where the header refuses (det == 0, a non-finite element)"""
    A = projection(K, R, t)[:, :3].astype(np.float64)
    Rd, td = np.asarray(R, F).reshape(3, 3).astype(np.float64), np.asarray(t, F).reshape(3).astype(np.float64)
    c = np.empty((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                c[i, j] = A[i1, j1] * A[i2, j2] - A[i1, j2] * A[i2, j1]
        det = (A[0, 0] * c[0, 0] + A[0, 1] * c[0, 1]) + A[0, 2] * c[0, 2]
        if det == 0:
            return None
        M = (c.T / det).astype(F)                                            # M[j][i] = c[i][j] / det
        C = np.array([-((Rd[0, j] * td[0] + Rd[1, j] * td[1]) + Rd[2, j] * td[2]) for j in range(3)]).astype(F)
    if not (np.isfinite(M).all() and np.isfinite(C).all()):
        return None
    return M, C


def cloud_render_oriented_ref(cloud, normals, K, R, t, w, h, radius=0.0, max_px=8, occlusion_diff=0.02, depth_diff=0.01, min_points=1, max_splats=1 << 34):
    """normals: [n, >= 3] float32, or None = the records' floats 3..5 -> cloud_render_ref's dict plus "occluder" ([h, w] float32, 0 where nothing
    covers) and "n_covered".  refused: n_splats > max_splats, and then no plane is in the dict."""
    c = np.asarray(cloud, F)
    nrm = np.asarray(c[:, 3:6] if normals is None else normals, F)[:, :3]
    M, C = splat_view(K, R, t)
    lands, xi, yi, p2, s = landings(c, K, R, t, w, h, radius, max_px)
    x0, x1 = np.maximum(xi - s, 0), np.minimum(xi + s, w - 1)
    y0, y1 = np.maximum(yi - s, 0), np.minimum(yi + s, h - 1)
    n_splats = int(((x1 - x0 + 1) * (y1 - y0 + 1))[lands].sum())
    if n_splats > max_splats:
        return {"n_splats": n_splats, "refused": True}
    idx = np.flatnonzero(lands)
    at = yi[idx] * w + xi[idx]
    cbits = p2[idx].view(np.uint32)
    zc = np.full(w * h, EMPTY64, np.uint64)
    np.minimum.at(zc, at, (cbits.astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64))
    landed = zc != EMPTY64
    # per landing point
    X, nn = c[idx, :3], nrm[idx]
    r2 = F(radius) * F(radius)
    with np.errstate(all="ignore"):
        oriented = np.isfinite(nn).all(axis=1) & (nn != 0).any(axis=1)
        a = [X[:, k] - C[k] for k in range(3)]
        num = (nn[:, 0] * a[0] + nn[:, 1] * a[1]) + nn[:, 2] * a[2]
        g = [(M[0, j] * nn[:, 0] + M[1, j] * nn[:, 1]) + M[2, j] * nn[:, 2] for j in range(3)]
        assert num.dtype == F and all(q.dtype == F for q in a + g) and r2.dtype == F
    zo = np.full(w * h, EMPTY32, np.uint32)
    n_covered = 0
    S = int(s[idx].max()) if len(idx) else 0
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            xx, yy = xi[idx] + dx, yi[idx] + dy
            m = (s[idx] >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            if dx == 0 and dy == 0:
                value, cover = p2[idx], m
            else:
                u, v = xx.astype(F), yy.astype(F)
                with np.errstate(all="ignore"):
                    den = g[0] * u + (g[1] * v + g[2])
                    z = num / den
                    e = [z * (M[k, 0] * u + (M[k, 1] * v + M[k, 2])) - a[k] for k in range(3)]
                    q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    assert z.dtype == F and q.dtype == F
                    cover = m & np.where(oriented, (z > 0) & (z < np.inf) & (q <= r2), True)
                value = np.where(oriented, z, p2[idx]).astype(F)
            n_covered += int(cover.sum())
            np.minimum.at(zo, (yy * w + xx)[cover], value[cover].view(np.uint32))
    with np.errstate(all="ignore"):
        Zc = np.where(landed, (zc >> np.uint64(32)).astype(np.uint32).view(F), F(np.nan)).astype(F)
        Zo = np.where(zo != EMPTY32, zo.view(F), F(np.nan)).astype(F)
        assert not (landed & ~(Zo <= Zc)).any()                              # the centre pixel is covered at p_2
        visible = landed & (Zc - Zo <= F(occlusion_diff) * Zo)
        near = np.abs(p2[idx] - Zc[at]) <= F(depth_diff) * Zc[at]
    support = np.zeros(w * h, np.int64)
    np.add.at(support, at[near], 1)
    kept = visible & (support >= int(min_points))
    winner = (zc & np.uint64(0xFFFFFFFF)).astype(np.int64)
    shape = (h, w)
    return {"depth": np.where(kept, Zc, F(0)).astype(F).reshape(shape), "count": np.minimum(support, 255).astype(np.uint8).reshape(shape),
            "index": np.where(kept, winner, -1).astype(np.int32).reshape(shape), "occluder": np.where(zo != EMPTY32, zo.view(F), F(0)).astype(F).reshape(shape),
            "n_splats": n_splats, "n_covered": n_covered, "refused": False, "Zc": Zc.reshape(shape), "Zo": Zo.reshape(shape), "landed": landed.reshape(shape),
            "visible": visible.reshape(shape), "support": support.reshape(shape), "n": len(c)}


# ---- the slanted scene -------------------------------------------------------------------------------------------------------------------
SLANT_W, SLANT_H = 160, 120
SLANT_N_FG, SLANT_N_BG = 6000, 40000


def slant_spacing(slope):
    """the foreground's point spacing on its own surface: sqrt(area / points), the rectangle being 0.5 * sqrt(1 + slope^2) by 0.4"""
    return float(np.sqrt(0.5 * np.sqrt(1.0 + slope * slope) * 0.4 / SLANT_N_FG))


def slant_camera():
    """a general camera: unequal focal lengths and a skew term in K, a rotation about all three axes, a translation -> (K, R, t) float32"""
    K = np.array([[200.0, 0.7, 80.0], [0.0, 198.0, 60.0], [0.0, 0.0, 1.0]], F)
    ax, ay, az = 0.31, -0.47, 0.23
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return K, (Rz @ Ry @ Rx).astype(F), np.array([0.4, -1.3, 2.1], F)


@functools.lru_cache(maxsize=None)
def slanted_scene(slope, seed=3):
    """In the camera's frame: a foreground plane z = 2 + slope * x over |x| < 0.25, |y| < 0.2 (SLANT_N_FG random points, first in the cloud)
    before a background plane z = 6 (SLANT_N_BG random points over the whole view), taken to the world of slant_camera().
    -> (cloud [n, 6] float32: position and the plane's unit normal, K, R, t)"""
    K, R, t = slant_camera()
    rng = np.random.default_rng(seed)
    fx, fy = rng.uniform(-0.25, 0.25, SLANT_N_FG), rng.uniform(-0.2, 0.2, SLANT_N_FG)
    fg = np.stack([fx, fy, 2.0 + slope * fx], 1)
    bg = np.stack([rng.uniform(-2.6, 2.6, SLANT_N_BG), rng.uniform(-2.0, 2.0, SLANT_N_BG), np.full(SLANT_N_BG, 6.0)], 1)
    n_fg = np.array([slope, 0.0, -1.0]) / np.sqrt(slope * slope + 1.0)
    cam = np.concatenate([fg, bg])
    nrm = np.concatenate([np.tile(n_fg, (SLANT_N_FG, 1)), np.tile([0.0, 0.0, 1.0], (SLANT_N_BG, 1))])
    Rd, td = R.astype(np.float64), t.astype(np.float64)
    cloud = np.concatenate([(cam - td) @ Rd, nrm @ Rd], axis=1).astype(F)   # X = R^T (X_cam - t), n = R^T n_cam
    return np.ascontiguousarray(cloud), K, R, t


def slant_silhouette(slope):
    """the pixels whose centre's ray meets the foreground rectangle, float64 -> [h, w] bool"""
    K, _, _ = slant_camera()
    v, u = np.mgrid[0:SLANT_H, 0:SLANT_W]
    d = np.linalg.inv(K.astype(np.float64)) @ np.stack([u.ravel(), v.ravel(), np.ones(u.size)]).astype(np.float64)
    with np.errstate(all="ignore"):
        z = 2.0 / (d[2] - slope * d[0])                                       # z * d_z = 2 + slope * z * d_x
        inside = (z > 0) & (np.abs(z * d[0]) < 0.25) & (np.abs(z * d[1]) < 0.2)
    return inside.reshape(SLANT_H, SLANT_W)


def slant_figures(one_pixel, render, slope):
    """of a render (a dict with "depth" and "index") of slanted_scene(slope), against the one-pixel render of the same cloud:
    -> (foreground pixels, those the render hides, background pixels it shows inside the analytic silhouette)"""
    fg = (one_pixel["index"] >= 0) & (one_pixel["index"] < SLANT_N_FG)
    hidden = fg & (render["depth"] == 0)
    through = slant_silhouette(slope) & (render["index"] >= SLANT_N_FG)
    return int(fg.sum()), int(hidden.sum()), int(through.sum())

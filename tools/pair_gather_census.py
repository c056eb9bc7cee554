#!/usr/bin/env python3
"""tools/pair_gather_census.py [width height views pixels] — how often the 16 bytes gathered at a row tap's quad-texture entry hold
the next tap's entry too (pm_tap_r5.h PAIR), on planes drawn the way the initialisation draws them, without a GPU.

For random pixels of the reference view a plane is drawn as pm_full_kernel<INIT> draws it (a Marsaglia unit vector turned towards
the camera, a disparity uniform over the depth range), one row of the box-11 window (six taps 2 px apart) is projected into every
source view of synth.make_cameras through the plane's homography, and each tap's element index lin = floor(v) (w + 2) + floor(u) is
formed as tap_position forms it.  Counted over the pairs (0,1), (2,3), (4,5) of rows that project inside the source image:
k = lin[j+1] - lin[j]; the pair is covered when 0 <= k <= 3.  float64 throughout: a census, not a restatement of the kernel's bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def draw_planes(rng, K0, xs, ys, depth_min, depth_max):
    """unit normals facing the camera and plane offsets d (n . X + d = 0 in reference-camera coordinates) through pixel (x, y) at a
    depth of uniform disparity"""
    n = xs.size
    a, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    s = a * a + b * b
    bad = s >= 1.0
    while bad.any():
        a[bad], b[bad] = rng.uniform(-1, 1, int(bad.sum())), rng.uniform(-1, 1, int(bad.sum()))
        s = a * a + b * b
        bad = s >= 1.0
    sq = np.sqrt(1.0 - s)
    nrm = np.stack([2 * a * sq, 2 * b * sq, 1 - 2 * s], 1)
    ray = np.linalg.solve(K0, np.stack([xs, ys, np.ones(n)], 0).astype(np.float64)).T     # z = 1
    flip = (nrm * ray).sum(1) > 0
    nrm[flip] = -nrm[flip]
    depth = 1.0 / rng.uniform(1.0 / depth_max, 1.0 / depth_min, n)
    d = -(nrm * (ray * depth[:, None])).sum(1)
    return nrm, d


def census(w=6048, h=4032, n_src=10, pixels=200000, seed=1, cam_seed=42, step=0.03, depth_min=3.2, depth_max=7.5, normals=None):
    """normals: None = the initialisation's draw; else a fixed (3,) normal for every pixel (a converged-like slanted plane)"""
    from tsar_mvs_amd import synth
    K, R, t = (m.astype(np.float64) for m in synth.make_cameras(w, h, n_src, cam_seed, step))
    rng = np.random.default_rng(seed)
    xs = rng.integers(5, w - 5, pixels).astype(np.float64)
    ys = rng.integers(5, h - 5, pixels).astype(np.float64)
    nrm, d = draw_planes(rng, K[0], xs, ys, depth_min, depth_max)
    if normals is not None:
        nv = np.asarray(normals, np.float64)
        nv = nv / np.linalg.norm(nv)
        ray = np.linalg.solve(K[0], np.stack([xs, ys, np.ones(pixels)], 0)).T
        depth = -d / (nrm * ray).sum(1)
        nrm = np.broadcast_to(nv, nrm.shape).copy()
        d = -(nrm * (ray * depth[:, None])).sum(1)
    row = rng.integers(0, 6, pixels) * 2 - 5                                     # one window row per pixel
    K0inv = np.linalg.inv(K[0])
    qp = w + 2
    ks, same_row = [], []
    for v in range(1, n_src + 1):
        Rr = R[v] @ R[0].T
        tr = t[v] - Rr @ t[0]
        H = K[v] @ (Rr[None] - tr[None, :, None] * nrm[:, None, :] / d[:, None, None]) @ K0inv          # (pixels, 3, 3)
        px = xs[:, None] + (2 * np.arange(6) - 5)[None]
        p = np.stack([px, np.broadcast_to((ys + row)[:, None], px.shape), np.ones_like(px)], 2)       # (pixels, 6, 3)
        q = np.einsum("nij,ntj->nti", H, p)
        Z = q[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, vv = q[..., 0] / Z, q[..., 1] / Z
        inside = ((Z > 0) & (u >= 0) & (u <= w - 1) & (vv >= 0) & (vv <= h - 1)).all(1)
        iu, iv = np.floor(u[inside]).astype(np.int64), np.floor(vv[inside]).astype(np.int64)
        lin = iv * qp + iu
        ks.append((lin[:, 1::2] - lin[:, 0::2]).ravel())
        same_row.append((iv[:, 1::2] == iv[:, 0::2]).ravel())
    k = np.concatenate(ks)
    same_row = np.concatenate(same_row)
    out = {"pairs": int(k.size), "covered": float(((k >= 0) & (k <= 3)).mean()), "same_row": float(same_row.mean()),
           "below": float((k < 0).mean()), "above": float((k > 3).mean())}
    for i in range(4):
        out[f"k{i}"] = float((k == i).mean())
    return out


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:5]]
    args = dict(zip(("w", "h", "n_src", "pixels"), a))
    r = census(**args)
    print("random planes :", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    r = census(normals=(0.3, 0.2, -0.93), **args)
    print("slanted plane :", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})

"""The geometric-consistency term (include/tsar.h, pm_core.h geom_term) restated in numpy float32, operation for operation, and that
restatement held to the float64 closed form of the same reprojection; the CPU oracle's own statement of the term (oracle/tsar_oracle.c
orc_geom_term, its multi-view cost and orc_pm_rescore) held to the numpy restatement bit for bit; the register budget of the kernels that
carry the term.  No GPU: tests/test_gpu_geom.py and tests/test_gpu_call_parity.py hold the kernels to these."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tsar_mvs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MAXCOST = F32(2.0)


def geom_term(F, B, depth_v, x, y, D, weight, clip):
    """lambda * e for hypotheses of depth D at reference pixels (x, y) (int arrays) against view v's depth map [h, w]; F, B the view's
    float32 3 x 4 matrices (Matcher.get_geom_matrices).  The sequence of include/tsar.h, each numpy float32 operation one IEEE
    operation; numpy's float32 '/' and sqrt are correctly rounded, like the kernels' persp_divide_exact and sqrt_rsq_exact."""
    F = np.asarray(F, F32)
    B = np.asarray(B, F32)
    h, w = depth_v.shape
    D = np.asarray(D, F32)
    X = np.asarray(x).astype(F32)
    Y = np.asarray(y).astype(F32)
    tau = F32(clip)
    with np.errstate(all="ignore"):
        xd, yd = X * D, Y * D
        a, b, s = (((F[r, 0] * xd + F[r, 1] * yd) + F[r, 2] * D) + F[r, 3] for r in range(3))
        u, v = a / s, b / s
        c, r = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        inside = (s > 0) & (c >= 0) & (c <= F32(w - 1)) & (r >= 0) & (r <= F32(h - 1))
        ci = np.where(inside, c, 0).astype(np.int64)
        ri = np.where(inside, r, 0).astype(np.int64)
        Dv = np.where(inside, depth_v[ri, ci], F32(0)).astype(F32)
        cd, rd = c * Dv, r * Dv
        p0, p1, p2 = (((B[k, 0] * cd + B[k, 1] * rd) + B[k, 2] * Dv) + B[k, 3] for k in range(3))
        xq, yq = p0 / p2, p1 / p2
        dx, dy = xq - X, yq - Y
        e2 = dx * dx + dy * dy
        root = np.sqrt(np.clip(np.nan_to_num(e2, nan=F32(2.0 ** -100)), F32(2.0 ** -100), F32(2.0 ** 100))).astype(F32)
        e = np.where(e2 < F32(2.0 ** -100), F32(0), root).astype(F32)
        ok = inside & (Dv > 0) & (p2 > 0) & (e2 < tau * tau)
        e = np.where(ok, np.minimum(e, tau), tau).astype(F32)
        return (F32(weight) * e).astype(F32)


def combine_view_costs(per_view, n_best, cost_comb=1):
    """multiview_cost (pm_core.h) in numpy over per_view = [(view, cost with its term, valid), ...] in the order the views are
    walked (the selection's): the last view attaining the minimum is the best view, the costs sorted, nb = min(valid, n_best) under
    best-N (cost_comb 1) and the number of valid views under every other combination -- the sorted list then also holds the invalid
    views at MAXCOST + lambda e, and the first nb entries are summed whatever they are."""
    h, w = per_view[0][1].shape
    cmin = np.full((h, w), np.inf, F32)
    bv = np.full((h, w), -1, np.int32)
    nvalid = np.zeros((h, w), np.int32)
    for v, c, valid in per_view:
        take = c <= cmin
        bv = np.where(take, v, bv)
        cmin = np.minimum(cmin, c)
        nvalid += valid
    srt = np.sort(np.stack([c for _, c, _ in per_view]), axis=0)
    nb = np.minimum(nvalid, n_best) if cost_comb == 1 else nvalid
    cost = np.zeros((h, w), F32)
    for k in range(srt.shape[0]):
        cost = np.where(k < nb, (cost + srt[k]).astype(F32), cost)
    with np.errstate(all="ignore"):
        cost = np.where(nb > 0, (cost / nb.astype(F32)).astype(F32), MAXCOST)
        ratio = (srt[0] / srt[1]).astype(F32) if srt.shape[0] >= 2 else np.zeros((h, w), F32)
    ratio = np.where(nb > 0, ratio, F32(0))
    bv = np.where(nb > 0, bv, -1)
    return cost, bv, ratio


def expected_cost_planes(orc, matrices, maps, planes, n_best, weight, clip, cost_comb=1, views=None, photometric=None):
    """what pm_cost_planes must return with `maps` installed: `orc`'s photometric cost per view (the oracle's pm_cost, which carries no
    term), the numpy restatement of the term, the combination of multiview_cost (pm_core.h) in numpy.  matrices[v] = (F, B) of view v.
    views: the selected views in selection order (default: every source view).  photometric: {view: cost [h, w]} from elsewhere (the
    device's own per-view score, say) in place of the oracle's pm_cost."""
    h, w = planes.shape[:2]
    n_views = len(maps)
    ys, xs = np.mgrid[0:h, 0:w]
    D = np.empty((h, w), F32)
    per_view = []
    for y in range(h):
        for x in range(w):
            D[y, x] = orc.depth_from_plane(planes[y, x], x, y)
    for v in (range(1, n_views) if views is None else views):
        if photometric is not None:
            c = np.asarray(photometric[v], F32)
        else:
            c = np.empty((h, w), F32)
            for y in range(h):
                for x in range(w):
                    c[y, x] = orc.pm_cost(v, x, y, planes[y, x])
        c = np.minimum(c, MAXCOST)
        valid = c < MAXCOST
        F, B = matrices[v]
        g = geom_term(F, B, maps[v], xs, ys, D, weight, clip) if maps[v] is not None else np.zeros((h, w), F32)
        per_view.append((v, (c + g).astype(F32), valid))
    return combine_view_costs(per_view, n_best, cost_comb)


def relative_pose(K, R, t, v):
    """float64 K_ref, K_v, R, t of view v relative to the reference camera (tsar_api.hip derive_cameras, cam_scale 1)"""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    if v == 0:                                  # the reference camera is exactly K[I|0] (derive_cameras)
        return K[0], K[0], np.eye(3), np.zeros(3)
    Rrel = R[v] @ R[0].T
    trel = t[v] - Rrel @ t[0]
    return K[0], K[v], Rrel, trel


def matrices64(K, R, t, v):
    """F = [K_v R K_ref^-1 | K_v t], B = [K_ref R^T K_v^-1 | -K_ref R^T t] in float64"""
    K0, Kv, Rr, tr = relative_pose(K, R, t, v)
    F = np.hstack([Kv @ Rr @ np.linalg.inv(K0), (Kv @ tr)[:, None]])
    B = np.hstack([K0 @ Rr.T @ np.linalg.inv(Kv), (-(K0 @ Rr.T) @ tr)[:, None]])
    return F, B


def closed_form64(K, R, t, v, depth_v, x, y, D, clip):
    """e in float64: the point D K_ref^-1 (x, y, 1) into view v, its nearest pixel, that pixel back with view v's depth, into the
    reference image; the distance to (x, y), tau where the chain breaks"""
    K0, Kv, Rr, tr = relative_pose(K, R, t, v)
    h, w = depth_v.shape
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    D = np.asarray(D, np.float64)
    P = D[..., None] * (np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(K0).T)
    q = (P @ Rr.T + tr) @ Kv.T
    with np.errstate(all="ignore"):
        c = np.floor(q[..., 0] / q[..., 2] + 0.5)
        r = np.floor(q[..., 1] / q[..., 2] + 0.5)
        inside = (q[..., 2] > 0) & (c >= 0) & (c <= w - 1) & (r >= 0) & (r <= h - 1)
        Dv = np.where(inside, depth_v[np.where(inside, r, 0).astype(int), np.where(inside, c, 0).astype(int)], 0.0).astype(np.float64)
        Q = Dv[..., None] * (np.stack([c, r, np.ones_like(c)], -1) @ np.linalg.inv(Kv).T)
        Pb = ((Q - tr) @ Rr) @ K0.T
        e = np.hypot(Pb[..., 0] / Pb[..., 2] - x, Pb[..., 1] / Pb[..., 2] - y)
        ok = inside & (Dv > 0) & (Pb[..., 2] > 0) & np.isfinite(e)
    return np.where(ok, np.minimum(e, clip), clip)


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(96, 72, 3, seed=31, all_gt=True)


def _grid(sc):
    h, w = sc.gt_depth.shape
    y, x = np.mgrid[0:h, 0:w]
    return x, y


@pytest.mark.parametrize("v", [1, 2])
def test_restatement_equals_the_float64_closed_form_on_ground_truth(scene, v):
    sc = scene
    x, y = _grid(sc)
    D = sc.gt_depth.numpy().astype(F32)
    dv = sc.meta["gt_all"][v][0].numpy().astype(F32)
    F, B = (m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, v))
    e32 = geom_term(F, B, dv, x, y, D, 1.0, 3.0)
    e64 = closed_form64(sc.K, sc.R, sc.t, v, dv, x, y, D, 3.0)
    seen = (e64 < 3.0)                                  # pixels whose point lands on the source image with an estimate there
    assert seen.mean() > 0.6
    # step 3 takes the NEAREST source pixel, so even on the true depths the way back lands off (x, y) by the rounding of the
    # projection (at most half a source pixel per axis, carried back through the local warp): what ground truth gives is that
    # bound, not zero.  The float32 sequence must give the float64 closed form's e within 1e-3 px
    assert np.median(e64[seen]) < 0.5 and (e64[seen] < 0.75).mean() > 0.95
    both = seen & (e32 < 3.0)
    assert both.mean() > 0.6
    assert np.abs(e32[both].astype(np.float64) - e64[both]).max() < 1e-3
    assert ((e32 >= 3.0) == (e64 >= 3.0)).mean() > 0.995
    # and where the projection lands on a pixel centre (no rounding), the true depth returns to (x, y): sampled by moving each
    # reference pixel's point to the centre of its nearest source pixel along the true surface of view v
    K0, Kv, Rr, tr = relative_pose(sc.K, sc.R, sc.t, v)
    h, w = dv.shape
    rr, cc = np.mgrid[8:h - 8:7, 8:w - 8:7]
    Q = dv[rr, cc].astype(np.float64)[..., None] * (np.stack([cc, rr, np.ones_like(cc)], -1).astype(np.float64) @ np.linalg.inv(Kv).T)
    Pr = ((Q - tr) @ Rr) @ K0.T
    xr, yr, Dr = Pr[..., 0] / Pr[..., 2], Pr[..., 1] / Pr[..., 2], Pr[..., 2]
    # (a fractional reference position: the closed form at that point, with the term's own arithmetic in float64)
    q = ((Dr[..., None] * (np.stack([xr, yr, np.ones_like(xr)], -1) @ np.linalg.inv(K0).T)) @ Rr.T + tr) @ Kv.T
    assert np.abs(q[..., 0] / q[..., 2] - cc).max() < 1e-4 and np.abs(q[..., 1] / q[..., 2] - rr).max() < 1e-4     # (float32 depths)


def test_exact_pixel_centres_give_zero_error():
    """The intent of a "ground truth gives e ~ 0" bar without the nearest-pixel rounding: a fronto-parallel plane at depth Z seen by a
    source camera moved along x so that the disparity f t / Z is exactly 3 px.  Every reference pixel then lands on a source pixel
    centre, the source depth there is Z, and the float32 term must return to (x, y) within 1e-3 px (the float64 closed form: 0)."""
    w, h, f, Z = 80, 60, 100.0, 5.0
    K = np.array([[f, 0, 40.0], [0, f, 30.0], [0, 0, 1]])
    R = np.stack([np.eye(3), np.eye(3)])
    t = np.array([[0.0, 0, 0], [-3.0 * Z / f, 0, 0]])             # x_v = x + f t_x / Z = x - 3 ... (t = -0.15: x_v = x - 3)
    Ks = np.stack([K, K])
    F, B = (m.astype(F32) for m in matrices64(Ks, R, t, 1))
    y, x = np.mgrid[0:h, 0:w]
    D = np.full((h, w), Z, F32)
    dv = np.full((h, w), Z, F32)
    e32 = geom_term(F, B, dv, x, y, D, 1.0, 3.0)
    e64 = closed_form64(Ks, R, t, 1, dv, x, y, D, 3.0)
    inner = x >= 3                                                   # (x - 3 >= 0: inside view 1)
    assert np.all(e64[inner] < 1e-9)
    assert np.all(e32[inner] < 1e-3)
    assert np.all(e32[~inner] == F32(3.0))


def test_the_term_is_tau_where_the_chain_breaks(scene):
    sc = scene
    h, w = sc.gt_depth.shape
    F, B = (m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, 1))
    dv = sc.meta["gt_all"][1][0].numpy().astype(F32)
    x, y = _grid(sc)
    D = sc.gt_depth.numpy().astype(F32)
    zero = np.zeros_like(dv)
    assert np.all(geom_term(F, B, zero, x, y, D, 1.0, 3.0) == F32(3.0))            # no estimate anywhere
    assert np.all(geom_term(F, B, dv, x, y, -D, 1.0, 3.0) == F32(3.0))             # behind the camera
    assert np.all(geom_term(F, B, dv, x, y, np.full_like(D, np.nan), 1.0, 3.0) == F32(3.0))
    far = np.full((1,), 1e6, F32)                                                   # lands outside the source image
    assert geom_term(F, B, dv, np.array([-100000]), np.array([0]), far, 0.5, 2.0)[0] == F32(1.0)
    # the weight scales, the clip bounds
    g = geom_term(F, B, dv * F32(1.1), x, y, D, 0.25, 3.0)
    assert g.max() <= F32(0.75) and g.min() >= 0


def test_matrices_are_inverse_of_each_other(scene):
    sc = scene
    for v in (1, 2):
        F, B = matrices64(sc.K, sc.R, sc.t, v)
        Fh = np.vstack([F, [0, 0, 0, 1]])
        Bh = np.vstack([B, [0, 0, 0, 1]])
        K0, Kv, _, _ = relative_pose(sc.K, sc.R, sc.t, v)
        # F takes (x D, y D, D, 1) to (c s, r s, s); B takes (c D_v, r D_v, D_v, 1) back: on a consistent depth the two compose to
        # the identity on the homogeneous point
        p = np.array([10.0 * 2.5, 20.0 * 2.5, 2.5, 1.0])
        q = Fh @ p
        assert np.allclose((Bh @ q)[:3], p[:3], rtol=1e-6, atol=1e-6)     # (R^T stands for R^-1: the cameras are float32)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_geom_sweep_kernels_keep_the_register_budget(tmp_path):
    """The sweep kernels with the term (variant bit 24) fit the 128 VGPRs of four waves per SIMD without scratch, like the others
    (tests/test_isa_guards.py), in the rolled and the packed form."""
    out = tmp_path / "pm_sweep.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "pm_sweep.hip"), str(out)], check=True,
                   capture_output=True, timeout=1200)
    txt = out.read_text()
    seen = {0: 0, 1: 0}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        mv = re.search(r"pm_sweep_kernelILi(\d+)ELi5ELb[01]ELb1ELi(\d+)ELi(?:128|256)ELb([01])E", name)
        if not mv or not (int(mv.group(2)) & (1 << 24)) or int(mv.group(1)) > 4:
            continue
        seen[int(mv.group(3))] += 1
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs"
    assert seen[0] >= 8 and seen[1] >= 8, seen

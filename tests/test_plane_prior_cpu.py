"""The plane-prior term of include/tsar.h (tsar_set_plane_prior) restated in numpy float32, one operation per operator of the header's
text, checked against a float64 closed form; and the register budget of the kernels that carry it.  test_gpu_plane_prior.py holds
the kernels to this restatement bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MAXCOST = F32(2.0)


def default_params():
    """(weight_depth, weight_normal, depth_clip, normal_clip) as tsar_default_plane_prior_params fills them"""
    return F32(0.1), F32(0.05), F32(0.02), F32(1.0 - np.cos(np.deg2rad(30.0)))


def plane_prior_term(prior, n4, D, weight_depth, weight_normal, depth_clip, normal_clip):
    """t of the header for hypotheses n4 [..., 4] of depth D [...] against the held prior [..., 4] = (q, Dp); 0 where the pixel has
    no prior (Dp == 0: the held entry is all zero there).  Every line is one float32 operation per operator."""
    prior, n4, D = np.asarray(prior, F32), np.asarray(n4, F32), np.asarray(D, F32)
    wd, wn, dc, nc = F32(weight_depth), F32(weight_normal), F32(depth_clip), F32(normal_clip)
    qx, qy, qz, Dp = prior[..., 0], prior[..., 1], prior[..., 2], prior[..., 3]
    with np.errstate(all="ignore"):
        a = np.abs(D - Dp)
        rel = a / Dp
        r_d = np.where(rel < dc, rel / dc, F32(1))
        s = F32(1) - ((n4[..., 0] * qx + n4[..., 1] * qy) + n4[..., 2] * qz)
        s0 = np.where(s < F32(0), F32(0), s)
        r_n = np.where(s < nc, s0 / nc, F32(1))
        t = (wd * r_d) + (wn * r_n)
    assert t.dtype == F32
    return np.where(Dp > F32(0), t, F32(0)).astype(F32)


def add_plane_prior(cost, beview, prior, n4, D, params):
    """the cost with the term: c + t where a view was valid (best view >= 0) and the pixel has a prior, else c"""
    cost = np.asarray(cost, F32)
    t = plane_prior_term(prior, n4, D, *params)
    has = (np.asarray(beview) >= 0) & (np.asarray(prior, F32)[..., 3] > F32(0))
    return np.where(has, cost + t, cost).astype(F32)


def hold_prior(depth, normal_cam):
    """the entry the context holds for a prior of `depth` and a normal ALREADY in reference-camera coordinates"""
    depth, normal_cam = np.asarray(depth, F32), np.asarray(normal_cam, F32)
    has = (depth > 0) & (depth < np.inf) & np.isfinite(normal_cam).all(-1)
    out = np.zeros(depth.shape + (4,), F32)
    out[has, :3] = normal_cam[has]
    out[has, 3] = depth[has]
    return out


def _closed_form(q, Dp, n, D, wd, wn, dc, nc):
    rel = abs(D - Dp) / Dp
    s = 1.0 - float(np.dot(n, q))
    r_d = rel / dc if rel < dc else 1.0
    r_n = max(s, 0.0) / nc if s < nc else 1.0
    return wd * r_d + wn * r_n


def _rot_x(n, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([n[0], c * n[1] - s * n[2], s * n[1] + c * n[2]])


def test_term_against_the_float64_closed_form():
    wd, wn, dc, nc = default_params()
    p64 = tuple(float(v) for v in (wd, wn, dc, nc))
    Dp = 5.0
    q = np.array([0.0, 0.0, -1.0])
    prior = hold_prior(np.array([Dp], F32), q[None].astype(F32))
    half_angle = np.arccos(1.0 - float(nc) / 2.0)                 # 1 - cos = half the clip
    cases = {
        "at the prior": (q, Dp),
        "half a clip in depth": (q, Dp * (1.0 + float(dc) / 2.0)),
        "half a clip in normal": (_rot_x(q, half_angle), Dp),
        "beyond both clips": (-q, Dp * 1.5),
        "nearer, inside the clip": (_rot_x(q, 0.1), Dp * 0.99),
    }
    for name, (n, D) in cases.items():
        n32 = n.astype(F32)
        n4 = np.array([[n32[0], n32[1], n32[2], 0.0]], F32)
        got = plane_prior_term(prior, n4, np.array([D], F32), wd, wn, dc, nc)[0]
        want = _closed_form(q, Dp, n32.astype(np.float64), float(F32(D)), *p64)
        # eight float32 operations on values <= 1, each within 2^-24 relative: 1e-6 of the largest term covers them
        assert abs(float(got) - want) <= 1e-6 * float(wd + wn), (name, got, want)
    at = plane_prior_term(prior, np.array([[0, 0, -1, 0]], F32), np.array([Dp], F32), wd, wn, dc, nc)[0]
    assert at == F32(0)
    beyond = plane_prior_term(prior, np.array([[0, 0, 1, 0]], F32), np.array([Dp * 1.5], F32), wd, wn, dc, nc)[0]
    assert beyond == wd + wn and beyond.dtype == F32              # exactly weight_depth + weight_normal
    half_d = plane_prior_term(prior, np.array([[0, 0, -1, 0]], F32), np.array([Dp * 1.01], F32), wd, wn, dc, nc)[0]
    assert abs(float(half_d) - 0.05) < 1e-5
    half_n = plane_prior_term(prior, np.append(_rot_x(q, half_angle), 0)[None].astype(F32), np.array([Dp], F32), wd, wn, dc, nc)[0]
    assert abs(float(half_n) - 0.025) < 1e-5


def test_nan_hypothesis_pays_both_weights_and_a_pixel_without_a_prior_pays_nothing():
    wd, wn, dc, nc = default_params()
    prior = hold_prior(np.array([5.0], F32), np.array([[0, 0, -1]], F32))
    nan4 = np.full((1, 4), np.nan, F32)
    t = plane_prior_term(prior, nan4, np.array([np.nan], F32), wd, wn, dc, nc)[0]
    assert t == wd + wn                                           # NaN fails both comparisons: both ratios are 1
    t = plane_prior_term(prior, np.array([[0, 0, -1, 0]], F32), np.array([np.nan], F32), wd, wn, dc, nc)[0]
    assert t == wd                                                # NaN depth alone: the depth ratio is 1, the normal's 0
    # pixels without a prior: depth 0, negative, inf, NaN, or a normal that is not finite
    depth = np.array([0.0, -1.0, np.inf, np.nan, 5.0, 5.0], F32)
    normal = np.array([[0, 0, -1]] * 4 + [[np.nan, 0, -1], [0, np.inf, -1]], F32)
    held = hold_prior(depth, normal)
    assert not held.any()
    n4 = np.tile(np.array([[0, 0, 1, 0]], F32), (6, 1))
    D = np.full(6, 9.0, F32)
    assert not plane_prior_term(held, n4, D, wd, wn, dc, nc).any()
    c = np.full(6, 0.25, F32)
    out = add_plane_prior(c, np.ones(6, np.int32), held, n4, D, (wd, wn, dc, nc))
    assert np.array_equal(out.view(np.uint32), c.view(np.uint32))
    # an invalid hypothesis (no valid view: MAXCOST, best view -1) keeps its cost where there is a prior
    out = add_plane_prior(np.array([MAXCOST, 0.25], F32), np.array([-1, 1]), np.tile(prior, (2, 1)), n4[:2], D[:2], (wd, wn, dc, nc))
    assert out[0] == MAXCOST and out[1] == F32(0.25) + (wd + wn)


def test_both_weights_zero_add_zero():
    _, _, dc, nc = default_params()
    prior = hold_prior(np.array([5.0] * 3, F32), np.array([[0, 0, -1]] * 3, F32))
    n4 = np.array([[0, 0, -1, 0], [0, 0, 1, 0], [np.nan] * 4], F32)
    D = np.array([5.0, 50.0, np.nan], F32)
    t = plane_prior_term(prior, n4, D, 0.0, 0.0, dc, nc)
    assert np.array_equal(t.view(np.uint32), np.zeros(3, np.uint32))   # +0 each: c + t is c, bit for bit


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_kernels_with_the_term_keep_the_register_budget(tmp_path):
    """The sweep kernels of variant bit 24, which now carry the plane-prior term beside the geometric one, still fit the 128 VGPRs of
    four waves per SIMD without scratch, in the rolled and the packed form (the method of
    test_geom_cpu.py::test_geom_sweep_kernels_keep_the_register_budget)."""
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

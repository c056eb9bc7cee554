#!/usr/bin/env python3
"""What a BUILT plane prior (include/tsar.h tsar_build_plane_prior) is worth, simulated on the CPU in strict arithmetic: the pipeline of
tests/test_gpu_plane_prior_build.py::test_built_prior_does_what_it_is_for.  Box 11, n_best 1, every view plus integer noise in {-1, 0, 1}
(default_rng(3), drawn in view order, clipped to 0..255), as in tools/plane_prior_oracle_bars.py:
  1. phase 1 on every view as reference (the C oracle: pm_init + 3 iterations, seed 77 + view), its depth and, for view 0, its cost;
  2. view 0's depth checked against the other views' phase-1 maps (tests/test_geom_check_cpu.py geom_check_ref, the defaults);
  3. the builder on the kept depths with view 0's phase-1 cost as the score (tests/test_plane_prior_build_cpu.py);
  4. view 0 rerun with the built prior at the default weights (plane_prior_oracle_bars.run: the rerun of the ground-truth prior).
--scene check (the default, the test's scene): make_scene(200, 144, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True), the scene of
test_check_does_what_it_is_for at a quarter of its size; --scene prior: make_scene(160, 120, 3, seed=65, textureless=True, all_gt=True,
step=0.2), the scene of test_prior_does_what_it_is_for, on which the check keeps too little for the built prior to cover 0.85 of the
constant-albedo pixels.
Printed: what the check keeps, what the prior covers, and per class the share of pixels within 1e-2 relative of ground truth for the
control (phase 1 of view 0) and the rerun; the bars of the GPU test are control + half the gain.

    python tools/plane_prior_build_oracle_bars.py [--scene check|prior] [--cell 4] [--iterations 3]

No GPU; about a minute."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import oracle_lib as ol                                               # noqa: E402
import plane_prior_oracle_bars as bars                                # noqa: E402
from test_geom_check_cpu import geom_check_ref                        # noqa: E402
from test_geom_cpu import matrices64                                  # noqa: E402
from test_plane_prior_build_cpu import build_plane_prior_ref          # noqa: E402
from test_plane_prior_cpu import default_params                       # noqa: E402
from tsar_mvs_amd import synth                                        # noqa: E402

F32 = np.float32


def noisy_scene(kind="prior"):
    """kind "prior": the scene of test_prior_does_what_it_is_for; "check": the scene of test_check_does_what_it_is_for at a quarter of
    its size (200 x 144); both with the same integer noise"""
    if kind == "prior":
        sc = synth.make_scene(160, 120, 3, seed=65, textureless=True, all_gt=True, step=0.2)
    else:
        sc = synth.make_scene(200, 144, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True)
    rng = np.random.default_rng(3)
    imgs = []
    for im in sc.images:                                              # in view order
        v = im.numpy().astype(np.int64)
        imgs.append(np.clip(v + rng.integers(-1, 2, v.shape), 0, 255).astype(F32))
    return sc, imgs


def phase1(sc, imgs, k, iterations):
    """(depth, cost) of view k as reference, the other views in their order as its sources"""
    order = [k] + [v for v in range(len(imgs)) if v != k]
    orc = ol.Oracle([imgs[v] for v in order], sc.K[order], sc.R[order], sc.t[order], sc.depth_min, sc.depth_max, box=11, n_best=1, seed=bars.SEED + k)
    orc.pm_init()
    orc.pm_iterate(iterations)
    cost = orc.c.copy()
    return orc.compute_disp()[..., 3].copy(), cost


def normal_to_camera(normal_world, R):
    """tsar_set_plane_prior's conversion: float32, (R[r][0] n_0 + R[r][1] n_1) + R[r][2] n_2"""
    R = np.asarray(R, F32)
    n = np.asarray(normal_world, F32)
    return np.stack([(R[r, 0] * n[..., 0] + R[r, 1] * n[..., 1]) + R[r, 2] * n[..., 2] for r in range(3)], -1).astype(F32)


def shares(D, gt, tex):
    ok = np.abs(D - gt) <= F32(1e-2) * gt
    return round(float(ok[tex].mean()), 4), round(float(ok[~tex].mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--scene", choices=("prior", "check"), default="check")
    a = ap.parse_args()
    t0 = time.time()
    sc, imgs = noisy_scene(a.scene)
    gt = sc.gt_depth.numpy().astype(F32)
    tex = sc.textured.numpy()
    n = len(imgs)
    first = [phase1(sc, imgs, k, a.iterations) for k in range(n)]
    depth0, cost0 = first[0]
    FB = [tuple(m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, v)) for v in range(n)]
    maps = [None] + [first[v][0] for v in range(1, n)]
    count, kept, mask = geom_check_ref([fb[0] for fb in FB], [fb[1] for fb in FB], maps, depth0, (2.0, 0.01, 2))
    keep = mask == 1
    good = np.abs(depth0 - gt) <= F32(1e-2) * gt
    print(json.dumps({"step": "check", "scene": a.scene, "size": [sc.w, sc.h], "constant_albedo_share": round(float((~tex).mean()), 4),
                      "kept": round(float(keep.mean()), 4), "kept_textured": round(float(keep[tex].mean()), 4),
                      "kept_constant_albedo": round(float(keep[~tex].mean()), 4), "kept_within_1e-2": round(float(good[keep].mean()), 4),
                      "seconds": round(time.time() - t0)}), flush=True)
    d, nw, lv = build_plane_prior_ref(kept, cost0, sc.K[0], sc.R[0], a.cell)
    has = lv != 255
    pgood = np.abs(d - gt) <= F32(1e-2) * gt
    print(json.dumps({"step": "build", "cell": a.cell, "covered": round(float(has.mean()), 4), "covered_textured": round(float(has[tex].mean()), 4),
                      "covered_constant_albedo": round(float(has[~tex].mean()), 4), "levels": sorted(int(v) for v in np.unique(lv)),
                      "prior_within_1e-2_textured": round(float(pgood[tex & has].mean()), 4),
                      "prior_within_1e-2_constant_albedo": round(float(pgood[~tex & has].mean()), 4)}), flush=True)
    c_tex, c_flat = shares(depth0, gt, tex)
    D = bars.run(sc, imgs, (d, normal_to_camera(nw, sc.R[0])), default_params(), a.iterations)
    b_tex, b_flat = shares(D, gt, tex)
    print(json.dumps({"step": "rerun", "control_textured": c_tex, "control_constant_albedo": c_flat, "built_textured": b_tex,
                      "built_constant_albedo": b_flat, "bar_textured_gain": round((b_tex - c_tex) / 2, 4),
                      "bar_constant_albedo_gain": round((b_flat - c_flat) / 2, 4), "seconds": round(time.time() - t0)}), flush=True)


if __name__ == "__main__":
    main()

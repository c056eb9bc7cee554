#!/usr/bin/env python3
"""What the plane-prior term (include/tsar.h tsar_set_plane_prior) is worth, simulated on the CPU in strict arithmetic: the sweep is
half_sweep of tests/test_oracle_independent_sweep.py with the C oracle as scorer and the term added in float32 on top of its multi-view
cost (tests/test_plane_prior_cpu.py states the term).  The set-up is that of
tests/test_gpu_plane_prior.py::test_prior_does_what_it_is_for: make_scene(160, 120, 3, seed=65, textureless=True, all_gt=True,
step=0.2), every view plus integer noise in {-1, 0, 1} (default_rng(3), drawn in view order, clipped to 0..255) so that constant-albedo
windows have a valid but uninformative cost, box 11, n_best 1, seed 77; pm_init, the initial costs rescored with the term, 3 iterations.
Printed per prior: the share of textured and of constant-albedo pixels whose plane's depth is within 1e-2 relative of ground truth.

    python tools/plane_prior_oracle_bars.py [--iterations 3] [--only NAME]

No GPU; a few minutes per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle_lib as ol                                               # noqa: E402
from test_oracle_independent_sweep import _Cam, half_sweep            # noqa: E402
from test_plane_prior_cpu import add_plane_prior, default_params, hold_prior, plane_prior_term   # noqa: E402
from tsar_mvs_amd import synth                                        # noqa: E402

F32 = np.float32
SEED = 77


class PriorScorer:
    """the oracle with the term added to pm_cost_multiview: everything else half_sweep reads is the oracle's own"""

    def __init__(self, orc, held, params):
        self._orc, self._held = orc, held
        self._wd, self._wn, self._dc, self._nc = (F32(v) for v in params)

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def term(self, x, y, n4):
        """plane_prior_term for one hypothesis, on float32 scalars (the same operations in the same order)"""
        q = self._held[y, x]
        Dp = q[3]
        if not Dp > 0:
            return None
        one, zero = F32(1), F32(0)
        with np.errstate(all="ignore"):
            D = F32(self._orc.depth_from_plane(n4, x, y))
            rel = abs(D - Dp) / Dp
            r_d = rel / self._dc if rel < self._dc else one
            s = one - ((n4[0] * q[0] + n4[1] * q[1]) + n4[2] * q[2])
            s0 = zero if s < zero else s
            r_n = s0 / self._nc if s < self._nc else one
            return (self._wd * r_d) + (self._wn * r_n)

    def pm_cost_multiview(self, x, y, n4):
        c, bv, rt = self._orc.pm_cost_multiview(x, y, n4)
        if bv >= 0 and self._held is not None:
            t = self.term(x, y, np.asarray(n4, F32))
            if t is not None:
                c = float(F32(c) + t)
        return c, bv, rt


def run(sc, imgs, prior, params, iterations):
    orc = ol.Oracle(imgs, sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=SEED)
    cam = _Cam(orc.camera(0))
    held = None
    if prior is not None:
        depth, normal_cam = prior
        held = hold_prior(depth, normal_cam)
    orc.pm_init()
    scorer = PriorScorer(orc, held, params)
    if held is not None:
        # the initial costs rescored with the term (odd box: tsar_pm_init scores on the sweeps' window)
        planes = orc.norm4.copy()
        c, bv, _ = orc.pm_cost_planes(planes)
        assert np.array_equal(c.view(np.uint32), orc.c.view(np.uint32))
        D = np.array([[orc.depth_from_plane(planes[y, x], x, y) for x in range(orc.w)] for y in range(orc.h)], F32)
        orc.c[:] = add_plane_prior(c, bv, held, planes, D, params)
        # the scalar form used inside the sweep is the array form, bit for bit
        for y in range(0, orc.h, 7):
            for x in range(0, orc.w, 5):
                t = scorer.term(x, y, planes[y, x])
                ta = plane_prior_term(held[y, x][None], planes[y, x][None], D[y, x][None], *params)[0]
                assert (t is None and held[y, x, 3] == 0) or F32(t).view(np.uint32) == ta.view(np.uint32)
    launch = 0
    for _ in range(iterations):
        for colour in (0, 1):
            c1, n1, r1, b1 = half_sweep(scorer, cam, colour, stream=1 + launch, seed=SEED)
            orc.c[:], orc.norm4[:], orc.ratio[:], orc.beview[:] = c1, n1, r1, b1
            launch += 1
    planes = orc.norm4
    return np.array([[orc.depth_from_plane(planes[y, x], x, y) for x in range(orc.w)] for y in range(orc.h)], F32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--only", default=None, help="run one row: control, gt, wrong or wrong_heavy")
    a = ap.parse_args()
    sc = synth.make_scene(160, 120, 3, seed=65, textureless=True, all_gt=True, step=0.2)
    rng = np.random.default_rng(3)
    imgs = []
    for im in sc.images:                                              # in view order
        v = im.numpy().astype(np.int64)
        imgs.append(np.clip(v + rng.integers(-1, 2, v.shape), 0, 255).astype(F32))
    gt = sc.gt_depth.numpy().astype(F32)
    normal_cam = sc.gt_normal.numpy().astype(F32)
    tex = sc.textured.numpy()
    wd, wn, dc, nc = default_params()
    rows = {
        "control": (None, (wd, wn, dc, nc)),
        "gt": ((gt, normal_cam), (wd, wn, dc, nc)),
        "wrong": (((gt.astype(np.float64) * 1.1).astype(F32), normal_cam), (wd, wn, dc, nc)),
        "wrong_heavy": (((gt.astype(np.float64) * 1.1).astype(F32), normal_cam), (F32(0.3), F32(0.1), dc, nc)),
    }
    for name, (prior, params) in rows.items():
        if a.only and a.only != name:
            continue
        t0 = time.time()
        D = run(sc, imgs, prior, params, a.iterations)
        ok = np.abs(D - gt) <= F32(1e-2) * gt
        print(json.dumps({"prior": name, "weight_depth": float(params[0]), "weight_normal": float(params[1]), "depth_clip": float(params[2]),
                          "normal_clip": float(params[3]), "textured": round(float(ok[tex].mean()), 4),
                          "constant_albedo": round(float(ok[~tex].mean()), 4), "seconds": round(time.time() - t0)}), flush=True)


if __name__ == "__main__":
    main()

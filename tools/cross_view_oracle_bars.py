#!/usr/bin/env python3
"""The bars of tests/test_gpu_geom_reproject.py::test_cross_view_does_what_it_is_for from the CPU oracle in strict arithmetic (which the
strict kernels reproduce bit for bit): phase 1 (3 iterations) on every view of the textureless scene of test_check_does_what_it_is_for,
then phase 2 of view 0 (2 iterations) without the cross-view merge, with K = 1 and with K = 2, and the control again with another seed
(the run-to-run noise of reseeding).  The merge is the composition include/tsar.h states for tsar_pm_merge_depths: rescore, the candidate
through Oracle.getD, pm_cost_planes, a strict select.  No GPU.

    python tools/cross_view_oracle_bars.py [--halve N]      (N times halved: 800 x 576 -> 400 x 288 -> ...)

The matrices are the float64 geometry rounded once to float32 (the device's are within one ulp of them, test_gpu_geom.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle_lib as ol                                         # noqa: E402
from test_geom_check_cpu import scene_matrices                  # noqa: E402
from test_geom_reproject_cpu import reproject_ref               # noqa: E402
from tsar_mvs_amd import synth                                  # noqa: E402

F32 = np.float32


def reorder(sc, imgs, k):
    order = [k] + [v for v in range(len(imgs)) if v != k]
    return [imgs[v] for v in order], sc.K[order], sc.R[order], sc.t[order]


def merge(orc, depth):
    """tsar_pm_merge_depths on the oracle's state; returns (pixels taken, rescored cost)"""
    orc.rescore()
    P, Cst = orc.norm4.copy(), orc.c.copy()
    usable = np.isfinite(depth) & (depth >= F32(orc_dmin)) & (depth <= F32(orc_dmax))
    Q = P.copy()
    for y, x in zip(*np.nonzero(usable)):
        Q[y, x, 3] = orc.getD(P[y, x, :3], int(x), int(y), float(depth[y, x]))
    cq, bq, rq = orc.pm_cost_planes(Q)
    take = cq < Cst
    orc.norm4[take] = Q[take]
    orc.c[take] = cq[take]
    orc.beview[take] = bq[take]
    orc.ratio[take] = rq[take]
    return int(take.sum()), Cst


def main():
    global orc_dmin, orc_dmax
    ap = argparse.ArgumentParser()
    ap.add_argument("--halve", type=int, default=0)
    a = ap.parse_args()
    w, h = 800 >> a.halve, 576 >> a.halve
    sc = synth.make_scene(w, h, 3, seed=5, textureless=True, flat_cell=6.0, all_gt=True)
    orc_dmin, orc_dmax = sc.depth_min, sc.depth_max
    imgs = [im.numpy().astype(np.uint8).astype(F32) for im in sc.images]
    n = len(imgs)
    t0 = time.time()
    depth1, normal1 = [], []
    for k in range(n):
        iv, K, R, t = reorder(sc, imgs, k)
        o = ol.Oracle(iv, K, R, t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=41 + k)
        o.pm_init()
        o.pm_iterate(3)
        out = o.compute_disp()
        depth1.append(out[..., 3].copy())
        normal1.append(np.ascontiguousarray(out[..., :3]))
    print("phase 1: %.0f s" % (time.time() - t0), file=sys.stderr)
    F, B = scene_matrices(sc)
    maps = [None] + depth1[1:]
    gt = sc.gt_depth.numpy()
    tex = sc.textured.numpy()
    good = lambda D: np.abs(D - gt) / gt < 1e-2
    render2 = reproject_ref(B, maps, 0.01, 2)[0]
    recoverable = ~good(depth1[0]) & good(render2)
    groups = {"all": np.ones_like(tex), "textured": tex, "constant_albedo": ~tex, "recoverable": recoverable}
    print(json.dumps({"w": w, "h": h, "phase1": {k: float(good(depth1[0])[g].mean()) for k, g in groups.items()},
                      "share_recoverable": float(recoverable.mean()), "render2_coverage": float((render2 > 0).mean())}))
    for name, seed, K in (("control", 41, 0), ("K=1", 41, 1), ("K=2", 41, 2), ("control_reseeded", 43, 0)):
        o = ol.Oracle(imgs, sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=seed)
        o.load_planes(depth1[0], normal1[0])
        o.set_geom(maps, list(zip(F, B)), weight=0.2, clip=3.0)
        rec = {"run": name}
        if K:
            taken, rescored = merge(o, reproject_ref(B, maps, 0.01, K)[0])
            rec["n_taken"] = taken
            rec["share_taken"] = taken / float(w * h)
            rec["cost_not_above_rescored"] = bool(np.all(o.c <= rescored))
        else:
            o.rescore()
        o.pm_iterate(2)
        D = o.compute_disp()[..., 3]
        rec.update({k: float(good(D)[g].mean()) for k, g in groups.items()})
        print(json.dumps(rec), flush=True)
    print("total: %.0f s" % (time.time() - t0), file=sys.stderr)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/geom_multiscale_timing.py — what the geometric-consistency pass costs coarse to fine, and what it does, on one GPU.

At bench.py's scene size with textureless patches (6048 x 4032, ten sources, box 11, default arithmetic, the 8-bit decode), the view's
own converged photometric result (--iters iterations) as its phase-1 maps and the sources' ground-truth depth maps standing in for
theirs (as tools/geom_timing.py does), phase 2 of the reference view by api.run_geom_pass_multiscale at L = 0, 1, 2 with --fine
iterations at every level below the coarsest and --coarse iterations at the coarsest (L = 0: api.run_geom_pass with --fine).
Per L one JSON line: the wall time (after a warm-up run, kernel timing off), then from a third run with the library's kernel timers
the time of each stage
    geom_pyramid      tsar_geom_pyramid, every coarse level
    pyramid_planes    tsar_pyramid_planes: the plane copy plus the rescore, every coarse level (L = 0: the fine level's rescore)
    coarse_sweeps     pm_sweep_geom on every coarse level (with L = 2 the middle level's --fine iterations included)
    upsample_merge    tsar_upsample_merge, every level (and the full-size launch alone)
    fine_sweeps       pm_sweep_geom at full size
and the median relative depth error of the result on textured and on textureless pixels.

    timeout -k 10 900 python tools/geom_multiscale_timing.py [--width 6048 --height 4032 --views 10 --iters 8 --fine 2 --coarse 8]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tsar_mvs_amd import api, synth  # noqa: E402


def total(t, name):
    return t.get(name, (0, 0.0))[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--fine", type=int, default=2)
    ap.add_argument("--coarse", type=int, default=8)
    ap.add_argument("--levels", default="0,1,2")
    a = ap.parse_args()
    sc = synth.make_scene(a.width, a.height, a.views, device="cuda", seed=1234, all_gt=True, textureless=True)
    imgs = [im.to(torch.uint8).contiguous() for im in sc.images]
    maps = [None] + [g[0].float().contiguous() for g in sc.meta["gt_all"][1:]]
    gt = sc.gt_depth.cpu().numpy().astype(np.float64)
    textured = sc.textured.cpu().numpy()
    cfg = {"width": a.width, "height": a.height, "src_views": a.views, "box": 11, "mode": "fast", "fine_iterations": a.fine,
           "coarse_iterations": a.coarse}

    m = api.matcher_from_scene(sc, box=11, n_best=1, seed=5)
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.pm_init()
    m.pm_iterate(a.iters)
    m.compute_disp()
    r = m.get_result(("depth", "normal"))
    own_d, own_n = r["depth"].copy(), r["normal"].copy()
    rel = np.abs(own_d.astype(np.float64) - gt) / gt
    print(json.dumps({"what": "phase 1 (own result)", **cfg, "iterations": a.iters, "median_rel_err_textured": float(np.median(rel[textured])),
                      "median_rel_err_textureless": float(np.median(rel[~textured]))}))

    coarse = [api.Matcher(m.device) for _ in range(2)]
    for L in [int(x) for x in a.levels.split(",")]:
        chain = [m] + coarse[:L]

        def run():
            api.run_geom_pass_multiscale(m, own_d, own_n, maps, L, a.coarse, a.fine, coarse=coarse[:L])
            for c in chain:
                c.synchronize()

        run()                                            # warm-up (code objects loaded, coarse contexts allocated)
        for c in chain:
            c.enable_kernel_timing(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        wall = (time.perf_counter() - t0) * 1e3
        for c in chain:
            c.enable_kernel_timing(True)
            c.L.tsar_reset_kernel_timing(c._ctx)
        run()
        ts = [c.kernel_timing() for c in chain]
        for c in chain:
            c.enable_kernel_timing(False)
        d = m.get_result(("depth",))["depth"].astype(np.float64)
        rel = np.abs(d - gt) / gt
        stages = {
            "geom_pyramid": sum(total(t, "geom_pyramid") for t in ts[1:]),
            "pyramid_planes": sum(total(t, "pm_pyramid_planes") + total(t, "pm_rescore") for t in ts[1:]) if L else total(ts[0], "pm_rescore"),
            "coarse_sweeps": sum(total(t, "pm_sweep_geom") for t in ts[1:]),
            "upsample_merge": sum(total(t, "pm_upsample_merge") for t in ts),
            "upsample_merge_full_size": total(ts[0], "pm_upsample_merge"),
            "fine_sweeps": total(ts[0], "pm_sweep_geom"),
        }
        per_level = [{k: [n, round(ms, 3)] for k, (n, ms) in t.items()} for t in ts]
        print(json.dumps({"what": "phase 2 of one view", **cfg, "geom_multi_scale": L, "wall_ms": round(wall, 1),
                          "stage_ms": {k: round(v, 3) for k, v in stages.items()}, "median_rel_err_textured": float(np.median(rel[textured])),
                          "median_rel_err_textureless": float(np.median(rel[~textured])), "kernels_per_level": per_level}))
    for c in coarse + [m]:
        c.close()


if __name__ == "__main__":
    main()

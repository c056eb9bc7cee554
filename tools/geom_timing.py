#!/usr/bin/env python3
"""tools/geom_timing.py — what the geometric-consistency pass costs, on one GPU.

At bench.py's scene (6048 x 4032, ten sources, box 11, default arithmetic, the 8-bit decode), with the sources' ground-truth depth
maps standing in for their phase-1 maps (the term's arithmetic and memory pattern do not depend on where the maps came from):
    sweep      one iteration (two launches, rolled form) from the converged photometric state: photometric vs with the term
    rescore    tsar_pm_rescore of the converged planes under the term
    pass N     api.run_geom_pass per view (load planes, install the ten maps from device memory, rescore, N iterations, compute_disp),
               wall time after a warm-up, for N = 1, 2, 4
One JSON line per measurement.

    timeout -k 10 900 python tools/geom_timing.py [--width 6048 --height 4032 --views 10 --iters 8 --passes 1,2,4]
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


def per_launch(t, name):
    n, ms = t.get(name, (0, 0.0))
    return (ms / n if n else None), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--passes", default="1,2,4")
    a = ap.parse_args()
    sc = synth.make_scene(a.width, a.height, a.views, device="cuda", seed=1234, all_gt=True)
    imgs = [im.to(torch.uint8).contiguous() for im in sc.images]
    maps = [None] + [g[0].float().contiguous() for g in sc.meta["gt_all"][1:]]
    cfg = {"width": a.width, "height": a.height, "src_views": a.views, "box": 11, "mode": "fast"}

    m = api.matcher_from_scene(sc, box=11, n_best=1, seed=5)
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.pm_init()
    m.pm_iterate(a.iters)
    m.compute_disp()
    r = m.get_result(("depth", "normal"))
    own_d, own_n = r["depth"].copy(), r["normal"].copy()
    planes, cost, _, _ = m.get_plane()

    # one iteration from the converged state, photometric and with the term (same planes, same sweep counter)
    m.enable_kernel_timing(True)
    for rep in range(2):                               # (the second repetition is reported: code objects loaded)
        m.L.tsar_reset_kernel_timing(m._ctx)
        m.clear_geom()
        m.set_plane(planes, cost)
        m.rescore()
        m.set_sweep_counter(2 * a.iters)              # (after rescore, which restarts the counter: the converged launches' form)
        m.pm_iterate(1)
        tp = m.kernel_timing()
        m.L.tsar_reset_kernel_timing(m._ctx)
        m.set_plane(planes, cost)
        m.set_geom_depths(maps)
        m.rescore()
        m.set_sweep_counter(2 * a.iters)
        m.pm_iterate(1)
        tg = m.kernel_timing()
        m.L.tsar_reset_kernel_timing(m._ctx)
    photo, n_p = per_launch(tp, "pm_sweep")
    geom, n_g = per_launch(tg, "pm_sweep_geom")
    resc_p, _ = per_launch(tp, "pm_rescore")
    resc_g, _ = per_launch(tg, "pm_rescore")
    print(json.dumps({"what": "sweep launch from the converged state", **cfg, "photometric_ms": photo, "geom_ms": geom, "launches": [n_p, n_g],
                      "increase": (geom / photo - 1.0) if photo and geom else None}))
    print(json.dumps({"what": "rescore", **cfg, "rescore_geom_ms": resc_g, "rescore_photometric_ms": resc_p}))

    m.enable_kernel_timing(False)
    for N in [int(x) for x in a.passes.split(",")]:
        walls = []
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.run_geom_pass(m, own_d, own_n, maps, N)
            m.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            m.clear_geom()
        m.enable_kernel_timing(True)
        m.L.tsar_reset_kernel_timing(m._ctx)
        api.run_geom_pass(m, own_d, own_n, maps, N)
        k = {name: round(ms, 3) for name, (n, ms) in m.kernel_timing().items()}
        m.clear_geom()
        m.enable_kernel_timing(False)
        print(json.dumps({"what": "phase 2 per view", **cfg, "geom_iterations": N, "wall_ms": round(walls[-1], 1), "kernel_ms_total": k}))
    m.close()


if __name__ == "__main__":
    main()

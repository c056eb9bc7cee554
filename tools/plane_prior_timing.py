#!/usr/bin/env python3
"""tools/plane_prior_timing.py — what the plane-prior term costs, on one GPU.

At bench.py's scene (6048 x 4032, ten sources, box 11, default arithmetic, the 8-bit decode), with the sources' ground-truth depth
maps as the geometric term's maps and the reference view's ground truth as the prior (the term's arithmetic and memory pattern do
not depend on where the prior came from):
    sweep      one iteration (two launches, rolled form) from the converged photometric state under the geometric term: without
               and with a prior (both run the variant-bit-24 kernels, timed as "pm_sweep_geom")
    rescore    tsar_pm_rescore of the converged planes, without and with a prior
    prior only the same two with a prior and no geometric term (the same kernels, every map null)
    set        tsar_set_plane_prior itself: wall time from host arrays and from device tensors, and its kernel ("plane_prior")
One JSON line per measurement.

    timeout -k 10 900 python tools/plane_prior_timing.py [--width 6048 --height 4032 --views 10 --iters 8]
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
    a = ap.parse_args()
    sc = synth.make_scene(a.width, a.height, a.views, device="cuda", seed=1234, all_gt=True)
    imgs = [im.to(torch.uint8).contiguous() for im in sc.images]
    maps = [None] + [g[0].float().contiguous() for g in sc.meta["gt_all"][1:]]
    prior_d = sc.gt_depth.float().contiguous()
    R0 = torch.as_tensor(np.asarray(sc.R[0], np.float32), device=prior_d.device)
    prior_n = (sc.gt_normal.float() @ R0).contiguous()                 # camera -> world: R^T n
    cfg = {"width": a.width, "height": a.height, "src_views": a.views, "box": 11, "mode": "fast"}

    m = api.matcher_from_scene(sc, box=11, n_best=1, seed=5)
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.pm_init()
    m.pm_iterate(a.iters)
    planes, cost, _, _ = m.get_plane()

    def one_iteration(with_maps, with_prior):
        """rescore + one iteration from the converged state; (sweep ms per launch, launches, rescore ms)"""
        m.L.tsar_reset_kernel_timing(m._ctx)
        m.clear_geom()
        m.clear_plane_prior()
        m.set_plane(planes, cost)
        if with_maps:
            m.set_geom_depths(maps)
        if with_prior:
            m.set_plane_prior(prior_d, prior_n)
        m.rescore()
        m.set_sweep_counter(2 * a.iters)              # (after rescore, which restarts the counter: the converged launches' form)
        m.pm_iterate(1)
        t = m.kernel_timing()
        sweep, n = per_launch(t, "pm_sweep_geom" if (with_maps or with_prior) else "pm_sweep")
        return sweep, n, per_launch(t, "pm_rescore")[0]

    m.enable_kernel_timing(True)
    res = {}
    for rep in range(2):                               # (the second repetition is reported: code objects loaded)
        for key, wm, wp in (("photometric", False, False), ("geom", True, False), ("geom_prior", True, True), ("prior_only", False, True)):
            res[key] = one_iteration(wm, wp)
    g, gp, po, ph = res["geom"], res["geom_prior"], res["prior_only"], res["photometric"]
    print(json.dumps({"what": "sweep launch from the converged state", **cfg, "photometric_ms": ph[0], "geom_ms": g[0], "geom_prior_ms": gp[0],
                      "prior_only_ms": po[0], "launches": [ph[1], g[1], gp[1], po[1]],
                      "prior_over_geom": (gp[0] / g[0] - 1.0) if g[0] and gp[0] else None}))
    print(json.dumps({"what": "rescore", **cfg, "rescore_photometric_ms": ph[2], "rescore_geom_ms": g[2], "rescore_geom_prior_ms": gp[2],
                      "rescore_prior_only_ms": po[2]}))

    # tsar_set_plane_prior itself
    m.clear_geom()
    host_d, host_n = prior_d.cpu().numpy(), prior_n.cpu().numpy()
    walls = {}
    for name, d, n in (("device", prior_d, prior_n), ("host", host_d, host_n)):
        for rep in range(2):
            m.L.tsar_reset_kernel_timing(m._ctx)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.set_plane_prior(d, n)
            walls[name] = (time.perf_counter() - t0) * 1e3
    kern, _ = per_launch(m.kernel_timing(), "plane_prior")
    print(json.dumps({"what": "tsar_set_plane_prior", **cfg, "wall_ms_device_tensors": round(walls["device"], 2),
                      "wall_ms_host_arrays": round(walls["host"], 2), "kernel_ms": kern}))
    m.close()


if __name__ == "__main__":
    main()

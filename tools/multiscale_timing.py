#!/usr/bin/env python3
"""tools/multiscale_timing.py — wall time and per-stage kernel time of coarse-to-fine PatchMatch against single scale, on one GPU.

At bench.py's scene (6048 x 4032, ten sources, box 11, default arithmetic), on the 8-bit decode (tsar_set_views_u8, what tsar_gipuma
hands over):
    single scale          init + ITERS iterations
    --multi_scale=L       pyramid, init + COARSE iterations at the coarsest level, upsample + FINE iterations per finer level
Stages: pyramid (tsar_pyramid_views, which includes the coarse views' quad textures), coarse sweeps (init + iterations of every coarse
level), upsample (pm_upsample), fine sweeps (iterations at the full level).  Each configuration runs twice; the second run is reported
(code objects loaded, coarse contexts reused as tsar_gipuma --all reuses them).  One JSON line per configuration.

    timeout -k 10 600 python tools/multiscale_timing.py [--width 6048 --height 4032 --views 10 --iters 8 --coarse 8 --fine 2,3,4]
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


def kernel_ms(ms):
    out = {}
    for m in ms:
        for name, (n, t) in m.kernel_timing().items():
            out[name] = out.get(name, 0.0) + t
    return out


def run(m, coarse, levels, iters, coarse_iters, fine_iters):
    for c in [m, *coarse]:
        c.reset_kernel_timing()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stages = {}
    if levels == 0:
        m.pm_init()
        m.pm_iterate(iters)
    else:
        chain = [m] + coarse[:levels]
        for finer, c in zip(chain[:-1], chain[1:]):
            c.pyramid_from(finer)
        t1 = time.perf_counter()
        chain[-1].pm_init()
        chain[-1].pm_iterate(coarse_iters)
        for k in range(levels - 1, -1, -1):
            chain[k].upsample_planes(chain[k + 1])
            chain[k].pm_iterate(fine_iters)
        km_c = kernel_ms(chain[1:])
        km_f = kernel_ms([m])
        stages["pyramid_ms"] = sum(v for k, v in km_c.items() if k in ("pyr_down", "expand_u8", "build_quad", "build_dquad"))
        stages["pyramid_wall_ms"] = (t1 - t0) * 1e3
        # (pm_sweep brackets every sweep launch; pm_sweep_packed is nested inside it)
        stages["coarse_sweeps_ms"] = km_c.get("pm_init", 0.0) + km_c.get("pm_sweep", 0.0)
        stages["upsample_ms"] = km_f.get("pm_upsample", 0.0) + km_c.get("pm_upsample", 0.0)
        stages["fine_sweeps_ms"] = km_f.get("pm_sweep", 0.0)
        stages["kernels"] = {"coarse": km_c, "fine": km_f}
    m.compute_disp()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    if levels == 0:
        km = kernel_ms([m])
        stages["fine_sweeps_ms"] = km.get("pm_sweep", 0.0)
        stages["init_ms"] = km.get("pm_init", 0.0)
        stages["kernels"] = {"fine": km}
    return wall, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--box", type=int, default=11)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--coarse", type=int, default=8)
    ap.add_argument("--fine", default="2,3,4")
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    sc = synth.make_scene(args.width, args.height, args.views, device="cuda", seed=1234, textureless=True)
    imgs = [im.to(torch.uint8).cpu().numpy() for im in sc.images]
    gt = sc.gt_depth.cpu().numpy()
    flat = ~sc.textured.cpu().numpy()
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=args.box, box_vsize=args.box, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, seed=2024))
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.enable_kernel_timing(True)
    coarse = [api.Matcher() for _ in range(max(int(x) for x in args.levels.split(",")))]
    for c in coarse:
        c.enable_kernel_timing(True)
    configs = [(0, args.iters, 0, 0)] + [(int(L), 0, args.coarse, int(f)) for L in args.levels.split(",") for f in args.fine.split(",")]
    lines = []
    for levels, iters, ci, fi in configs:
        for rep in range(2):
            wall, stages = run(m, coarse, levels, iters, ci, fi)
        depth = m.get_result(("depth",))["depth"]
        rel = np.abs(depth - gt) / gt
        row = {"multi_scale": levels, "iterations": iters if levels == 0 else fi, "coarse_iterations": ci, "wall_ms": round(wall, 2),
               **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in stages.items() if k != "kernels"},
               "median_rel_err_textureless": round(float(np.median(rel[flat])), 5), "median_rel_err_textured": round(float(np.median(rel[~flat])), 5),
               "kernels": {lv: {k: round(v, 3) for k, v in d.items()} for lv, d in stages["kernels"].items()},
               "size": [args.width, args.height], "views": args.views, "box": args.box}
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for c in [m, *coarse]:
        c.close()


if __name__ == "__main__":
    main()

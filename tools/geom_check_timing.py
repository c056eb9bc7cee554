#!/usr/bin/env python3
"""tools/geom_check_timing.py — kernel time of the geometric-consistency check (tsar_geom_check) beside pm_rescore with the term, on one GPU.

At bench.py's scene size (6048 x 4032, ten sources, box 11, default arithmetic), on the 8-bit decode, with every view's ground-truth
depth map as the installed term and the reference view's ground-truth map as the map to check (device memory in, device memory out,
count and filtered depth both requested).  The two kernels alternate REPS times in one process after a warm-up of each; the
context's kernel timing (hipEvents around each launch) gives the per-launch mean, minimum and maximum.  One JSON line per kernel,
also written to profiles/geom_check/ (README.md there reads the recorded run).

The check's traffic per pixel, from the shapes: 4 B map read + 4 B gather per source + 9 B stored (mask, filtered depth, count).

    timeout -k 10 900 python tools/geom_check_timing.py [--width 6048 --height 4032 --views 10 --reps 10 --out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tsar_mvs_amd import api, synth  # noqa: E402


def one_launch_ms(m, name, call):
    m.reset_kernel_timing()
    call()
    launches, total = m.kernel_timing()[name]
    assert launches == 1, (name, launches)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--box", type=int, default=11)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/geom_check/timing_<W>x<H>_n<views>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "geom_check", "timing_%dx%d_n%d.jsonl" % (args.width, args.height, args.views))
    sc = synth.make_scene(args.width, args.height, args.views, device="cuda", seed=1234, all_gt=True)
    imgs = [im.to(torch.uint8).cpu().numpy() for im in sc.images]
    maps = [None] + [g[0].contiguous() for g in sc.meta["gt_all"][1:]]           # device tensors
    own = sc.gt_depth.contiguous()
    normal_world = (sc.gt_normal.to(torch.float64) @ torch.from_numpy(np.asarray(sc.R[0], np.float64)).cuda()).to(torch.float32).contiguous()   # R^T n
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=args.box, box_vsize=args.box, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, seed=2024))
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.enable_kernel_timing(True)
    m.load_planes(own, normal_world)
    m.set_geom_depths(maps, weight=0.2, clip=3.0)
    res = {}

    def check():
        res.update(m.geom_check(own))

    m.rescore()                                                  # warm-up: code objects loaded, planes scored
    check()
    ms = {"pm_rescore": [], "geom_check": []}
    for _ in range(args.reps):                                   # alternating, so that drift of the machine hits both alike
        ms["pm_rescore"].append(one_launch_ms(m, "pm_rescore", m.rescore))
        ms["geom_check"].append(one_launch_ms(m, "geom_check", check))
    kept = float((res["count"] >= 2).float().mean())
    n_px = args.width * args.height
    lines = []
    for name, t in ms.items():
        row = {"kernel": name, "size": [args.width, args.height], "sources": args.views, "box": args.box, "reps": args.reps,
               "mean_ms": round(float(np.mean(t)), 4), "min_ms": round(float(np.min(t)), 4), "max_ms": round(float(np.max(t)), 4)}
        if name == "geom_check":
            nbytes = n_px * (4 + 4 * args.views + 9)
            row.update({"bytes_from_shapes": nbytes, "gb_per_s_at_mean": round(nbytes / (np.mean(t) * 1e-3) / 1e9, 1), "share_kept_at_defaults": round(kept, 4)})
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
    if args.out:                                                 # (an empty --out: standard output only)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    m.close()


if __name__ == "__main__":
    main()

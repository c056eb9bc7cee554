#!/usr/bin/env python3
"""tools/geom_reproject_timing.py — kernel time of the cross-view render (tsar_geom_reproject) and of its offer to the matcher
(tsar_pm_merge_depths) beside geom_check and pm_rescore with the term, on one GPU.

At bench.py's scene size (6048 x 4032, ten sources, box 11, default arithmetic), on the 8-bit decode, with every view's ground-truth depth
map as the installed term (device memory); the render goes to device memory (depth and count), the merge is offered that render.  The
four calls alternate REPS times in one process after a warm-up of each; the context's kernel timing (hipEvents around each launch) gives
the times.  "geom_reproject" is three launches per call (z-buffer pass with the two memsets, support pass, resolve): the sum per call is
recorded here, and the mean per launch beside it; which of the three dominates is read from a kernel trace of this tool
(profiles/geom_reproject/README.md).  A merge call is one "pm_rescore", one "pm_cost_planes" and two "pm_merge_depths" launches.  One JSON
line per name, also written to profiles/geom_reproject/.

The render's traffic floor per call, from the shapes, with N maps of P pixels: 2 x 4 N P bytes of maps read (both scatter passes),
12 P bytes of temporaries preset, 4 P + 8 P read and 5 P stored by the resolve; and up to N P four-byte and N P eight-byte atomics.

    timeout -k 10 900 python tools/geom_reproject_timing.py [--width 6048 --height 4032 --views 10 --reps 10 --out FILE.jsonl]
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


def call_ms(m, call):
    """{timer name: (launches, total ms)} of one call"""
    m.reset_kernel_timing()
    call()
    return m.kernel_timing()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--box", type=int, default=11)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--min_views", type=int, default=2)
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/geom_reproject/timing_<W>x<H>_n<views>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "geom_reproject", "timing_%dx%d_n%d.jsonl" % (args.width, args.height, args.views))
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
    res, taken = {}, []

    def render():
        res.update(m.geom_reproject(0.01, args.min_views, device=True))

    def merge():
        taken.append(m.merge_depths(res["depth"]))

    def check():
        m.geom_check(own)

    m.rescore()                                                  # warm-up: code objects loaded, planes scored, the arena sized
    for _ in range(2):
        render()
        merge()
        check()
    ms = {"geom_reproject": [], "pm_merge_depths": [], "pm_cost_planes (within the merge)": [], "pm_rescore (within the merge)": [], "geom_check": [], "pm_rescore": []}
    for _ in range(args.reps):                                   # alternating, so that drift of the machine hits all alike
        t = call_ms(m, render)
        assert t["geom_reproject"][0] == 3, t
        ms["geom_reproject"].append(t["geom_reproject"][1])
        t = call_ms(m, merge)
        assert t["pm_merge_depths"][0] == 2 and t["pm_rescore"][0] == 1 and t["pm_cost_planes"][0] == 1, t
        ms["pm_merge_depths"].append(t["pm_merge_depths"][1])
        ms["pm_cost_planes (within the merge)"].append(t["pm_cost_planes"][1])
        ms["pm_rescore (within the merge)"].append(t["pm_rescore"][1])
        ms["geom_check"].append(call_ms(m, check)["geom_check"][1])
        ms["pm_rescore"].append(call_ms(m, m.rescore)["pm_rescore"][1])
    n_px = args.width * args.height
    covered = float((res["depth"] > 0).float().mean())
    landed = float((res["count"] > 0).float().mean())
    lines = []
    for name, t in ms.items():
        row = {"name": name, "size": [args.width, args.height], "sources": args.views, "box": args.box, "reps": args.reps,
               "mean_ms_per_call": round(float(np.mean(t)), 4), "min_ms": round(float(np.min(t)), 4), "max_ms": round(float(np.max(t)), 4)}
        if name == "geom_reproject":
            floor = n_px * (2 * 4 * args.views + 12 + 12 + 5)
            row.update({"launches_per_call": 3, "mean_ms_per_launch": round(float(np.mean(t)) / 3, 4), "floor_bytes_from_shapes": floor,
                        "gb_per_s_of_floor_at_mean": round(floor / (np.mean(t) * 1e-3) / 1e9, 1), "atomics_4B_at_most": n_px * args.views,
                        "atomics_8B_at_most": n_px * args.views, "min_views": args.min_views, "share_covered": round(covered, 4), "share_landed": round(landed, 4)})
        if name == "pm_merge_depths":
            row.update({"launches_per_call": 2, "share_taken_last_call": round(taken[-1] / n_px, 6)})
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

#!/usr/bin/env python3
"""tools/plane_prior_build_timing.py — kernel time of the plane-prior builder (tsar_build_plane_prior) beside tsar_geom_check and
tsar_set_plane_prior, on one GPU.

At bench.py's scene size (6048 x 4032, ten sources, box 11, default arithmetic), on the 8-bit decode, every view's ground-truth depth
map installed as the term.  The builder runs on two candidate maps made from the reference view's ground-truth depth, both in device
memory with a random score, all three outputs requested:
  dense    about 60 % kept: blocks of 48 x 48 pixels kept with probability 0.65, their pixels with probability 0.92 (what a check leaves
           of a scene with weakly textured regions);
  sparse   about 2 % kept: blocks of 16 x 16 pixels kept with probability 0.02 (most level-0 cells are empty: many levels are walked).
The calls alternate REPS times in one process after a warm-up of each; the context's kernel timing (hipEvents around each launch group)
gives per-call times: the builder's three groups (level-0 supports, coarser levels, look-up) and their sum.  One JSON line per row, also
written to profiles/plane_prior_build/ (README.md there reads the recorded run).

The builder's traffic per pixel, from the shapes: 8 B read (depth and score, by the level-0 supports) and 17 B stored (by the look-up);
the look-up's reads are the grids (8 B per cell, L2-resident) and three gathered depths per covered pixel.

    timeout -k 10 900 python tools/plane_prior_build_timing.py [--width 6048 --height 4032 --views 10 --cell 4 --reps 10 --out FILE.jsonl]
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

GROUPS = ("plane_prior_build_supports", "plane_prior_build_levels", "plane_prior_build")


def timed(m, names, call):
    """ms per name of one call"""
    m.reset_kernel_timing()
    call()
    t = m.kernel_timing()
    return [t[n][1] if n in t else 0.0 for n in names]


def block_mask(h, w, block, p_block, p_pixel, gen):
    bh, bw = -(-h // block), -(-w // block)
    blocks = torch.rand((bh, bw), generator=gen, device="cuda") < p_block
    m = blocks.repeat_interleave(block, 0).repeat_interleave(block, 1)[:h, :w]
    if p_pixel < 1:
        m = m & (torch.rand((h, w), generator=gen, device="cuda") < p_pixel)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--box", type=int, default=11)
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/plane_prior_build/timing_<W>x<H>_n<views>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "plane_prior_build", "timing_%dx%d_n%d.jsonl" % (args.width, args.height, args.views))
    w, h = args.width, args.height
    sc = synth.make_scene(w, h, args.views, device="cuda", seed=1234, all_gt=True)
    imgs = [im.to(torch.uint8).cpu().numpy() for im in sc.images]
    maps = [None] + [g[0].contiguous() for g in sc.meta["gt_all"][1:]]           # device tensors
    own = sc.gt_depth.contiguous()
    normal_world = (sc.gt_normal.to(torch.float64) @ torch.from_numpy(np.asarray(sc.R[0], np.float64)).cuda()).to(torch.float32).contiguous()   # R^T n
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    zero = torch.zeros_like(own)
    cand = {"dense": torch.where(block_mask(h, w, 48, 0.65, 0.92, gen), own, zero).contiguous(),
            "sparse": torch.where(block_mask(h, w, 16, 0.02, 1.0, gen), own, zero).contiguous()}
    score = torch.rand((h, w), generator=gen, device="cuda").contiguous()
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=args.box, box_vsize=args.box, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, seed=2024))
    m.set_views(imgs, sc.K, sc.R, sc.t, u8=True)
    m.enable_kernel_timing(True)
    m.set_geom_depths(maps, weight=0.0, clip=3.0)
    built = {}
    calls = {"geom_check": (("geom_check",), lambda: m.geom_check(own)),
             "set_plane_prior": (("plane_prior",), lambda: m.set_plane_prior(own, normal_world))}
    for kind in cand:
        calls["build_" + kind] = (GROUPS, lambda kind=kind: built.__setitem__(kind, m.build_plane_prior(cand[kind], score, cell=args.cell)))
    for names, call in calls.values():                           # warm-up: code objects loaded, the scratch arena at its size
        call()
        call()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                                   # alternating, so that drift of the machine hits all alike
        for k, (names, call) in calls.items():
            ms[k].append(timed(m, names, call))
    n_px = w * h
    lines = []
    for k, (names, _) in calls.items():
        t = np.asarray(ms[k], np.float64)                        # [reps][groups]
        total = t.sum(1)
        row = {"call": k, "size": [w, h], "sources": args.views, "reps": args.reps, "mean_ms": round(float(total.mean()), 4),
               "min_ms": round(float(total.min()), 4), "max_ms": round(float(total.max()), 4)}
        if k.startswith("build_"):
            kind = k[6:]
            lv = built[kind]["level"]
            hist = torch.bincount(lv.flatten().to(torch.int64), minlength=256)
            nbytes = n_px * (8 + 17)
            row.update({"cell": args.cell, "share_candidates": round(float((cand[kind] > 0).float().mean()), 4),
                        "share_covered": round(float((lv != 255).float().mean()), 4),
                        "pixels_per_level": {str(i): int(hist[i]) for i in range(255) if int(hist[i])},
                        "mean_ms_by_group": {n: round(float(v), 4) for n, v in zip(names, t.mean(0))},
                        "bytes_from_shapes": nbytes, "gb_per_s_at_mean": round(nbytes / (total.mean() * 1e-3) / 1e9, 1)})
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

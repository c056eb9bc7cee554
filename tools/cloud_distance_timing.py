#!/usr/bin/env python3
"""tools/cloud_distance_timing.py — kernel times of tsar_cloud_distance on two large synthetic clouds, on one GPU.

Two clouds of N points each in device memory, on the same noisy surfaces: a wavy sheet z = 0.1 sin(7x) cos(5y) over the unit square and
a sphere of radius 0.3, two thirds / one third of the points, each point displaced by Gaussian noise of a quarter of the mean point
spacing s = sqrt(area / N).  The query cloud is drawn independently of the target cloud, as a reconstruction is of a scan.  The call runs
at R = 1, 4 and 16 times s with three tolerances (R, R / 2, R / 4) and both per-query outputs; the context's kernel timing gives the
milliseconds of each launch group (include/tsar.h names them), and `pairs` per second is pairs over the search kernel's time.  For scale:
scipy's cKDTree (float64, one thread) on the first SUBSET queries against the whole target cloud, where scipy imports.

One JSON line per R, also written to profiles/cloud_distance/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_distance_timing.py [--points 20000000 --reps 3 --subset 1000000 --out FILE.jsonl]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tsar_mvs_amd import api  # noqa: E402

GROUPS = ("cloud_bounds", "cloud_keys", "cloud_sort", "cloud_gather", "cloud_pairs", "cloud_distance")
SHEET_AREA, SPHERE_AREA = 1.0, 4.0 * math.pi * 0.3 ** 2


def surface_cloud(n, noise, gen):
    n_sheet = (2 * n) // 3
    xy = torch.rand((n_sheet, 2), generator=gen, device="cuda")
    sheet = torch.cat([xy, (0.1 * torch.sin(7 * xy[:, :1]) * torch.cos(5 * xy[:, 1:]))], 1)
    d = torch.randn((n - n_sheet, 3), generator=gen, device="cuda")
    sphere = 0.3 * d / d.norm(dim=1, keepdim=True) + torch.tensor([0.5, 0.5, 0.6], device="cuda")
    pts = torch.cat([sheet, sphere], 0)
    pts = pts + noise * torch.randn(pts.shape, generator=gen, device="cuda")
    return pts[torch.randperm(n, generator=gen, device="cuda")].to(torch.float32).contiguous()      # no order a scan would not have either


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points per cloud")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subset", type=int, default=1000000, help="queries of the cKDTree comparison (0: skip it)")
    ap.add_argument("--factors", default="1,4,16", help="R in units of the mean point spacing")
    ap.add_argument("--max-pairs", type=int, default=None, dest="max_pairs")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_distance/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_distance", "timing_n%d.jsonl" % args.points)
    n = args.points
    spacing = math.sqrt((SHEET_AREA + SPHERE_AREA) / n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    target = surface_cloud(n, 0.25 * spacing, gen)
    query = surface_cloud(n, 0.25 * spacing, gen)
    m = api.Matcher()
    m.enable_kernel_timing(True)
    lines = []
    tree, tree_build_s = None, None                              # built once, at the first R that runs
    for factor in [float(v) for v in args.factors.split(",")]:
        R = factor * spacing
        tol = [R, R / 2, R / 4]
        row = {"points": n, "mean_spacing": spacing, "R_over_spacing": factor, "R": R, "reps": args.reps}
        try:
            api.cloud_distance(query, target, R, tol, max_pairs=args.max_pairs, matcher=m)           # warm-up: code objects loaded
        except api.TsarError as e:
            row.update({"refused": str(e), "pairs": getattr(e, "pairs", None)})
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
            continue
        ms, wall = [], []
        for _ in range(args.reps):
            m.reset_kernel_timing()
            t0 = time.perf_counter()
            r = api.cloud_distance(query, target, R, tol, max_pairs=args.max_pairs, matcher=m)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = m.kernel_timing()
            ms.append([t[g][1] if g in t else 0.0 for g in GROUPS])
        ms = np.asarray(ms, np.float64)
        search = float(ms[:, GROUPS.index("cloud_distance")].mean())
        row.update({"pairs": r["pairs"], "pairs_per_query": r["pairs"] / n, "within": r["within"].tolist(), "n_valid_query": r["n_valid_query"],
                    "mean_ms_by_group": {g: round(float(v), 3) for g, v in zip(GROUPS, ms.mean(0))}, "kernels_ms_mean": round(float(ms.sum(1).mean()), 3),
                    "kernels_ms_min": round(float(ms.sum(1).min()), 3), "kernels_ms_max": round(float(ms.sum(1).max()), 3),
                    "call_wall_ms_mean": round(float(np.mean(wall)), 3), "pairs_per_s_search_kernel": r["pairs"] / (search * 1e-3) if search > 0 else None})
        if args.subset:
            try:
                from scipy.spatial import cKDTree
                tq = query[:args.subset].cpu().numpy().astype(np.float64)
                if tree is None:
                    t0 = time.perf_counter()
                    tree = cKDTree(target.cpu().numpy().astype(np.float64))
                    tree_build_s = time.perf_counter() - t0
                t1 = time.perf_counter()
                d, _ = tree.query(tq, k=1, distance_upper_bound=R)
                t2 = time.perf_counter()
                d2 = r["dist2"][:args.subset].cpu().numpy()
                both = np.isfinite(d) & np.isfinite(d2)
                row["ckdtree"] = {"queries": len(tq), "build_s": round(tree_build_s, 3), "query_s": round(t2 - t1, 3), "hits": int(np.isfinite(d).sum()),
                                  "hits_here": int(np.isfinite(d2).sum()),
                                  "max_rel_difference_of_distance": float(np.max(np.abs(np.sqrt(d2[both].astype(np.float64)) - d[both]) / d[both].clip(1e-30))) if both.any() else None}
            except ImportError:
                row["ckdtree"] = "scipy does not import"
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

#!/usr/bin/env python3
"""tools/cloud_normals_timing.py — kernel times of tsar_cloud_normals on one large synthetic cloud, on one GPU, beside tsar_cloud_neighbors at
the same radius and k.

One cloud of N points in device memory on the noisy surfaces of tools/cloud_neighbors_timing.py (a wavy sheet and a sphere, Gaussian noise of
a quarter of the mean point spacing s), generated on the device.  The call runs at R = 1, 2 and 4 times s with k = 8, 16 and 32 (the three
list lengths) and every output asked for; the context's kernel timing gives the milliseconds of each launch group (include/tsar.h names them).
Every repetition alternates with a tsar_cloud_neighbors call at the same R and k, in the same process and context: the same pairs looked at,
with a list of 32-bit distances instead of 64-bit codes and nothing after the search.

One JSON line per (R, k), also written to profiles/cloud_normals/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_normals_timing.py [--points 20000000 --reps 3 --out FILE.jsonl]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cloud_distance_timing import SHEET_AREA, SPHERE_AREA, surface_cloud  # noqa: E402
from cloud_neighbors_timing import GROUPS as NEIGHBOR_GROUPS  # noqa: E402
from cloud_neighbors_timing import group_ms  # noqa: E402
from tsar_mvs_amd import api  # noqa: E402

GROUPS = ("cloud_bounds", "cloud_keys", "cloud_sort", "cloud_gather", "cloud_pairs", "cloud_normals")
WANT = ("knn_index", "n_used", "normal", "curvature", "cov")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points of the cloud")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", default="1,2,4", help="R in units of the mean point spacing")
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_normals/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_normals", "timing_n%d.jsonl" % args.points)
    n = args.points
    spacing = math.sqrt((SHEET_AREA + SPHERE_AREA) / n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    cloud = surface_cloud(n, 0.25 * spacing, gen)
    m = api.Matcher()
    m.enable_kernel_timing(True)
    lines = []
    for factor in [float(v) for v in args.factors.split(",")]:
        R = factor * spacing
        for k in [int(v) for v in args.ks.split(",")]:
            row = {"points": n, "mean_spacing": spacing, "R_over_spacing": factor, "R": R, "k": k, "min_neighbors": 5, "reps": args.reps}
            api.cloud_normals(cloud, R, k, want=WANT, matcher=m)                                # warm-up: code objects loaded
            api.cloud_neighbors(cloud, R, k, matcher=m)
            ms, wall, nms, nwall = [], [], [], []
            for _ in range(args.reps):
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                r = api.cloud_normals(cloud, R, k, want=WANT, matcher=m)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(group_ms(m, GROUPS))
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                nb = api.cloud_neighbors(cloud, R, k, matcher=m)
                nwall.append((time.perf_counter() - t0) * 1e3)
                nms.append(group_ms(m, NEIGHBOR_GROUPS))
            ms, nms = np.asarray(ms, np.float64), np.asarray(nms, np.float64)
            by_group = {g: round(float(v), 3) for g, v in zip(GROUPS, ms.mean(0))}
            n_by_group = {g: round(float(v), 3) for g, v in zip(NEIGHBOR_GROUPS, nms.mean(0))}
            fit, search = by_group["cloud_normals"], n_by_group["cloud_neighbors"]
            used = r["n_used"]
            row.update({"n_valid": r["n_valid"], "n_normals": r["n_normals"], "pairs": r["pairs"], "pairs_per_point": r["pairs"] / max(r["n_valid"], 1),
                        "mean_used": float(used.double().mean().item()), "mean_ms_by_group": by_group, "kernels_ms_mean": round(float(ms.sum(1).mean()), 3),
                        "kernels_ms_min": round(float(ms.sum(1).min()), 3), "kernels_ms_max": round(float(ms.sum(1).max()), 3),
                        "call_wall_ms_mean": round(float(np.mean(wall)), 3), "normals_ns_per_pair": 1e6 * fit / max(r["pairs"], 1),
                        "normals_ns_per_point": 1e6 * fit / max(r["n_valid"], 1), "neighbors_pairs": nb["pairs"], "neighbors_mean_ms_by_group": n_by_group,
                        "neighbors_kernels_ms_mean": round(float(nms.sum(1).mean()), 3), "neighbors_call_wall_ms_mean": round(float(np.mean(nwall)), 3),
                        "neighbors_search_ns_per_pair": 1e6 * search / max(nb["pairs"], 1), "normals_over_neighbors_search": round(fit / max(search, 1e-9), 3)})
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

#!/usr/bin/env python3
"""tools/cloud_neighbors_timing.py — kernel times of tsar_cloud_neighbors on one large synthetic cloud, on one GPU, beside tsar_cloud_distance
of the cloud against itself.

One cloud of N points in device memory on the noisy surfaces of tools/cloud_distance_timing.py (a wavy sheet and a sphere, Gaussian noise of a
quarter of the mean point spacing s), generated on the device.  The call runs at R = 1, 2 and 4 times s with k = 0 (the count-only kernel), 8
and 32 (the lists of 8 and 32 entries); the context's kernel timing gives the milliseconds of each launch group (include/tsar.h names them).
Every repetition alternates with a tsar_cloud_distance call of the cloud against itself at the same R, in the same process and context: the
nearest thing the library could do before, looking at the same pairs with the same record loads and keeping a single minimum.

One JSON line per (R, k), also written to profiles/cloud_neighbors/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_neighbors_timing.py [--points 20000000 --reps 3 --out FILE.jsonl]
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
from cloud_distance_timing import GROUPS as DISTANCE_GROUPS  # noqa: E402
from tsar_mvs_amd import api  # noqa: E402

GROUPS = ("cloud_bounds", "cloud_keys", "cloud_sort", "cloud_gather", "cloud_pairs", "cloud_neighbors")
RECORD_BYTES = 16                                                     # one (x, y, z, index) record per pair looked at


def group_ms(m, groups):
    t = m.kernel_timing()
    return [t[g][1] if g in t else 0.0 for g in groups]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points of the cloud")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", default="1,2,4", help="R in units of the mean point spacing")
    ap.add_argument("--ks", default="0,8,32")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_neighbors/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_neighbors", "timing_n%d.jsonl" % args.points)
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
        api.cloud_distance(cloud, cloud, R, matcher=m)                                          # warm-up of the distance call
        for k in [int(v) for v in args.ks.split(",")]:
            row = {"points": n, "mean_spacing": spacing, "R_over_spacing": factor, "R": R, "k": k, "reps": args.reps}
            api.cloud_neighbors(cloud, R, k, matcher=m)                                         # warm-up: code objects loaded
            ms, wall, dms, dwall = [], [], [], []
            for _ in range(args.reps):
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                r = api.cloud_neighbors(cloud, R, k, matcher=m)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(group_ms(m, GROUPS))
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                d = api.cloud_distance(cloud, cloud, R, matcher=m)
                dwall.append((time.perf_counter() - t0) * 1e3)
                dms.append(group_ms(m, DISTANCE_GROUPS))
            ms, dms = np.asarray(ms, np.float64), np.asarray(dms, np.float64)
            by_group = {g: round(float(v), 3) for g, v in zip(GROUPS, ms.mean(0))}
            d_by_group = {g: round(float(v), 3) for g, v in zip(DISTANCE_GROUPS, dms.mean(0))}
            search, d_search = by_group["cloud_neighbors"], d_by_group["cloud_distance"]
            count = r["count"]
            row.update({"n_valid": r["n_valid"], "pairs": r["pairs"], "pairs_per_point": r["pairs"] / max(r["n_valid"], 1),
                        "mean_count": float(count.double().mean().item()), "max_count": int(count.max().item()),
                        "mean_ms_by_group": by_group, "kernels_ms_mean": round(float(ms.sum(1).mean()), 3), "kernels_ms_min": round(float(ms.sum(1).min()), 3),
                        "kernels_ms_max": round(float(ms.sum(1).max()), 3), "call_wall_ms_mean": round(float(np.mean(wall)), 3),
                        "search_ns_per_pair": 1e6 * search / max(r["pairs"], 1), "search_record_load_GB_per_s": RECORD_BYTES * r["pairs"] / max(search, 1e-9) / 1e6,
                        "distance_pairs": d["pairs"], "distance_mean_ms_by_group": d_by_group, "distance_kernels_ms_mean": round(float(dms.sum(1).mean()), 3),
                        "distance_call_wall_ms_mean": round(float(np.mean(dwall)), 3), "distance_search_ns_per_pair": 1e6 * d_search / max(d["pairs"], 1),
                        "distance_search_record_load_GB_per_s": RECORD_BYTES * d["pairs"] / max(d_search, 1e-9) / 1e6,
                        "search_within_the_distance_search_per_pair": bool(search / max(r["pairs"], 1) <= d_search / max(d["pairs"], 1))})
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

#!/usr/bin/env python3
"""tools/cloud_voxel_timing.py — kernel times of tsar_cloud_voxels on one large synthetic cloud, on one GPU, beside tsar_cloud_distance.

One cloud of N points in device memory on the noisy surfaces of tools/cloud_distance_timing.py (a wavy sheet and a sphere, Gaussian noise of a
quarter of the mean point spacing s).  The call runs at V = 1, 4 and 16 times s, once with every output but no distances, once with dist2 (the
distance call's output against a second cloud) and three tolerances; the context's kernel timing gives the milliseconds of each launch group
(include/tsar.h names them).  Every repetition alternates with a tsar_cloud_distance call at R = s in the same process and context, so that the
two totals are measured under the same conditions.

One JSON line per (V, with / without dist2), also written to profiles/cloud_voxels/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_voxel_timing.py [--points 20000000 --reps 3 --out FILE.jsonl]
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

GROUPS = ("cloud_bounds", "voxel_keys", "cloud_sort", "voxel_heads", "voxel_scan", "voxel_reduce", "voxel_finish")


def group_ms(m, groups):
    t = m.kernel_timing()
    return [t[g][1] if g in t else 0.0 for g in groups]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points of the cloud")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", default="1,4,16", help="V in units of the mean point spacing")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_voxels/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_voxels", "timing_n%d.jsonl" % args.points)
    n = args.points
    spacing = math.sqrt((SHEET_AREA + SPHERE_AREA) / n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    other = surface_cloud(n, 0.25 * spacing, gen)
    cloud = surface_cloud(n, 0.25 * spacing, gen)
    m = api.Matcher()
    m.enable_kernel_timing(True)
    R = spacing
    tol = [R, R / 2, R / 4]
    dist2 = api.cloud_distance(cloud, other, R, tol, want=("dist2",), matcher=m)["dist2"]     # (also the distance call's warm-up)
    lines = []
    for factor in [float(v) for v in args.factors.split(",")]:
        V = factor * spacing
        for with_dist2 in (False, True):
            kw = {"dist2": dist2, "tolerances": tol} if with_dist2 else {}
            row = {"points": n, "mean_spacing": spacing, "V_over_spacing": factor, "V": V, "with_dist2_and_3_tolerances": with_dist2, "reps": args.reps}
            api.cloud_voxels(cloud, V, matcher=m, **kw)                                         # warm-up: code objects loaded
            ms, wall, dms, dwall = [], [], [], []
            for _ in range(args.reps):
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                r = api.cloud_voxels(cloud, V, matcher=m, **kw)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(group_ms(m, GROUPS))
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                api.cloud_distance(cloud, other, R, tol, matcher=m)
                dwall.append((time.perf_counter() - t0) * 1e3)
                dms.append(group_ms(m, DISTANCE_GROUPS))
            ms, dms = np.asarray(ms, np.float64), np.asarray(dms, np.float64)
            by_group = {g: round(float(v), 3) for g, v in zip(GROUPS, ms.mean(0))}
            row.update({"n_voxels": r["n_voxels"], "n_valid": r["n_valid"], "points_per_voxel": r["n_valid"] / max(r["n_voxels"], 1),
                        "mean_ms_by_group": by_group, "largest_group": max(by_group, key=by_group.get),
                        "kernels_ms_mean": round(float(ms.sum(1).mean()), 3), "kernels_ms_min": round(float(ms.sum(1).min()), 3),
                        "kernels_ms_max": round(float(ms.sum(1).max()), 3), "call_wall_ms_mean": round(float(np.mean(wall)), 3),
                        "distance_call_R_over_spacing": 1.0, "distance_kernels_ms_mean": round(float(dms.sum(1).mean()), 3),
                        "distance_kernels_ms_min": round(float(dms.sum(1).min()), 3), "distance_kernels_ms_max": round(float(dms.sum(1).max()), 3),
                        "distance_call_wall_ms_mean": round(float(np.mean(dwall)), 3),
                        "below_the_distance_call": bool(ms.sum(1).mean() < dms.sum(1).mean())})
            if with_dist2:
                row["within_total"] = r["within"].sum(dim=0).tolist()
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

#!/usr/bin/env python3
"""tools/cloud_render_timing.py — kernel times of tsar_cloud_render and tsar_depth_compare on one large synthetic cloud, on one GPU.

One cloud of N points in device memory on the noisy surfaces of tools/cloud_distance_timing.py (a wavy sheet and a sphere, Gaussian noise of a
quarter of the mean point spacing s), rendered into a W x H camera that looks at them along +z from 1.2 units in front of the sheet, with a
focal length that makes s about 1.3 pixels there.  The render runs at radius = 0, 1 and 2 times s, each with the footprint loop's plain load
that lets a lane skip a minimum (the default) and without it (TSAR_RENDER_SKIP=0, a context of its own); the context's kernel timing gives
the milliseconds of each launch (include/tsar.h names them).  tsar_depth_compare is timed on the rendered map against a noisy copy, with and
without error_out.

One JSON line per (radius, skip) and two for the comparison, also written to profiles/cloud_render/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_render_timing.py [--points 20000000 --width 6048 --height 4032 --reps 3 --out FILE.jsonl]
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
from tsar_mvs_amd import api  # noqa: E402

GROUPS = ("cloud_render_count", "cloud_render_scatter", "cloud_render_support", "cloud_render_resolve")


def group_ms(m, groups):
    t = m.kernel_timing()
    return [t[g][1] if g in t else 0.0 for g in groups]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points of the cloud")
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", default="0,1,2", help="radius in units of the mean point spacing")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_render/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_render", "timing_n%d.jsonl" % args.points)
    n, w, h = args.points, args.width, args.height
    spacing = math.sqrt((SHEET_AREA + SPHERE_AREA) / n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    cloud = surface_cloud(n, 0.25 * spacing, gen)
    dist = 1.2
    f = 1.3 * dist / spacing                                      # one mean spacing is 1.3 pixels at the sheet
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)
    R = np.eye(3, dtype=np.float32)
    t = np.array([-0.5, -0.5, dist], np.float32)
    lines = []
    depth = None
    for factor in [float(v) for v in args.factors.split(",")]:
        for skip in ((1,) if factor == 0 else (1, 0)):
            os.environ["TSAR_RENDER_SKIP"] = str(skip)          # read once, when the context is created
            m = api.Matcher()
            m.enable_kernel_timing(True)
            kw = dict(radius=factor * spacing, want=("depth", "count"), matcher=m)
            row = {"points": n, "width": w, "height": h, "focal": f, "mean_spacing": spacing, "radius_over_spacing": factor, "load_before_atomic_skip": bool(skip),
                   "reps": args.reps}
            api.cloud_render(cloud, K, R, t, w, h, **kw)                                     # warm-up: code objects loaded
            ms, wall = [], []
            for _ in range(args.reps):
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                r = api.cloud_render(cloud, K, R, t, w, h, **kw)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(group_ms(m, GROUPS))
            ms = np.asarray(ms, np.float64)
            by_group = {g: round(float(v), 3) for g, v in zip(GROUPS, ms.mean(0))}
            scatter = float(ms[:, 1].mean())
            row.update({"n_splats": r["n_splats"], "splats_per_point": r["n_splats"] / n, "pixels_kept": int((r["depth"] > 0).sum().item()),
                        "mean_ms_by_launch": by_group, "scatter_ms_min": round(float(ms[:, 1].min()), 3), "scatter_ms_max": round(float(ms[:, 1].max()), 3),
                        "kernels_ms_mean": round(float(ms.sum(1).mean()), 3), "kernels_ms_min": round(float(ms.sum(1).min()), 3),
                        "kernels_ms_max": round(float(ms.sum(1).max()), 3), "call_wall_ms_mean": round(float(np.mean(wall)), 3),
                        "splats_per_second_in_the_scatter": r["n_splats"] / (scatter * 1e-3) if scatter > 0 else None})
            if row["splats_per_second_in_the_scatter"]:
                row["seconds_of_scatter_at_the_default_max_splats"] = float(1 << 34) / row["splats_per_second_in_the_scatter"]
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            if factor > 0 and skip:
                depth = r["depth"]
            m.close()
    os.environ.pop("TSAR_RENDER_SKIP", None)
    if depth is None:
        depth = api.cloud_render(cloud, K, R, t, w, h, want=("depth",))["depth"]
    noisy = (depth * (1 + 5e-3 * torch.randn(depth.shape, generator=gen, device="cuda"))).contiguous()
    m = api.Matcher()
    m.enable_kernel_timing(True)
    for want_error in (False, True):
        api.depth_compare(noisy, depth, [0.001, 0.01], want_error=want_error, matcher=m)
        ms = []
        for _ in range(args.reps):
            m.reset_kernel_timing()
            r = api.depth_compare(noisy, depth, [0.001, 0.01], want_error=want_error, matcher=m)
            ms.append(group_ms(m, ("depth_compare",))[0])
        row = {"depth_compare": True, "pixels": w * h, "error_out": want_error, "n_gt": r["n_gt"], "n_both": r["n_both"], "within": r["within"].tolist(),
               "kernel_ms_mean": round(float(np.mean(ms)), 3), "kernel_ms_min": round(float(np.min(ms)), 3), "kernel_ms_max": round(float(np.max(ms)), 3),
               "bytes_read_and_written": w * h * (8 + (4 if want_error else 0))}
        row["GB_per_second"] = row["bytes_read_and_written"] / (row["kernel_ms_mean"] * 1e-3) / 1e9 if row["kernel_ms_mean"] > 0 else None
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
    m.close()
    if args.out:                                                 # (an empty --out: standard output only)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/cloud_splat_timing.py — kernel times of tsar_cloud_render_oriented beside tsar_cloud_render on one large synthetic cloud, on one GPU.

The cloud, the camera and the settings are tools/cloud_render_timing.py's: N points in device memory on the noisy surfaces of
tools/cloud_distance_timing.py (a wavy sheet and a sphere, Gaussian noise of a quarter of the mean point spacing s), in random order, seen
along +z from 1.2 units in front of the sheet with a focal length that makes s about 1.3 pixels there.  The normals are the surfaces' own
(the sheet's gradient, the sphere's radius), not estimated: the draws are surface_cloud's, in its order, so the points are the same bits.
Per radius (1, 2 and 4 times s) the square and the oriented render alternate in one context, one warm-up call each and then `reps` timed
pairs; the context's kernel timing gives the milliseconds of each launch (include/tsar.h names them).

One JSON line per radius, also written to profiles/cloud_splat/ (README.md there reads the recorded run).

    timeout -k 10 900 python tools/cloud_splat_timing.py [--points 20000000 --width 6048 --height 4032 --reps 3 --out FILE.jsonl]
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

SQUARE = ("cloud_render_count", "cloud_render_scatter", "cloud_render_support", "cloud_render_resolve")
ORIENTED = ("cloud_splat_count", "cloud_splat_scatter", "cloud_splat_support", "cloud_splat_resolve")


def surface_cloud_with_normals(n, noise, gen):
    """surface_cloud's points, draw for draw, and the unit normal of the noiseless surface under each -> ([n, 3], [n, 3]) float32"""
    n_sheet = (2 * n) // 3
    xy = torch.rand((n_sheet, 2), generator=gen, device="cuda")
    x, y = xy[:, :1], xy[:, 1:]
    sheet = torch.cat([xy, 0.1 * torch.sin(7 * x) * torch.cos(5 * y)], 1)
    sheet_n = torch.cat([-0.7 * torch.cos(7 * x) * torch.cos(5 * y), 0.5 * torch.sin(7 * x) * torch.sin(5 * y), torch.ones_like(x)], 1)      # (-dz/dx, -dz/dy, 1)
    d = torch.randn((n - n_sheet, 3), generator=gen, device="cuda")
    unit = d / d.norm(dim=1, keepdim=True)
    sphere = 0.3 * d / d.norm(dim=1, keepdim=True) + torch.tensor([0.5, 0.5, 0.6], device="cuda")
    pts = torch.cat([sheet, sphere], 0)
    nrm = torch.cat([sheet_n / sheet_n.norm(dim=1, keepdim=True), unit], 0)
    pts = pts + noise * torch.randn(pts.shape, generator=gen, device="cuda")
    perm = torch.randperm(n, generator=gen, device="cuda")
    return pts[perm].to(torch.float32).contiguous(), nrm[perm].to(torch.float32).contiguous()


def group_ms(m, groups):
    t = m.kernel_timing()
    return [t[g][1] if g in t else 0.0 for g in groups]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000, help="points of the cloud")
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factors", default="1,2,4", help="radius in units of the mean point spacing")
    ap.add_argument("--out", default=None, help="where the JSON lines go as well (default: profiles/cloud_splat/timing_n<points>.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cloud_splat", "timing_n%d.jsonl" % args.points)
    n, w, h = args.points, args.width, args.height
    spacing = math.sqrt((SHEET_AREA + SPHERE_AREA) / n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    cloud, normals = surface_cloud_with_normals(n, 0.25 * spacing, gen)
    gen.manual_seed(7)
    assert torch.equal(cloud, surface_cloud(n, 0.25 * spacing, gen)), "the cloud is no longer tools/cloud_render_timing.py's"
    dist = 1.2
    f = 1.3 * dist / spacing                                      # one mean spacing is 1.3 pixels at the sheet
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)
    R = np.eye(3, dtype=np.float32)
    t = np.array([-0.5, -0.5, dist], np.float32)
    lines = []
    m = api.Matcher()
    m.enable_kernel_timing(True)
    for factor in [float(v) for v in args.factors.split(",")]:
        kw = dict(radius=factor * spacing, want=("depth", "count"), matcher=m)
        forms = (("square", None, SQUARE), ("oriented", normals, ORIENTED))
        for _, nrm, _ in forms:                                   # warm-up: code objects loaded
            api.cloud_render(cloud, K, R, t, w, h, normals=nrm, **kw)
        ms = {name: [] for name, _, _ in forms}
        wall = {name: [] for name, _, _ in forms}
        last = {}
        for _ in range(args.reps):
            for name, nrm, groups in forms:                       # the two forms alternate
                m.reset_kernel_timing()
                t0 = time.perf_counter()
                last[name] = api.cloud_render(cloud, K, R, t, w, h, normals=nrm, **kw)
                wall[name].append((time.perf_counter() - t0) * 1e3)
                ms[name].append(group_ms(m, groups))
        row = {"points": n, "width": w, "height": h, "focal": f, "mean_spacing": spacing, "radius_over_spacing": factor, "reps": args.reps,
               "n_splats": last["oriented"]["n_splats"], "n_covered": last["oriented"]["n_covered"],
               "covered_over_examined": last["oriented"]["n_covered"] / max(last["oriented"]["n_splats"], 1)}
        assert last["square"]["n_splats"] == last["oriented"]["n_splats"]
        for name, _, groups in forms:
            a = np.asarray(ms[name], np.float64)
            row[name] = {"mean_ms_by_launch": {g: round(float(v), 3) for g, v in zip(groups, a.mean(0))}, "scatter_ms_min": round(float(a[:, 1].min()), 3),
                         "scatter_ms_max": round(float(a[:, 1].max()), 3), "kernels_ms_mean": round(float(a.sum(1).mean()), 3),
                         "call_wall_ms_mean": round(float(np.mean(wall[name])), 3), "pixels_kept": int((last[name]["depth"] > 0).sum().item())}
        row["oriented_over_square_scatter"] = round(row["oriented"]["mean_ms_by_launch"][ORIENTED[1]] / row["square"]["mean_ms_by_launch"][SQUARE[1]], 3)
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

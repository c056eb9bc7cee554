#!/usr/bin/env python3
"""CPU-only census of the sweep's partial-window bound (tsar-mvs_amd/csrc/pm_tap_common.h prune_proven): how often
the pruning kernels would leave a refinement view early, per lane and per wave, and whether a proven (lane, view) ever scores below
the lane's cost.  The check is restated in numpy float32 as the kernel evaluates it: the same taps in the same order (rows of six),
sequential fp32 sums, the same test with the same constants.  Fused multiply-adds are formed in float64 and rounded
once (the product of two floats is exact there).  The truth it is held against is the CPU oracle's restatement of the fast
arithmetic, one view at a time (Oracle.pm_cost); without a device the oracle's reciprocal is the correctly rounded one, which moves a
tap by ~1e-4 pixel and a cost by ~1e-5, three hundred times less than the margin.

    python tools/prune_bound_census.py [--width 768 --height 512 --views 10 --waves 600 --iters 1,2,4,8]

prints one JSON line per (state, step).  tests/test_prune_bound_cpu.py imports the functions below."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

f32 = np.float32
# pm_tap_common.h / pm_tap_r5.h
E_FULL, E_PART, SLACK = f32(0.9), f32(0.45), f32(1.0e-4)
FIRST_LINE, LAST_LINE = 2, 4
OFFS = np.arange(-5, 6, 2)


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def reference_window(img, xs, ys):
    """weights and reference texels of the box-11 window of pixels (xs, ys), [N, row, tap along x], and the hoisted PixelRef terms
    (hoist_reference: summed column by column)"""
    h, w = img.shape
    yy = np.clip(ys[:, None, None] + OFFS[None, :, None], 0, h - 1)
    xx = np.clip(xs[:, None, None] + OFFS[None, None, :], 0, w - 1)
    r = img[yy, xx].astype(f32)
    cen = img[ys, xs].astype(f32)[:, None, None]
    sd = np.sqrt((OFFS[None, :, None] ** 2 + OFFS[None, None, :] ** 2).astype(f32))
    wt = np.exp(-sd / f32(50.0) - np.abs(r - cen) / f32(18.0)).astype(f32)
    s_r = np.zeros(len(xs), f32); s_rr = np.zeros(len(xs), f32); s_w = np.zeros(len(xs), f32)
    for i in range(6):            # column
        for j in range(6):        # row
            wr = wt[:, j, i] * r[:, j, i]
            s_r = s_r + wr
            s_rr = fma(wr, r[:, j, i], s_rr)
            s_w = s_w + wt[:, j, i]
    inv_wsum = f32(1.0) / s_w
    mean = s_r * inv_wsum
    var_ref = s_rr * inv_wsum - mean * mean
    return wt, r, inv_wsum, var_ref


def warped_samples(H, img, xs, ys):
    """the fast arithmetic's samples of the window under homographies H [N, 9]: [N, row, tap along x]"""
    h, w = img.shape
    H = H.astype(f32)
    yi = (ys[:, None] + OFFS[None, :]).astype(f32)                    # [N, row]
    xj = (xs[:, None] + OFFS[None, :]).astype(f32)                    # [N, tap]
    bx = fma(H[:, 1, None], yi, H[:, 2, None]); by = fma(H[:, 4, None], yi, H[:, 5, None]); bz = fma(H[:, 7, None], yi, H[:, 8, None])
    X = fma(H[:, 0, None, None], xj[:, None, :], bx[:, :, None])
    Y = fma(H[:, 3, None, None], xj[:, None, :], by[:, :, None])
    Z = fma(H[:, 6, None, None], xj[:, None, :], bz[:, :, None])
    with np.errstate(all="ignore"):
        rz = f32(1.0) / Z
        u = np.clip(np.nan_to_num(X * rz, nan=0.0), f32(0.0), f32(w - 1))
        v = np.clip(np.nan_to_num(Y * rz, nan=0.0), f32(0.0), f32(h - 1))
    fu, fv = np.floor(u), np.floor(v)
    ax, ay = (u - fu).astype(f32), (v - fv).astype(f32)
    iu, iv = fu.astype(np.int64), fv.astype(np.int64)
    iu1, iv1 = np.minimum(iu + 1, w - 1), np.minimum(iv + 1, h - 1)
    t00, t10, t01, t11 = img[iv, iu], img[iv, iu1], img[iv1, iu], img[iv1, iu1]
    d1, d2, d3 = t10 - t00, t01 - t00, (t11 - t01) - (t10 - t00)
    return fma(ay, fma(ax, d3, d2), fma(ax, d1, t00))


def proven_after_lines(wt, r, s, inv_wsum, var_ref, cost_now):
    """prune_proven after lines FIRST_LINE .. LAST_LINE: bool [N, n_checks] (a lane's own verdicts, no wave vote).  The device's
    v_rcp_f32 / v_rsq_f32 (1 ulp) are the correctly rounded operations here: the slack term covers them."""
    n = wt.shape[0]
    z = lambda: np.zeros(n, f32)
    one = f32(1.0)
    src, src_src, ref_src = z(), z(), z()
    out = []
    with np.errstate(all="ignore"):
        for line in range(LAST_LINE):
            for j in range(6):
                w_, r_, s_ = wt[:, line, j], r[:, line, j], s[:, line, j]
                ws = w_ * s_
                src = src + ws
                src_src = fma(ws, s_, src_src)
                ref_src = fma(ws, r_, ref_src)
            if line + 1 < FIRST_LINE:
                continue
            aw, ar, arr = z(), z(), z()
            for l in range(line + 1):
                for j in range(6):
                    w_, r_ = wt[:, l, j], r[:, l, j]
                    wr = w_ * r_
                    aw = aw + w_
                    ar = ar + wr
                    arr = fma(wr, r_, arr)
            E = E_PART * aw * aw
            a_lo = fma(aw, arr, -(ar * ar)) - E
            b_lo = fma(aw, src_src, -(src * src)) - E
            c_hi = np.abs(fma(aw, ref_src, -(ar * src))) + E
            raw = one / aw
            q = fma(-(c_hi * c_hi), one / b_lo, a_lo) * raw
            vs, vr = (b_lo * raw) * inv_wsum, var_ref - E_FULL
            n2 = fma(-q, inv_wsum * (one / (var_ref + E_FULL)), one)
            eg = E_FULL * (one / np.sqrt(vr * vs)).astype(f32)
            tt = one - cost_now
            lhs = fma(eg, f32(2.0) + eg, n2)
            rhs = (fma(tt, tt, -SLACK) * (one - E_FULL * (one / vr))) * (one - E_FULL * (one / vs))
            out.append((cost_now < one) & (vr >= f32(2.0) * E_FULL) & (vs >= f32(2.0) * E_FULL) & (lhs <= rhs))
    return np.stack(out, axis=1)


def draw_hypotheses(orc, sc, xs, ys, step, rng):
    """fresh refinement hypotheses of step `step` around the oracle's current planes, as planeRefinement draws them (widths 1 / 4^step
    and max_disp / 2 / 10^step; numpy's generator in place of the kernels' Philox stream): planes [N, 4]"""
    n4 = orc.norm4[ys, xs].astype(f32)
    fb = f32(orc.max_disp) * f32(sc.depth_min)
    dN, dZ = f32(1.0) / f32(4.0) ** step, f32(orc.max_disp) / f32(2.0) / f32(10.0) ** step
    out = np.empty((len(xs), 4), f32)
    for i in range(len(xs)):
        x, y = int(xs[i]), int(ys[i])
        depth = orc.depth_from_plane(n4[i], x, y)
        disp = fb / f32(depth)
        lo, hi = -min(dZ, f32(orc.min_disp) + disp), min(dZ, f32(orc.max_disp) - disp)
        d_out = min(max(disp + f32(rng.uniform(lo, hi)), f32(orc.min_disp)), f32(orc.max_disp))
        nt = n4[i, :3] + rng.uniform(-dN, dN, 3).astype(f32)
        nt = (nt / np.sqrt(np.dot(nt, nt))).astype(f32)
        if np.dot(nt, orc.view_vector(x, y)) > 0:
            nt = -nt
        out[i, :3] = nt
        out[i, 3] = orc.getD(nt, x, y, float(fb / d_out))
    return out


def exact_rcp_table():
    """a stand-in for the device's v_rcp_f32 table where there is no device: the correctly rounded reciprocals"""
    return (f32(1.0) / (f32(1.0) + np.arange(1 << 23, dtype=np.float64) * 2.0 ** -23).astype(f32)).astype(f32)


def fast_oracle(sc, seed, ol, table):
    orc = ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, seed=seed, flags=ol.FLAGS_FAST_8BIT_IMAGERY)
    orc.set_rcp_table(table)
    return orc


def census(orc, sc, xs, ys, step, rng, with_costs=True):
    """for pixels (xs, ys) and one fresh hypothesis each: verdicts [N, views, checks], the oracle's per-view costs [N, views] and cost_now"""
    img0 = orc.images[0]
    wt, r, inv_wsum, var_ref = reference_window(img0, xs, ys)
    planes = draw_hypotheses(orc, sc, xs, ys, step, rng)
    cost_now = orc.c[ys, xs].astype(f32)
    views = list(range(1, orc.n_views))
    verdict = np.zeros((len(xs), len(views), LAST_LINE - FIRST_LINE + 1), bool)
    costs = np.zeros((len(xs), len(views)), f32)
    for k, v in enumerate(views):
        H = np.stack([orc.homography(v, planes[i]).reshape(9) for i in range(len(xs))])
        s = warped_samples(H, orc.images[v], xs, ys)
        verdict[:, k] = proven_after_lines(wt, r, s, inv_wsum, var_ref, cost_now)
        if with_costs:
            costs[:, k] = [orc.pm_cost(v, int(xs[i]), int(ys[i]), planes[i]) for i in range(len(xs))]
    return verdict, costs, cost_now, var_ref


def wave_pixels(w, h, n_waves, colour, rng):
    """pixels of n_waves whole waves with the sweep's lane -> pixel map (4 rows x 16 pixels of one colour in a 32 x 4 strip): [waves, 64]"""
    xs, ys = [], []
    for _ in range(n_waves):
        x0, y0 = 32 * int(rng.integers(0, w // 32)), 4 * int(rng.integers(0, h // 4))
        ly, k = np.divmod(np.arange(64), 16)
        y = y0 + ly
        xs.append(x0 + 2 * k + ((colour + y) & 1)); ys.append(y)
    return np.array(xs), np.array(ys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=768); ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--views", type=int, default=10); ap.add_argument("--waves", type=int, default=600)
    ap.add_argument("--iters", default="1,2,4,8"); ap.add_argument("--steps", default="0,1,2")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import oracle_lib as ol
    from tsar_mvs_amd import synth
    sc = synth.make_scene(args.width, args.height, args.views, seed=21)
    orc = fast_oracle(sc, 17, ol, exact_rcp_table())
    orc.pm_init()
    done = 0
    rng = np.random.default_rng(5)
    for it in [int(v) for v in args.iters.split(",")]:
        orc.pm_iterate(it - done); done = it
        wx, wy = wave_pixels(args.width, args.height, args.waves, 0, rng)
        for step in [int(v) for v in args.steps.split(",")]:
            verdict, costs, cost_now, var_ref = census(orc, sc, wx.reshape(-1), wy.reshape(-1), step, rng)
            nv = verdict.shape[1]
            cum = np.logical_or.accumulate(verdict, axis=2)                       # proven at or before each check
            wave = cum.reshape(args.waves, 64, nv, -1).all(axis=1)               # every lane of the wave
            first = np.where(wave.any(axis=2), wave.argmax(axis=2) + FIRST_LINE, 6)
            below = costs < cost_now[:, None]
            print(json.dumps({"after_iters": it, "step": step, "lane_view_proven": [round(float(v), 4) for v in cum.mean(axis=(0, 1))],
                              "wave_view_all_proven": [round(float(v), 4) for v in wave.mean(axis=(0, 1))],
                              "tap_work_left": round(float(first.mean() / 6.0), 4), "lanes_accepting": round(float(below.any(axis=1).mean()), 5),
                              "proven_but_below": int((cum[:, :, -1] & below).sum()), "samples": int(cum[:, :, -1].size),
                              "var_ref_p10": round(float(np.percentile(var_ref, 10)), 1)}), flush=True)


if __name__ == "__main__":
    main()

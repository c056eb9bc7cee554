#!/usr/bin/env python3
"""CPU-only census of the sweep's partial-window bound (tsar-mvs_amd/csrc/pm_tap_common.h prune_proven): how often
the pruning kernels would leave a refinement view early, per lane and per wave, and whether a proven (lane, view) ever scores below
the lane's cost.  The check is restated in numpy float32 as the kernel evaluates it: the same taps in the same order (rows of six),
sequential fp32 sums, the same test with the same constants.  Fused multiply-adds are formed in float64 and rounded
once (the product of two floats is exact there).  The truth it is held against is the CPU oracle's restatement of the fast
arithmetic, one view at a time (Oracle.pm_cost); without a device the oracle's reciprocal is the correctly rounded one, which moves a
tap by ~1e-4 pixel and a cost by ~1e-5, three hundred times less than the margin.

    python tools/prune_bound_census.py [--width 768 --height 512 --views 10 --waves 600 --iters 1,2,4,8]

prints one JSON line per (state, step).

    python tools/prune_bound_census.py --adversarial [--windows 20000]

holds the same restatement to synthetic windows chosen to sit at the rounding allowances (bright, low-variance, binary, nearly
weightless and uniform references; sources whose first lines say nothing of the rest, noisy copies, inverted halves, unrelated ones)
and prints one JSON line per (class, mode): eligible windows, windows proven at cost_now = 0.02, false proofs with cost_now just
above the window's own cost, the largest |fp32 - float64| cost.  tests/test_prune_bound_cpu.py and
tests/test_prune_bound_adversarial_cpu.py import the functions below."""
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


def window_weights(r, cen):
    """the kernel's tap weights exp(-sd / 50 - |r - centre| / 18) of box-11 windows r [N, row, tap along x] with centre texels cen [N]"""
    sd = np.sqrt((OFFS[None, :, None] ** 2 + OFFS[None, None, :] ** 2).astype(f32))
    return np.exp(-sd / f32(50.0) - np.abs(r - cen[:, None, None]) / f32(18.0)).astype(f32)


def hoisted_terms(wt, r):
    """the hoisted PixelRef terms of windows with weights wt and reference texels r (hoist_reference: summed column by column):
    inv_wsum, mean_ref, var_ref"""
    n = wt.shape[0]
    s_r = np.zeros(n, f32); s_rr = np.zeros(n, f32); s_w = np.zeros(n, f32)
    for i in range(6):            # column
        for j in range(6):        # row
            wr = wt[:, j, i] * r[:, j, i]
            s_r = s_r + wr
            s_rr = fma(wr, r[:, j, i], s_rr)
            s_w = s_w + wt[:, j, i]
    inv_wsum = f32(1.0) / s_w
    mean = s_r * inv_wsum
    var_ref = s_rr * inv_wsum - mean * mean
    return inv_wsum, mean, var_ref


def reference_window_mean(img, xs, ys):
    """weights and reference texels of the box-11 window of pixels (xs, ys), [N, row, tap along x], and the hoisted PixelRef terms
    inv_wsum, mean_ref, var_ref"""
    h, w = img.shape
    yy = np.clip(ys[:, None, None] + OFFS[None, :, None], 0, h - 1)
    xx = np.clip(xs[:, None, None] + OFFS[None, None, :], 0, w - 1)
    r = img[yy, xx].astype(f32)
    wt = window_weights(r, img[ys, xs].astype(f32))
    inv_wsum, mean, var_ref = hoisted_terms(wt, r)
    return wt, r, inv_wsum, mean, var_ref


def reference_window(img, xs, ys):
    """reference_window_mean without the mean: wt, r, inv_wsum, var_ref"""
    wt, r, inv_wsum, _, var_ref = reference_window_mean(img, xs, ys)
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


MAXCOST = f32(2.0)


def full_window_cost(wt, r, s, inv_wsum, mean_ref, var_ref):
    """the fast arithmetic's cost of the whole window: tap_accumulate<false> over rows of six, then ncc_cost's tail with the correctly
    rounded root (sqrt_rsq_exact is one); MAXCOST below the variance thresholds"""
    n = wt.shape[0]
    src, src_src, ref_src = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    for line in range(6):
        for j in range(6):
            ws = wt[:, line, j] * s[:, line, j]
            src = src + ws
            src_src = fma(ws, s[:, line, j], src_src)
            ref_src = fma(ws, r[:, line, j], ref_src)
    src, src_src, ref_src = src * inv_wsum, src_src * inv_wsum, ref_src * inv_wsum
    var_src = src_src - src * src
    covar = ref_src - mean_ref * src
    with np.errstate(all="ignore"):
        vrs = np.sqrt(var_ref * var_src).astype(f32)
        cost = np.maximum(f32(0.0), np.minimum(MAXCOST, f32(1.0) - covar / vrs)).astype(f32)
    return np.where((var_ref < f32(1e-5)) | (var_src < f32(1e-5)), MAXCOST, cost).astype(f32)


def float64_window_cost(wt, r, s):
    """1 - weighted NCC of the same weights, texels and samples in float64 throughout (centred sums); NaN without variance"""
    w_, r_, s_ = (np.asarray(a, np.float64).reshape(len(wt), -1) for a in (wt, r, s))
    W = w_.sum(axis=1, keepdims=True)
    dr, ds = r_ - (w_ * r_).sum(axis=1, keepdims=True) / W, s_ - (w_ * s_).sum(axis=1, keepdims=True) / W
    with np.errstate(all="ignore"):
        return 1.0 - (w_ * dr * ds).sum(axis=1) / np.sqrt((w_ * dr * dr).sum(axis=1) * (w_ * ds * ds).sum(axis=1))


# ---- adversarial windows: synthetic box-11 windows near the rounding allowances, where natural texture never goes -------------------
REF_CLASSES = ("bright", "lowvar", "binary", "lonely", "uniform")
SRC_MODES = ("tail", "noisy", "anti", "random")
COST_NOW_STEPS = (None, 3e-5, 1e-4, 1e-3, 1e-2)        # cost_now = nextafter(c) and c + each of these


def adversarial_reference(rng, n, cls):
    """n reference windows of class cls: texels [n, row, tap along x] and the centre texel [n] (not one of the 36 taps), 8-bit values.
    bright: 246..255 (the largest sums, the smallest variances beside them).  lowvar: a base value plus 0..5, var_ref on both sides
    of the variance gate (var_ref - E_FULL >= 2 E_FULL).  binary: 0 or 255 (the largest variance; half the weights ~1e-6).  lonely: 0..39 under a centre of 255, every weight
    ~1e-6.  uniform: 0..255."""
    shape = (n, 7, 6)                                                           # the 36 taps and, in [:, 6, 0], the centre
    if cls == "bright":
        t = rng.integers(246, 256, shape)
    elif cls == "lowvar":
        t = rng.integers(0, 250, (n, 1, 1)) + rng.integers(0, 6, shape)
    elif cls == "binary":
        t = 255 * rng.integers(0, 2, shape)
    elif cls == "lonely":
        t = rng.integers(0, 40, shape)
        t[:, 6, 0] = 255
    elif cls == "uniform":
        t = rng.integers(0, 256, shape)
    else:
        raise ValueError(cls)
    return t[:, :6].astype(f32), t[:, 6, 0].astype(f32)


def adversarial_source(rng, n, mode, r, cls):
    """source samples [n, row, tap along x] for the reference windows r of class cls.  tail: the first 2 to 4 lines are an unrelated
    window of the class, the rest equals the reference (the partial window says nothing of the whole; the bound is tightest here).
    noisy: the reference plus Gaussian noise of sigma 0.2 to 3, kept in 0..255 (costs of 1e-4 .. 1e-1, fractional samples).  anti:
    the first three lines are 255 - r.  random: an unrelated window of the class."""
    other = adversarial_reference(rng, n, cls)[0]
    if mode == "tail":
        lines = rng.integers(2, 5, n)
        return np.where(np.arange(6)[None, :, None] < lines[:, None, None], other, r).astype(f32)
    if mode == "noisy":
        sigma = rng.uniform(0.2, 3.0, (n, 1, 1))
        return np.clip(r + sigma * rng.standard_normal(r.shape), 0.0, 255.0).astype(f32)
    if mode == "anti":
        return np.where(np.arange(6)[None, :, None] < 3, f32(255.0) - r, r).astype(f32)
    if mode == "random":
        return other
    raise ValueError(mode)


def cost_now_values(cost):
    """the five costs a lane is tried with: the next float above the window's cost, and the cost plus 3e-5 .. 1e-2"""
    return [np.nextafter(cost, f32(np.inf)) if d is None else (cost + f32(d)).astype(f32) for d in COST_NOW_STEPS]


def adversarial_census(cls, mode, n, rng, inv_wsum_scale=1.0):
    """n windows of (cls, mode): the fast arithmetic's cost of each whole window, and prune_proven's verdicts with cost_now just above
    it.  A proven verdict of an eligible window (var_ref >= 1e-5, cost < 1) is a false proof: the kernel would leave a view that
    scores below the lane's cost.  inv_wsum_scale mis-scales the check's inv_wsum alone (a mutation for the tests)."""
    r, cen = adversarial_reference(rng, n, cls)
    wt = window_weights(r, cen)
    inv_wsum, mean_ref, var_ref = hoisted_terms(wt, r)
    s = adversarial_source(rng, n, mode, r, cls)
    cost = full_window_cost(wt, r, s, inv_wsum, mean_ref, var_ref)
    eligible = (var_ref >= f32(1e-5)) & (cost < f32(1.0))
    check_inv = (inv_wsum * f32(inv_wsum_scale)).astype(f32)
    verdicts = np.stack([proven_after_lines(wt, r, s, check_inv, var_ref, cn) for cn in cost_now_values(cost)], axis=1)   # [n, 5, checks]
    power = proven_after_lines(wt, r, s, check_inv, var_ref, np.full(n, 0.02, f32))
    with np.errstate(all="ignore"):
        err = np.abs(cost.astype(np.float64) - float64_window_cost(wt, r, s))
    err = err[eligible & (cost > 0) & np.isfinite(err)]                         # (a cost clamped at 0 says nothing of the rounding)
    return {"n": n, "eligible": eligible, "verdicts": verdicts, "false": verdicts & eligible[:, None, None], "power": power,
            "cost": cost, "var_ref": var_ref, "max_err": float(err.max()) if err.size else 0.0}


def adversarial_main(n):
    for cls in REF_CLASSES:
        for mode in SRC_MODES:
            c = adversarial_census(cls, mode, n, np.random.default_rng(1))
            print(json.dumps({"class": cls, "mode": mode, "windows": n, "eligible": int(c["eligible"].sum()),
                              "proven_at_0.02": int(c["power"].any(axis=1).sum()), "falsely_proven": int(c["false"].sum()),
                              "verdicts": int(c["verdicts"].size), "max_abs_fp32_minus_float64": float("%.3g" % c["max_err"]),
                              "var_ref_p1": round(float(np.percentile(c["var_ref"], 1)), 2)}), flush=True)


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
    ap.add_argument("--adversarial", action="store_true", help="the synthetic window classes instead of a scene: one line per (class, mode)")
    ap.add_argument("--windows", type=int, default=20000, help="windows per (class, mode) with --adversarial")
    args = ap.parse_args()
    if args.adversarial:
        return adversarial_main(args.windows)
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

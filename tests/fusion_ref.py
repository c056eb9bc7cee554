"""Depth-map fusion restated in numpy float64, from the prose of include/tsar.h (tsar_fuse) and the header of
oracle/tsar_oracle_fusion.c — not from either loop — and the comparison that holds a fuser (the CPU oracle's orc_fuse, the GPU's
tsar_fuse) to it.  Shared by tests/test_fusion_cpu.py and tests/test_gpu_fusion_edges.py.

What fusion computes, for every pixel (c, r) of every view i whose depth is positive:
  unproject    X = R_i^T (depth K_i^-1 (c, r, 1) - t_i)
  and for every entry j of view i's source list
  project      (sx, sy, sd) = K_j (R_j X + t_j), dehomogenised; the entry is dropped when sd <= 0
  nearest pixel (sc, sr) = (floor(sx + 1/2), floor(sy + 1/2)); dropped when outside the image or when view j has no depth there
  back-project Y = view j's own point at (sc, sr), projected into view i: (bx, by, bd)
  three tests  |(c, r) - (bx, by)| < reproj_error,  |bd - depth| / depth < depth_diff,  n_i(c, r) . n_j(sc, sr) >= cos(angle)
  the pixel is kept when at least num_consistent entries pass all three; its record is the mean of X and the agreeing Y (position),
  of the normals (renormalised) and of the grays, the number of agreeing entries, and i.
With used_list = 0 the views do not influence each other, which is the case restated here.

A float32 fuser may decide an entry differently where a decision lies within rounding of its threshold, so pixels with ANY decision
inside a margin of its threshold are left out of the comparison (and their share is bounded by the caller)."""
import numpy as np

# the margins are multiples of this triple: pixels (nearest-pixel rounding, reprojection error), relative depth, cosine
MARGIN_UNIT = (1e-3, 1e-5, 1e-4)
# Measured against orc_fuse on make_inputs(173, 61) and make_inputs(333, 251), num_consistent 1, 2, 3: the smallest margin at which
# every remaining pixel agrees is 0.0048 units at 173 x 61 (5 pixels of 40 083 inside it) and 0.0208 units at 333 x 251 (76 of
# 317 615): 2.1e-5 px, about one float32 step of a pixel coordinate near 300.  Times 10 for the GPU's differently scheduled float32:
MARGIN_SCALE = 0.21          # 2.1e-4 px, 2.1e-6 relative depth, 2.1e-5 cosine; leaves out 0.23 % of the candidate pixels
EXCLUDED_CAP = 0.03
# the largest deviation of an agreeing record from the float64 means, same runs: position 1.75e-7 of the scene's coordinate scale,
# normal 1.4e-7, gray 4.0e-8 of 255.  Times 4:
RECORD_TOL = 7e-7


def make_inputs(w, h, seed=1):
    """4 views of the analytic scene with what makes every rejection bite: 0.4 % depth noise against the 1 % depth test, 5 % holes,
    normals perturbed by sigma = 0.12 per component against the 15 degree test, and a baseline wide enough for the image border to
    matter.  Source lists: uneven, one empty, one holding the view itself and a duplicate, view 3 listed by nobody."""
    from tsar_mvs_amd import synth
    sc = synth.make_scene(w, h, 3, seed=8, all_gt=True, step=0.12)
    n = len(sc.images)
    rng = np.random.default_rng(seed)
    depths, normals = [], []
    for v, (d, nc) in enumerate(sc.meta["gt_all"]):
        d = d.numpy() * (1 + rng.normal(0, 0.004, d.shape).astype(np.float32))
        d[rng.uniform(size=d.shape) < 0.05] = 0
        nw = (nc.numpy() @ sc.R[v]).astype(np.float32)                      # n_w = R^T n_c
        nw = nw + rng.normal(0, 0.12, nw.shape).astype(np.float32)
        nw /= np.linalg.norm(nw, axis=-1, keepdims=True)
        depths.append(np.ascontiguousarray(d, np.float32))
        normals.append(np.ascontiguousarray(nw, np.float32))
    grays = [im.numpy() for im in sc.images]
    pairs = {0: [1, 2], 1: [0, 2, 1, 2], 2: [], 3: [0, 1, 2]}
    assert all(3 not in p for p in pairs.values()) and n == 4
    return dict(w=w, h=h, n=n, depths=depths, normals=normals, grays=grays, K=sc.K, R=sc.R, t=sc.t, pairs=pairs)


def _unproject(K, R, t, x, y, depth):
    pc = np.stack([depth * (x - K[0, 2]) / K[0, 0], depth * (y - K[1, 2]) / K[1, 1], depth], -1)
    return (pc - t) @ R                                                     # R^T (pc - t), row vectors


def _project(K, R, t, X):
    pc = X @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        return K[0, 0] * pc[..., 0] / pc[..., 2] + K[0, 2], K[1, 1] * pc[..., 1] / pc[..., 2] + K[1, 2], pc[..., 2]


def restate_view(inp, i, reproj_error=2.0, depth_diff=0.01, angle_deg=15.0):
    """view i against its source list, used_list = 0, in float64.  -> dict over the candidate pixels (depth > 0) of view i:
    pix [m] raster index; ncons [m]; pos [m, 3], nrm [m, 3], gray [m] the record's means; near [m, 3] the smallest distance of any
    of the pixel's decisions to its threshold (pixels, relative depth, cosine); and the four rejection counts over (pixel, entry)
    pairs: out of the image, no source depth, depth test, angle test, with the number of pairs."""
    w, h = inp["w"], inp["h"]
    K, R, t = (np.asarray(inp[k], np.float64) for k in ("K", "R", "t"))
    cos_angle = np.cos(np.float64(np.float32(angle_deg)) * np.pi / 180.0)
    d_i = inp["depths"][i].astype(np.float64).ravel()
    pix = np.nonzero(d_i > 0)[0]
    c, r = (pix % w).astype(np.float64), (pix // w).astype(np.float64)
    depth = d_i[pix]
    n_i = inp["normals"][i].astype(np.float64).reshape(-1, 3)[pix]
    X = _unproject(K[i], R[i], t[i], c, r, depth)
    acc, nacc, gacc = X.copy(), n_i.copy(), inp["grays"][i].astype(np.float64).ravel()[pix].copy()
    ncons = np.zeros(len(pix), np.int64)
    near = np.full((len(pix), 3), np.inf)
    rej = dict(pairs=0, outside=0, no_depth=0, depth=0, angle=0)
    for j in list(inp["pairs"][i])[:64]:
        rej["pairs"] += len(pix)
        sx, sy, sd = _project(K[j], R[j], t[j], X)
        front = sd > 0
        fx, fy = np.floor(sx + 0.5), np.floor(sy + 0.5)
        # how far the rounding is from picking the neighbouring pixel
        rnd = np.minimum(0.5 - np.abs(sx - fx), 0.5 - np.abs(sy - fy))
        near[front, 0] = np.minimum(near[front, 0], rnd[front])
        inside = front & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
        rej["outside"] += int((~inside).sum())
        q = np.where(inside, fy * w + fx, 0).astype(np.int64)
        d_j = inp["depths"][j].astype(np.float64).ravel()[q]
        have = inside & (d_j > 0)
        rej["no_depth"] += int((inside & ~have).sum())
        Y = _unproject(K[j], R[j], t[j], fx, fy, np.where(have, d_j, 1.0))
        bx, by, bd = _project(K[i], R[i], t[i], Y)
        err = np.hypot(c - bx, r - by)
        rel = np.abs(bd - depth) / depth
        n_j = inp["normals"][j].astype(np.float64).reshape(-1, 3)[q]
        cosang = np.einsum("ij,ij->i", n_i, n_j)
        near[have, 0] = np.minimum(near[have, 0], np.abs(err - reproj_error)[have])
        near[have, 1] = np.minimum(near[have, 1], np.abs(rel - depth_diff)[have])
        near[have, 2] = np.minimum(near[have, 2], np.abs(cosang - cos_angle)[have])
        rej["depth"] += int((have & ~(rel < depth_diff)).sum())
        rej["angle"] += int((have & ~(cosang >= cos_angle)).sum())
        ok = have & (err < reproj_error) & (rel < depth_diff) & (cosang >= cos_angle)
        acc[ok] += Y[ok]
        nacc[ok] += n_j[ok]
        gacc[ok] += inp["grays"][j].astype(np.float64).ravel()[q][ok]
        ncons += ok
    inv = 1.0 / (ncons + 1.0)
    nn = nacc * inv[:, None]
    return dict(pix=pix, ncons=ncons, pos=acc * inv[:, None], nrm=nn / np.linalg.norm(nn, axis=1, keepdims=True), gray=gacc * inv,
                near=near, rej=rej)


def identify_pixels(fuse_fn, inp, num_consistent):
    """which pixel is each record of fuse_fn's output?  The fuser runs twice more per view: with that view's gray image replaced
    by ones, then by its pixel indices, every other gray zero.  The first record's gray is m / (agreeing entries + 1), m = 1 + the
    agreeing entries that are the view itself; the second's is m index / (agreeing entries + 1), which a float32 holds to a
    hundredth for the image sizes used (indices below 2^17).  fuse_fn(depths, normals, grays, num_consistent) -> [m, 9] records
    with used_list = 0.  -> list over views of the kept pixels' raster indices, in record order."""
    w, h, n = inp["w"], inp["h"], inp["n"]
    assert w * h < (1 << 17)
    idx = np.arange(w * h, dtype=np.float32).reshape(h, w)
    one = np.ones((h, w), np.float32)
    zero = np.zeros((h, w), np.float32)
    out = []
    for i in range(n):
        recs = []
        for mine in (one, idx):
            rec = fuse_fn(inp["depths"], inp["normals"], [mine if v == i else zero for v in range(n)], num_consistent)
            recs.append(rec[rec[:, 8] == i].astype(np.float64))
        m = recs[0][:, 6] * (recs[0][:, 7] + 1.0)
        assert np.all(np.abs(m - np.rint(m)) < 1e-3) and np.all(np.rint(m) >= 1)
        g = recs[1][:, 6] * (recs[1][:, 7] + 1.0) / np.rint(m)
        p = np.rint(g).astype(np.int64)
        assert np.all(np.abs(g - p) < 0.05)
        out.append(p)
    return out


def compare(fuse_fn, inp, num_consistent, margin_scale, pos_tol, reproj_error=2.0):
    """hold fuse_fn (used_list = 0) to the restatement.  Pixels whose nearest decision lies within margin_scale * MARGIN_UNIT of its
    threshold are left out.  Asserts: the same (view, pixel) pairs kept, the same agreeing-view count, position / normal / gray
    within pos_tol (relative to the coordinate scale, absolute for the unit normal, relative to 255 for gray); every record
    projects into its view within reproj_error of its pixel.  -> dict(excluded share, candidates, the largest deviations among the
    agreeing pixels, and `needed`: the smallest margin_scale at which nothing would disagree; margin_scale = inf measures it)."""
    w, h, n = inp["w"], inp["h"], inp["n"]
    K, R, t = (np.asarray(inp[k], np.float64) for k in ("K", "R", "t"))
    rec_all = fuse_fn(inp["depths"], inp["normals"], inp["grays"], num_consistent)
    kept_pix = identify_pixels(fuse_fn, inp, num_consistent)
    unit = np.asarray(MARGIN_UNIT)
    stats = dict(candidates=0, excluded=0, compared_kept=0, needed=0.0, dpos=0.0, dnrm=0.0, dgray=0.0)
    for i in range(n):
        ref = inp.setdefault("_restated", {}).get((i, reproj_error))                   # (does not depend on num_consistent)
        if ref is None:
            ref = inp["_restated"][(i, reproj_error)] = restate_view(inp, i, reproj_error=reproj_error)
        rec = rec_all[rec_all[:, 8] == i]
        assert len(rec) == len(kept_pix[i]), (i, len(rec), len(kept_pix[i]))
        assert np.all(np.diff(kept_pix[i]) > 0)                                          # raster order, no pixel twice
        # the record lies where its pixel looks: it projects into view i within the reprojection bound of that pixel
        bx, by, _ = _project(K[i], R[i], t[i], rec[:, :3].astype(np.float64))
        assert np.all(np.hypot(bx - kept_pix[i] % w, by - kept_pix[i] // w) < reproj_error)
        got_keep = np.zeros(w * h, bool)
        got_keep[kept_pix[i]] = True
        row = np.full(w * h, -1)
        row[kept_pix[i]] = np.arange(len(rec))
        assert got_keep[ref["pix"]].sum() == len(rec)                                    # only pixels with a depth are ever kept
        want_keep = ref["ncons"] >= num_consistent
        scaled = (ref["near"] / unit).min(axis=1)                                        # nearest decision in units of the margin triple
        sure = scaled >= margin_scale
        stats["candidates"] += len(ref["pix"])
        stats["excluded"] += int((~sure).sum())
        g_keep = got_keep[ref["pix"]]
        g_ncons = np.append(rec[:, 7], -1.0)[row[ref["pix"]]].astype(np.int64)             # (-1: not kept)
        both = g_keep & want_keep
        r_ = np.vstack([rec, np.zeros((1, 9), rec.dtype)])[row[ref["pix"]]].astype(np.float64)
        scale = max(1.0, float(np.abs(ref["pos"]).max()))
        dpos = np.where(both, np.abs(r_[:, :3] - ref["pos"]).max(axis=1) / scale, 0.0)
        dnrm = np.where(both, np.abs(r_[:, 3:6] - ref["nrm"]).max(axis=1), 0.0)
        dgray = np.where(both, np.abs(r_[:, 6] - ref["gray"]) / 255.0, 0.0)
        # a pixel differs when it is kept on one side only, with another count, or (another source pixel chosen at a rounding tie:
        # same count, other points) with a record off by more than the tolerance
        differs = (g_keep != want_keep) | (both & (g_ncons != ref["ncons"])) | (np.maximum(np.maximum(dpos, dnrm), dgray) > pos_tol)
        if differs.any():
            stats["needed"] = max(stats["needed"], float(scaled[differs].max()))
        assert not (differs & sure).any(), (i, int((differs & sure).sum()), float(scaled[differs & sure].max()), float(dpos[sure].max()),
                                             float(dnrm[sure].max()), float(dgray[sure].max()))
        ok = sure & both & ~differs
        stats["compared_kept"] += int((sure & both).sum())
        for k, d in (("dpos", dpos), ("dnrm", dnrm), ("dgray", dgray)):
            stats[k] = max(stats[k], float(d[ok].max(initial=0.0)))
    stats["excluded_share"] = stats["excluded"] / max(1, stats["candidates"])
    return stats

"""Inputs that take the SLIC kernels (slic_kernels.hip; oracle tsar_oracle_slic.c) to every size class of the centre update's window and
to the image edges, and a PLAIN STATEMENT of what each stage computes.  Shared by the CPU test (oracle against the plain statement,
test_slic_edges_cpu.py) and the GPU test (kernels against both, test_gpu_slic_edges.py).  No test functions here.

What the centre update sums (Update_Cluster_Center_device, GPU.cu:260-357).  With nblk = ceil(9 S^2 / 256) (in float32, as the code
computes it) and bpl = max(3S / 16, 1), pixel (xo, yo) of the window of superpixel (sx, sy) is visited if and only if
    xo < 3S and yo < 3S,    xo / 16 < bpl,    (yo / 16) bpl + xo / 16 < nblk
and the image pixel is (sx S - S + xo, sy S - S + yo): inside the image, carrying label id.  Not a rectangle — size_class() below:
    clamped   S = 4, 5: 3S / 16 is 0, clamped to 1 (the reference would divide by zero); the whole window is visited
    truncated 235 of the 253 sizes S = 4..256 (all but 4, 5 and the multiples of 16): columns >= 16 bpl are never visited; at S = 9, 10
              not even the superpixel's own cell is covered (2S > 16 bpl): a superpixel with sx >= 1 can own pixels and end with n = 0
    ragged    103 of those (S = 11, 17, 22, 23, 27, 28, 33, ...): the last block row is visited in its first few blocks only
    exact     S = 4, 5 and the multiples of 16
plain_update() states this one superpixel at a time as a mask over the window — no block loop, no reduction tree — sums in int64 /
float64 and divides once in float32.  Where every sum is an integer below 2^24 (RGB space, these shapes: asserted) every float32
partial sum of ANY summation order is exact, so kernel and oracle must equal it bit for bit.  For float inputs (CIELAB, XYZ) and for
S = 256 plain_update_bound() gives the float64 means and a derived bound instead.

The association (find_center_association_shared, shared.h:106-134) is stated by plain_assoc_check() in float64.

A case is a dict: tag, S, w, h, mw, mh, weight, bgra [h, w, 4] uint8."""
import numpy as np

import oracle_lib as ol

SPIXEL_DTYPE = ol.SPIXEL_DTYPE
U = 2.0 ** -24                 # unit roundoff of float32
WEIGHT = 5.0
MARGIN_SHARE_CAP = 0.01


# ---- the visited set ---------------------------------------------------------------------------------------------------------------
def grid_of(S):
    """(nblk, bpl) as the code computes them"""
    nblk = int(np.ceil(np.float32(S * S * 9) / np.float32(256.0)))
    return nblk, max(S * 3 // 16, 1)


def visited(S):
    """[3S, 3S] bool, indexed [yo, xo]: the window pixels the centre update visits"""
    nblk, bpl = grid_of(S)
    yo, xo = np.mgrid[0:3 * S, 0:3 * S]
    return (xo // 16 < bpl) & ((yo // 16) * bpl + xo // 16 < nblk)


def size_class(S):
    """the set of {"clamped", "truncated", "ragged", "own_cell_cut", "exact"} that S belongs to, counted from visited(S)"""
    v = visited(S)
    out = set()
    if S * 3 // 16 < 1:
        out.add("clamped")
    cols = v.any(axis=0)
    if not cols.all():
        out.add("truncated")                                    # a window column no row visits
    if not v[:, cols].all():
        out.add("ragged")                                       # a row that leaves out a column other rows visit
    if not v[S:2 * S, S:2 * S].all():
        out.add("own_cell_cut")
    if v.all():
        out.add("exact")
    return out


def _window(sx, sy, S, w, h):
    """the part of superpixel (sx, sy)'s window inside the image: image slices and the matching slices of visited(S)"""
    x0, y0 = sx * S - S, sy * S - S
    xa, xb, ya, yb = max(x0, 0), min(x0 + 3 * S, w), max(y0, 0), min(y0 + 3 * S, h)
    return (slice(ya, yb), slice(xa, xb)), (slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))


def _sums(lab, labels, S):
    """per superpixel: n (int64), the float64 sums of x, y and the four channels [nc, 6], and the sums of their magnitudes"""
    lab = np.asarray(lab, np.float32)
    labels = np.asarray(labels)
    h, w = labels.shape
    mw, mh = w // S, h // S
    v = visited(S)
    yy, xx = np.mgrid[0:h, 0:w]
    n = np.zeros(mw * mh, np.int64)
    s = np.zeros((mw * mh, 6), np.float64)
    sabs = np.zeros((mw * mh, 6), np.float64)
    for sy in range(mh):
        for sx in range(mw):
            i = sy * mw + sx
            img, win = _window(sx, sy, S, w, h)
            take = v[win] & (labels[img] == i)
            n[i] = int(take.sum())
            vals = np.concatenate([xx[img][take][:, None], yy[img][take][:, None], lab[img][take]], axis=1).astype(np.float64)
            s[i] = vals.sum(axis=0)
            sabs[i] = np.abs(vals).sum(axis=0)
    return n, s, sabs


def _records(n, mean):
    out = np.zeros(len(n), SPIXEL_DTYPE)
    out["center"] = mean[:, :2]
    out["color"] = mean[:, 2:]
    out["id"] = np.arange(len(n))
    out["n"] = n
    return out


def plain_update(lab, labels, S):
    """the centres after one update, as SPIXEL_DTYPE records.  Only for inputs on which float32 summation is exact in any order:
    integer values whose sums all stay below 2^24 (asserted: a condition on the inputs, not a tolerance)."""
    lab = np.asarray(lab, np.float32)
    assert np.array_equal(lab, np.rint(lab)), "plain_update is for integer-valued images (RGB space)"
    n, s, sabs = _sums(lab, labels, S)
    assert sabs.max(initial=0.0) < 2 ** 24, "a sum reaches 2^24: float32 partial sums are no longer exact (use plain_update_bound)"
    mean = np.zeros((len(n), 6), np.float32)
    own = n != 0                                                # an empty superpixel keeps its zero sums: centre (0, 0), colour 0
    mean[own] = s[own].astype(np.float32) / n[own].astype(np.float32)[:, None]
    return _records(n, mean)


def plain_update_bound(lab, labels, S):
    """(n [nc] int64, mean [nc, 6] float64, bound [nc, 6] float64): the components are cx, cy, colour 0..3.
    Derivation of the bound.  The inputs (float32 pixel values, integer coordinates < 2^24) are exact.  A component's sum passes, per
    addend, through at most 8 additions of the block's reduction tree and nblk additions of the block sums, and the result through one
    division: k = nblk + 9 roundings, each (1 + d), |d| <= u = 2^-24.  Hence |got - mean| <= g_k sum|v| / n, g_k = k u / (1 - k u)
    (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  Counts are integers: exact."""
    nblk, _ = grid_of(S)
    k = nblk + 9
    gamma = k * U / (1.0 - k * U)
    n, s, sabs = _sums(lab, labels, S)
    mean = np.zeros_like(s)
    bound = np.zeros_like(s)
    own = n != 0
    mean[own] = s[own] / n[own][:, None]
    bound[own] = gamma * sabs[own] / n[own][:, None]
    return n, mean, bound


def within_bound(got, lab, labels, S):
    """-> (ok, largest |got - mean| / bound over the components with a non-zero bound).  Counts and ids must be exact, a component
    whose bound is 0 (an empty superpixel, the alpha channel) must be exactly the mean."""
    n, mean, bound = plain_update_bound(lab, labels, S)
    g = np.concatenate([got["center"], got["color"]], axis=1).astype(np.float64)
    err = np.abs(g - mean)
    ok = np.array_equal(got["n"], n) and np.array_equal(got["id"], np.arange(len(n))) and bool((err <= bound).all())
    nz = bound > 0
    return ok, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def prefilled_centres(nc):
    """records to hand an update as its output array: every float a large finite value, every count 12345 — an update that left an
    empty superpixel's record as it was would show"""
    out = np.zeros(nc, SPIXEL_DTYPE)
    out["center"], out["color"], out["n"] = 777.0, -555.0, 12345
    out["id"] = np.arange(nc)
    return out


def oracle_update(lab, labels, S):
    """orc_slic_update_centers into prefilled records (ol.slic_update_centers hands it zeros)"""
    lab = np.ascontiguousarray(lab, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    h, w = labels.shape
    out = prefilled_centres((w // S) * (h // S))
    ol.lib().orc_slic_update_centers(lab.ctypes.data, labels.ctypes.data, out.ctypes.data, w, h, w // S, h // S, S)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_centres(a, b):
    """every field of the records, floats by their bits"""
    return (np.array_equal(bits(a["center"]), bits(b["center"])) and np.array_equal(bits(a["color"]), bits(b["color"]))
            and np.array_equal(a["id"], b["id"]) and np.array_equal(a["n"], b["n"]))


def empty_records_ok(c):
    """the records with n == 0 are centre (0, 0), colour (0, 0, 0, 0), id kept"""
    e = c["n"] == 0
    return bool((c["center"][e] == 0).all() and (c["color"][e] == 0).all() and np.array_equal(c["id"], np.arange(len(c))))


# ---- the association ---------------------------------------------------------------------------------------------------------------
ASSOC_REL = 4 * U


def plain_assoc_check(lab, centres, labels, mw, mh, S, weight):
    """-> (ok, share, detail).  For every pixel: the chosen id is one of its valid candidates — the <= 9 centres around (x / S, y / S)
    inside the centre map; the chosen centre's float64 distance is within ASSOC_REL (relative) of the float64 minimum over the
    candidates; and where the runner-up's float64 distance exceeds the minimum by more than ASSOC_REL (relative), the label IS the
    float64 argmin.  share = the pixels on which only the second rule decides (margin within the bound: exact ties among them, where
    the first candidate in scan order wins — the known answers of this file check that rule, not this function).

    The bound.  compute_slic_distance (shared.h:92-104) forms sqrt(dc^2 + (dxy nxy weight)^2) with dc = sqrt(d0^2 + d1^2 + d2^2), dxy =
    sqrt(ex^2 + ey^2), nxy = 1.0f / S: three square roots.  A square root halves the relative error that enters it and adds one
    rounding, so of the ~6 roundings on the longer path into each of dc and dxy about 3 u survive each root, squaring doubles them and
    the last root halves them again: the worst case of one distance is 7 u to first order (colour path: 5 roundings into the sum, root
    -> 3.5 u, squared with its rounding -> 8 u; spatial path: 4 into the sum, root -> 3 u, two products -> 5 u, squared -> 11 u; the
    sum's rounding, halved by the last root, plus its own: <= 7 u), with roundings of both signs a distance is typically within 1-2 u.
    The check asks 4 u of the DIFFERENCE of two distances, which is tighter than that worst case twice over would allow: it holds on the
    oracle on every case here (test_slic_edges_cpu.py asserts it) and is therefore asked of the kernel on the same inputs."""
    lab = np.asarray(lab, np.float64)
    labels = np.asarray(labels)
    h, w = labels.shape
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = xx // S, yy // S
    nxy = float(np.float32(1.0) / np.float32(S))
    cen = np.asarray(centres["center"], np.float64)
    col = np.asarray(centres["color"], np.float64)
    ids = np.asarray(centres["id"])
    dist = np.full((9, h, w), np.inf)
    cand = np.full((9, h, w), -1, np.int64)
    k = 0
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            px, py = cx + j, cy + i
            valid = (px >= 0) & (py >= 0) & (px < mw) & (py < mh)
            c = np.where(valid, py * mw + px, 0)
            dc2 = ((lab[..., :3] - col[c][..., :3]) ** 2).sum(-1)
            dxy2 = (xx - cen[c][..., 0]) ** 2 + (yy - cen[c][..., 1]) ** 2
            d = np.sqrt(dc2 + dxy2 * (nxy * float(np.float32(weight))) ** 2)
            dist[k][valid] = d[valid]
            cand[k][valid] = ids[c][valid]
            k += 1
    dmin = dist.min(axis=0)
    amin = np.take_along_axis(cand, dist.argmin(axis=0)[None], 0)[0]
    chosen = cand == labels[None]
    is_candidate = chosen.any(axis=0)
    dchosen = np.where(chosen, dist, np.inf).min(axis=0)
    tol = ASSOC_REL * dmin
    near = dchosen <= dmin + tol
    others = np.where(cand == amin[None], np.inf, dist)          # the runner-up: the nearest candidate of another id
    clear = others.min(axis=0) > dmin + tol
    right = ~clear | (labels == amin)
    ok = bool(is_candidate.all() and near.all() and right.all())
    detail = dict(not_a_candidate=int((~is_candidate).sum()), too_far=int((is_candidate & ~near).sum()), wrong=int((~right).sum()))
    return ok, float((~clear).mean()), detail


def plain_connectivity(labels):
    """supress_local_lable (shared.h:175-204) pixel by pixel: a pixel within 2 of the border keeps its label; elsewhere, if at least 16
    of the 25 labels around it differ from its own, it takes the last differing one in scan order (rows outer)"""
    labels = np.asarray(labels, np.int32)
    h, w = labels.shape
    out = labels.copy()
    for y in range(2, h - 2):
        for x in range(2, w - 2):
            nb = labels[y - 2:y + 3, x - 2:x + 3].ravel()
            diff = nb[nb != labels[y, x]]
            if len(diff) >= 16:
                out[y, x] = diff[-1]
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _rule(S):
    return 3 * S + S // 2 + 1, 3 * S - 1


# tag -> (S, w, h): the smallest shapes at which each edge still exists
TABLE = {
    "clamp4": (4, 15, 11), "clamp5": (5, 18, 14),                          # bpl clamp, remainder stripes on both axes
    "own-cell-cut-9": (9, 32, 26), "own-cell-cut-10": (10, 36, 29),        # 2S > 16 bpl
    **{"ragged-%d" % S: (S,) + _rule(S) for S in (11, 17, 22, 27)},        # ragged last block row
    **{"trunc-%d" % S: (S,) + _rule(S) for S in (6, 21)},                  # right columns cut
    **{"exact-%d" % S: (S,) + _rule(S) for S in (16, 48)},                 # clean control
    "one-centre": (20, 39, 20),                                            # mw == mh == 1, stripe S - 1 wide, h == S
    "one-row": (12, 61, 23),                                               # mh == 1
    "big": (256, 300, 256),                                                # mw = mh = 1, nblk = 2304
}
TAGS = tuple(TABLE)
EXACT_TAGS = tuple(t for t in TAGS if t != "big")                          # RGB sums below 2^24: plain_update applies
EXPECTED_CLASS = {"clamp4": {"clamped", "exact"}, "clamp5": {"clamped", "exact"},
                  "own-cell-cut-9": {"truncated", "own_cell_cut"}, "own-cell-cut-10": {"truncated", "own_cell_cut"},
                  "ragged-11": {"truncated", "ragged"}, "ragged-17": {"truncated", "ragged"}, "ragged-22": {"truncated", "ragged"},
                  "ragged-27": {"truncated", "ragged"}, "trunc-6": {"truncated"}, "trunc-21": {"truncated"},
                  "exact-16": {"exact"}, "exact-48": {"exact"}, "one-centre": {"truncated"}, "one-row": {"truncated"}, "big": {"exact"}}


def noise_bgra(w, h, seed):
    """seeded rng.integers(0, 256) noise averaged with the low-frequency terms of the golden generator's synth_bgra"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    low = np.stack([127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0), (xx * 3 + yy * 2) % 256,
                    100.0 * ((xx // 40 + yy // 30) % 2) + 15], axis=-1)
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = ((rng.integers(0, 256, size=(h, w, 3)) + low) / 2).astype(np.uint8)
    img[..., 3] = 255
    return img


_cache = {}


def case(tag):
    """the case `tag`, built once per process"""
    if tag not in _cache:
        S, w, h = TABLE[tag]
        _cache[tag] = dict(tag=tag, S=S, w=w, h=h, mw=w // S, mh=h // S, weight=WEIGHT, bgra=noise_bgra(w, h, 1000 + S))
    return _cache[tag]


def random_labels(c, seed=5):
    return np.random.default_rng(seed + c["S"]).integers(0, c["mw"] * c["mh"], size=(c["h"], c["w"])).astype(np.int32)


def stray_labels(c, labels):
    """labels with values no centre may sum: negative ones, ones >= mw mh, and — where the centre map is wide enough for a pixel to
    lie outside a window — id 0 placed ONLY outside its own window (x >= 2S).  -> (labels, ids that must end empty)"""
    rng = np.random.default_rng(9 + c["S"])
    out = np.array(labels, np.int32)
    u = rng.random(out.shape)
    nc = c["mw"] * c["mh"]
    out[u < 0.05] = -1
    out[(u >= 0.05) & (u < 0.08)] = np.iinfo(np.int32).min
    out[(u >= 0.08) & (u < 0.13)] = nc
    out[(u >= 0.13) & (u < 0.16)] = np.iinfo(np.int32).max
    empty = []
    if c["w"] > 2 * c["S"] and nc > 1:
        out[out == 0] = 1
        out[:, 2 * c["S"]:][u[:, 2 * c["S"]:] > 0.7] = 0
        assert (out[:, 2 * c["S"]:] == 0).any() and not (out[:, :2 * c["S"]] == 0).any()
        empty.append(0)
    return out, empty


def cut_census(labels, S):
    """how many pixels carry the id of a superpixel whose 3S x 3S window holds them and whose update does not visit them: (in a
    column no row visits, in a visited column of the ragged last block row, of those inside the superpixel's own cell)"""
    labels = np.asarray(labels)
    h, w = labels.shape
    mw, mh = w // S, h // S
    v = visited(S)
    cols = v.any(axis=0)
    right = ragged = own = 0
    for sy in range(mh):
        for sx in range(mw):
            img, win = _window(sx, sy, S, w, h)
            mine = labels[img] == sy * mw + sx
            right += int((mine & ~cols[win[1]][None, :]).sum())
            ragged += int((mine & ~v[win] & cols[win[1]][None, :]).sum())
            cell = np.zeros((3 * S, 3 * S), bool)
            cell[S:2 * S, S:2 * S] = True
            own += int((mine & ~v[win] & cell[win]).sum())
    return right, ragged, own


# ---- known answers -----------------------------------------------------------------------------------------------------------------
CONSTANT = (90, 140, 200)
# (S, mw, mh, remainder on both axes) -> superpixels the oracle leaves with n == 0 after an update of the weight-0 labels
WEIGHT0 = {(4, 3, 3, 0): 5, (9, 3, 2, 0): 5, (20, 3, 2, 0): 4, (9, 3, 2, 5): 4}


def constant_bgra(w, h):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = CONSTANT
    img[..., 3] = 255
    return img


def weight0_case(key):
    """a constant image in RGB space with coh_weight 0: every candidate ties at distance 0 and the first in scan order wins, whatever
    the number of iterations: label = min(max(y / S - 1, 0), mh - 1) mw + min(max(x / S - 1, 0), mw - 1)"""
    S, mw, mh, rem = key
    w, h = mw * S + rem, mh * S + rem
    yy, xx = np.mgrid[0:h, 0:w]
    want = np.minimum(np.maximum(yy // S - 1, 0), mh - 1) * mw + np.minimum(np.maximum(xx // S - 1, 0), mw - 1)
    return dict(tag="weight0-%d-%dx%d+%d" % key, S=S, w=w, h=h, mw=mw, mh=mh, weight=0.0, bgra=constant_bgra(w, h),
                labels=want.astype(np.int32), n_empty=WEIGHT0[key])


def tie_case():
    """S = 4, 12 x 4, constant colour, weight 5, no iterations: pixels x = 4 and x = 8 lie at distance exactly 2 from two centres
    (x = 2, 6, 10; y = 2) and the earlier one wins"""
    row = [0] * 5 + [1] * 4 + [2] * 3
    return dict(tag="tie", S=4, w=12, h=4, mw=3, mh=1, weight=5.0, bgra=constant_bgra(12, 4), labels=np.array([row] * 4, np.int32))


def threshold_images():
    """-> ((9 x 9 labels, expected label of the centre pixel) for 15 and for 16 differing labels around (4, 4)).  Background and
    centre are 7; the differing labels are 2 (first in scan order), 1 (most frequent) and 3 (last in scan order)."""
    out = []
    for count in (15, 16):
        lb = np.full((9, 9), 7, np.int32)
        cells = [(x, y) for y in range(2, 7) for x in range(2, 7) if (x, y) != (4, 4)]
        for x, y in cells[:count - 1]:
            lb[y, x] = 1
        lb[2, 2] = 2
        lb[6, 6] = 3
        nb = lb[2:7, 2:7]
        assert int((nb != 7).sum()) == count and set(np.unique(nb[nb != 7])) == {1, 2, 3}
        out.append((lb, 7 if count == 15 else 3))
    return out


def all_border_images():
    """4 x 4 and 4 x 9: every pixel is within 2 of the border; 5 x 5: every pixel but (2, 2), whose 24 neighbours all differ"""
    rng = np.random.default_rng(77)
    out = [rng.integers(0, 4, size=(4, 4)).astype(np.int32), rng.integers(0, 4, size=(9, 4)).astype(np.int32)]
    lb = rng.integers(0, 4, size=(5, 5)).astype(np.int32)
    lb[2, 2] = 9
    out.append(lb)
    return out

"""Inputs that take the weighted median filter (wmf_kernels.hip; oracle orc_wmf_detect / orc_wmf_fill) to the edges that a random
70-85 % reliability mask over a PatchMatch state never reaches: fill passes 4-6, a full window (121 reliable taps), a nearly empty one
(1, 2, 3 taps, where the zero slot of SURVEY quirk 12 decides the result), lists full of ties with +-0 and fp32 denormals, infinite
entries in the depth list, fill waves with one or a few active lanes, images narrower than one tap gap.  Shared by the CPU test (oracle
against the reference's text, test_wmf_edges_cpu.py) and the GPU test (kernel against oracle, test_gpu_wmf_edges.py).

A case is a dict:
    scene          synth.Scene
    planes         [h, w, 4] float32, camera frame (Matcher.set_plane / Oracle.norm4); lines->depth follows from them through getview
    mask           [h, w] float32 reliability mask (lines->scale) the FILL passes start from — and the detection passes too, unless
    detect_mask    is present: then the detection run starts from that one
    labels, region_text   the regions (a pixel is textured where region_text[labels] == 1)
    fill_passes    number of gipuma_WMF_Final passes to run
    fill_from      where the fill passes start: "detect" = from what the four detection passes left, "mask" = from `mask` again (a
                   constructed mask would not survive detection, which rewrites every pixel's reliability; and detection finds a
                   piecewise-constant state reliable everywhere, which leaves the fill passes nothing to do); both: two runs
    islands / targets     the pixels the case is about (six_passes / sparse), see there

tap_count() says, from the mask alone, how many reliable taps a pixel's window holds: the tests assert with it that a case reaches what
it is for, independently of oracle and kernel."""
import numpy as np

import oracle_lib as ol
from tsar_mvs_amd import synth

W, H = 416, 352
SEED = 31                      # PatchMatch seed of the shared state


def detect_grid(it):
    """(radius, gap, ths) of gipuma_WMF pass it = 0..3 (gipuma.cu:1506-1512)"""
    po = 1 << it
    return 80 // po, 16 // po, 24 // po


def fill_grid(it):
    """(radius, gap, ths) of gipuma_WMF_Final pass it = 0..5 (gipuma.cu:1301-1306)"""
    po = 1 << it
    return 5 * po, po, 32 // po


def tap_count(mask, radius, gap):
    """per pixel: the number of taps (x + i, y + j), i, j = -radius, -radius + gap, .., radius, that are inside the image and reliable
    (mask == 1) — a sum of shifted masks"""
    h, w = mask.shape
    pad = np.zeros((h + 2 * radius, w + 2 * radius), np.int32)
    pad[radius:radius + h, radius:radius + w] = mask == 1
    out = np.zeros((h, w), np.int32)
    for i in range(0, 2 * radius + 1, gap):
        for j in range(0, 2 * radius + 1, gap):
            out += pad[j:j + h, i:i + w]
    return out


def oracle_of(scene, nofma=False, seed=SEED):
    return ol.Oracle([im.cpu().numpy() for im in scene.images], scene.K, scene.R, scene.t, scene.depth_min, scene.depth_max, seed=seed, nofma=nofma)


def load_oracle(case, nofma=False, mask=None):
    """an oracle in the case's state: planes, lines->depth through getview, reliability mask, regions"""
    orc = oracle_of(case["scene"], nofma)
    orc.norm4[...] = case["planes"]
    orc.c[...] = 0
    orc.getview()
    orc.scale[...] = case["mask"] if mask is None else mask
    orc.set_regions(case["labels"], case["region_text"])
    return orc


_cache = {}


def _base(nofma):
    """the 416 x 352 two-view scene and a PatchMatch state on it (pm_init + one iteration)"""
    key = ("base", nofma)
    if key not in _cache:
        sc = synth.make_scene(W, H, 1, seed=23)
        orc = oracle_of(sc, nofma)
        orc.pm_init()
        orc.pm_iterate(1)
        _cache[key] = (sc, orc.norm4.copy())
    return _cache[key]


def _textured_everywhere(h, w):
    return np.zeros((h, w), np.int32), np.array([1.0], np.float32)


def _full(nofma):
    sc, planes = _base(nofma)
    rng = np.random.default_rng(101)
    mask = (rng.random((H, W)) >= 0.005).astype(np.float32)
    labels, text = _textured_everywhere(H, W)
    return dict(scene=sc, planes=planes.copy(), mask=mask, labels=labels, region_text=text, fill_passes=6, fill_from=("detect",))


TIES_NORMALS = ((0.0, 0.0, -1.0), (0.0, -0.6, -0.8), (0.6, 0.0, -0.8), (-0.0, 0.28, -0.96))
TIES_BLOCK = (24, 32)          # width, height of a block of constant plane


def _shift_ulps(a, k):
    for _ in range(abs(k)):
        a = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf))
    return a


def _ties(nofma):
    w, h = 96, 64
    sc = synth.make_scene(w, h, 1, seed=7)
    orc = oracle_of(sc, nofma)
    rng = np.random.default_rng(102)
    bw, bh = TIES_BLOCK
    levels = np.linspace(sc.depth_min * 1.3, sc.depth_max * 0.75, 4).astype(np.float32)
    planes = np.empty((h, w, 4), np.float32)
    target = np.empty((h, w), np.float32)
    for y in range(h):
        for x in range(w):
            bx, by = x // bw, y // bh
            n = np.array(TIES_NORMALS[(bx + by) % 4], np.float32)
            target[y, x] = levels[(bx + 2 * by) % 4]
            planes[y, x, :3] = n
            planes[y, x, 3] = orc.getD(n, x, y, float(target[y, x]))
    # the offset that getD gives puts the plane through the pixel at the block's depth only to rounding: move it by a few ulps to
    # where getDepthFromPlane3 returns the block's depth exactly, so that lines->depth (f b / depth) is constant over a block
    bad = orc.depth_from_planes(planes) != target
    d0 = planes[..., 3].copy()
    for k in (1, -1, 2, -2, 3, -3, 4, -4):
        if not bad.any():
            break
        trial = planes.copy()
        trial[..., 3][bad] = _shift_ulps(d0[bad], k)
        hit = bad & (orc.depth_from_planes(trial) == target)
        planes[..., 3][hit] = trial[..., 3][hit]
        bad &= ~hit
    # exactly-zero components: 10 % become -0, a further 10 % of the x components 1e-40f, 5 % of the y components -1e-41f (denormals)
    for c, tiny, share in ((0, np.float32(1e-40), 0.10), (1, np.float32(-1e-41), 0.05)):
        comp = planes[..., c]
        zero = comp == 0
        u = rng.random((h, w))
        comp[zero & (u < 0.10)] = np.float32(-0.0)
        comp[zero & (u >= 0.10) & (u < 0.10 + share)] = tiny
    mask = (rng.random((h, w)) < 0.85).astype(np.float32)
    labels, text = _textured_everywhere(h, w)
    return dict(scene=sc, planes=planes, mask=mask, labels=labels, region_text=text, fill_passes=3, fill_from=("detect", "mask"))


# (pass, kind, x, y) of the 4 x 4 islands' first pixel.  "inside": the pass's whole window of every island pixel lies in the image
# (the scalar-offset addressing path of the kernel, the island's four pixels of a row being the only active lanes of their wave);
# "clamped": at a border or corner.  An island of pass it >= 1 sits in a moat of half-width 5 2^(it-1) + 1 — the radius of the pass
# before, plus one — of unreliable, non-textured pixels: no earlier pass finds a reliable tap, and the moat itself is never filled.
ISLAND = 4
ISLANDS = ((0, "inside", 300, 300), (0, "clamped", 412, 100),
           (1, "inside", 200, 300), (1, "clamped", 200, 0),
           (2, "inside", 60, 300), (2, "clamped", 120, 348),
           (3, "inside", 60, 150), (3, "clamped", 0, 250),
           (4, "inside", 332, 130), (4, "clamped", 412, 300),
           (5, "inside", 206, 174), (5, "clamped", 0, 0))


def moat_half_width(it):
    return 0 if it == 0 else 5 * (1 << (it - 1)) + 1


def _six_passes(nofma):
    sc, planes = _base(nofma)
    rng = np.random.default_rng(103)
    mask = (rng.random((H, W)) < 0.90).astype(np.float32)
    labels = np.zeros((H, W), np.int32)
    covered = np.zeros((H, W), bool)
    for it, _, cx, cy in ISLANDS:
        m = moat_half_width(it)
        x0, x1, y0, y1 = max(cx - m, 0), min(cx + ISLAND + m, W), max(cy - m, 0), min(cy + ISLAND + m, H)
        assert not covered[y0:y1, x0:x1].any(), "moats overlap"
        covered[y0:y1, x0:x1] = True
        mask[y0:y1, x0:x1] = 0
        labels[y0:y1, x0:x1] = 1
        labels[cy:cy + ISLAND, cx:cx + ISLAND] = 0
    text = np.array([1.0, -1.0], np.float32)
    return dict(scene=sc, planes=planes.copy(), mask=mask, labels=labels, region_text=text, fill_passes=6, fill_from=("mask",),
                islands=ISLANDS)


# Everything unreliable and non-textured, except the targets (textured, unreliable) and single reliable pixels at offsets that only
# the tap grids of pass 4 (gap 16, radius 80) and pass 5 (gap 32, radius 160) reach.  Each group lives on its own residue modulo 16
# in x, so that no group's pixels lie on another group's grid.  (x, y, tap offsets, num at pass 4, num at pass 5 if it gets there,
# pass that rewrites the target, what the only tap is made to be)
SPARSE_TARGETS = (
    dict(x=208, y=176, taps=((64, 0),), num4=1, num5=1, at=5, tap="as it is"),                       # skipped at 4 (num = ths - 1)
    dict(x=97, y=81, taps=((48, 0), (-32, 0)), num4=2, num5=None, at=4, tap="as it is"),
    dict(x=50, y=242, taps=((48, 0), (0, -48), (48, 48)), num4=3, num5=None, at=4, tap="as it is"),
    dict(x=323, y=99, taps=((-96, 0), (0, 128)), num4=0, num5=2, at=5, tap="as it is"),
    dict(x=340, y=308, taps=((-96, 0), (0, -96), (-128, -64)), num4=0, num5=3, at=5, tap="as it is"),
    dict(x=37, y=325, taps=((64, 0),), num4=1, num5=1, at=5, tap="negative normal"),                 # all three components < 0
    dict(x=390, y=38, taps=((-64, 0),), num4=1, num5=1, at=5, tap="negative depth"),                 # [d, 0]: the tap itself is walked
)


def _sparse(nofma):
    sc, planes = _base(nofma)
    planes = planes.copy()
    orc = oracle_of(sc, nofma)
    mask = np.zeros((H, W), np.float32)
    labels = np.ones((H, W), np.int32)
    for t in SPARSE_TARGETS:
        labels[t["y"], t["x"]] = 0
        for dx, dy in t["taps"]:
            px, py = t["x"] + dx, t["y"] + dy
            mask[py, px] = 1
            depth = orc.depth_from_plane(planes[py, px], px, py)
            if t["tap"] == "negative normal":
                n = np.array([-0.3, -0.4, -np.sqrt(0.75)], np.float32)
                planes[py, px, :3] = n
                planes[py, px, 3] = orc.getD(n, px, py, depth if depth > 0 else 0.5 * (sc.depth_min + sc.depth_max))
            elif t["tap"] == "negative depth":
                planes[py, px, 3] = -planes[py, px, 3]
    rng = np.random.default_rng(104)
    detect_mask = (rng.random((H, W)) < 0.02).astype(np.float32)
    text = np.array([1.0, -1.0], np.float32)
    return dict(scene=sc, planes=planes, mask=mask, detect_mask=detect_mask, labels=labels, region_text=text, fill_passes=6,
                fill_from=("mask",), targets=SPARSE_TARGETS)


def _inf_depth(nofma):
    sc, planes = _base(nofma)
    planes = planes.copy()
    rng = np.random.default_rng(105)
    u = rng.random((H, W))
    planes[..., 3][u < 0.01] = np.float32(0.0)          # getview: depth -+0, lines->depth -+inf (no clamp in gipuma_getview)
    planes[..., 3][(u >= 0.01) & (u < 0.02)] = np.float32(-0.0)
    mask = (rng.random((H, W)) < 0.80).astype(np.float32)
    labels, text = _textured_everywhere(H, W)
    return dict(scene=sc, planes=planes, mask=mask, labels=labels, region_text=text, fill_passes=3, fill_from=("detect",))


def _tiny(w, h):
    def make(nofma):
        sc = synth.make_scene(w, h, 1, seed=9)
        orc = oracle_of(sc, nofma)
        rng = np.random.default_rng(106 + w)
        planes = np.empty((h, w, 4), np.float32)
        for y in range(h):
            for x in range(w):
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                if n @ orc.view_vector(x, y) > 0:
                    n = -n
                n = n.astype(np.float32)
                planes[y, x, :3] = n
                planes[y, x, 3] = orc.getD(n, x, y, rng.uniform(sc.depth_min, sc.depth_max))
        mask = (rng.random((h, w)) < 0.90).astype(np.float32)
        labels, text = _textured_everywhere(h, w)
        return dict(scene=sc, planes=planes, mask=mask, labels=labels, region_text=text, fill_passes=3, fill_from=("detect", "mask"))
    return make


# tiny: every window is clamped and the image is narrower than a tap gap.  tsar_set_views takes no image below 8 x 8, so 7 x 5 (35
# pixels) and 33 x 3 reach the oracle only; the kernel gets the smallest sizes of the same kind that the ABI admits: 9 x 8 (72 pixels:
# three workgroups, the last with 8 of its 32 pixels) and 33 x 8.
_MAKERS = {"full": _full, "ties": _ties, "six_passes": _six_passes, "sparse": _sparse, "inf_depth": _inf_depth,
           "tiny_9x8": _tiny(9, 8), "tiny_33x8": _tiny(33, 8), "tiny_7x5": _tiny(7, 5), "tiny_33x3": _tiny(33, 3)}
BELOW_THE_ABI = ("tiny_7x5", "tiny_33x3")
NAMES = tuple(n for n in _MAKERS if n not in BELOW_THE_ABI)


def case(name, nofma=False):
    """the case `name`, built once per process and oracle build (the PatchMatch state of the -DORC_NO_FMA oracle is its own)"""
    key = (name, nofma)
    if key not in _cache:
        c = _MAKERS[name](nofma)
        c["name"] = name
        _cache[key] = c
    return _cache[key]


# ---- the oracle's run over a case, and the conditions that make the case what it is for -------------------------------------------------
def snapshot(orc):
    return dict(scale=orc.scale.copy(), depth=orc.depth.copy(), norm4=orc.norm4.copy())


def same_bits(got, want):
    """element-wise: identical bits, or NaN on both sides (only where the oracle's element is NaN)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(want) & np.isnan(got))


def run_oracle(c, nofma=False, hook=None):
    """the four detection passes, then the fill passes from each of the case's starts.  hook(kind, it, before, orc, start) is called
    after every pass with the snapshot the pass read.  Returns
        detect_in[it]      the reliability mask pass `it` read,   detect_scale   the mask after the four passes
        lines_depth        lines->depth as getview left it
        fill[start][it]    dict(scale_in, scale, depth, norm4, disp, rewritten) after fill pass `it`
    and asserts the case's conditions (check_conditions)."""
    rec = dict(detect_in=[], fill={})
    orc = load_oracle(c, nofma, c.get("detect_mask"))
    rec["lines_depth"] = orc.depth.copy()
    for it in range(4):
        before = snapshot(orc)
        orc.wmf_detect(it)
        if hook:
            hook("detect", it, before, orc, None)
        rec["detect_in"].append(before["scale"])
    rec["detect_scale"] = orc.scale.copy()
    for start in c["fill_from"]:
        if start == "mask":
            orc = load_oracle(c, nofma)
        states = []
        for it in range(c["fill_passes"]):
            before = snapshot(orc)
            orc.wmf_fill(it)
            if hook:
                hook("fill", it, before, orc, start)
            after = snapshot(orc)
            rewritten = (after["norm4"].view(np.uint32) != before["norm4"].view(np.uint32)).any(-1) | (after["scale"] != before["scale"])
            states.append(dict(after, scale_in=before["scale"], disp=orc.compute_disp()[..., 3].copy(), rewritten=rewritten))
        rec["fill"][start] = states
    check_conditions(c, rec)
    return rec


def check_conditions(c, rec):
    name = c["name"]
    h, w = c["mask"].shape
    if name == "full":
        # a full window: 122 valid entries go through the sorting network, rank 121 is written, the last walk batch reads ranks 112..127
        for it in range(4):
            radius, gap, _ = detect_grid(it)
            assert int((tap_count(rec["detect_in"][it], radius, gap) == 121).sum()) >= 1000, it
    if name == "ties":
        assert len(np.unique(rec["lines_depth"])) <= 16
        n = c["planes"][..., :3]
        neg_zero = (n == 0) & np.signbit(n)
        denormal = (n != 0) & (np.abs(n) < np.finfo(np.float32).tiny)
        assert neg_zero[..., :2].sum() > 400 and denormal[..., 0].sum() > 100 and denormal[..., 1].sum() > 50
        # detection finds the piecewise-constant state reliable (almost) everywhere: the fill passes that write plane bits out of
        # these lists are the ones that start from the mask
        assert sum(int(s["rewritten"].sum()) for s in rec["fill"]["mask"]) >= 500
    if name == "six_passes":
        states = rec["fill"]["mask"]
        for it, kind, cx, cy in c["islands"]:
            isl = (slice(cy, cy + ISLAND), slice(cx, cx + ISLAND))
            radius = fill_grid(it)[0]
            inside = cx - radius >= 0 and cx + ISLAND - 1 + radius < w and cy - radius >= 0 and cy + ISLAND - 1 + radius < h
            assert inside == (kind == "inside"), (it, kind)
            for k in range(it):
                assert not states[k]["rewritten"][isl].any(), (it, kind, k)
            assert int(states[it]["rewritten"][isl].sum()) >= 16, (it, kind)
        for it in range(6):
            assert {kind for i, kind, _, _ in c["islands"] if i == it} == {"inside", "clamped"}
    if name == "sparse":
        states = rec["fill"]["mask"]
        num4, num5 = (tap_count(states[it]["scale_in"], *fill_grid(it)[:2]) for it in (4, 5))
        seen = set()
        for t in c["targets"]:
            x, y = t["x"], t["y"]
            assert num4[y, x] == t["num4"] and (t["num5"] is None or num5[y, x] == t["num5"]), t
            for it in range(6):
                assert bool(states[it]["rewritten"][y, x]) == (it == t["at"]), (t, it)
            seen.add((t["at"], t["num4"] if t["at"] == 4 else t["num5"]))
            if len(t["taps"]) == 1:
                px, py = x + t["taps"][0][0], y + t["taps"][0][1]
                d, n = rec["lines_depth"][py, px], c["planes"][py, px, :3]
                assert (d < 0) if t["tap"] == "negative depth" else (d > 0), t       # d > 0: sorted list [0, d], only the zero slot is walked
                if t["tap"] == "negative normal":
                    assert (n < 0).all()
        assert {(4, 2), (4, 3), (5, 1), (5, 2), (5, 3)} <= seen
        assert any(t["num4"] == fill_grid(4)[2] - 1 for t in c["targets"])          # num = ths - 1: skipped
        tc = tap_count(rec["detect_in"][0], *detect_grid(0)[:2])
        assert all((tc == k).any() for k in (0, 1, 2))
    if name == "inf_depth":
        d = rec["lines_depth"]
        reliable = rec["detect_in"][0] == 1
        assert (np.isposinf(d) & reliable).sum() > 500 and (np.isneginf(d) & reliable).sum() > 500
    if name.startswith("tiny"):
        assert min(w, h) < detect_grid(0)[1]                                        # narrower than the coarse tap gaps
        assert (w * h + 31) // 32 >= 2 and (w * h) % 32 != 0                        # more than one workgroup, the last partial

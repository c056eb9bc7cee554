"""The host code around the launches: how a call stages a caller's buffers, hands results back and leaves the context when it refuses.

One 53 x 37 scene (1961 pixels: no plane's byte size is a multiple of the scratch arena's 256-byte granule; both sides odd; the
quarter-resolution image is 13 x 9, the coarse level 27 x 19), 8-bit imagery, box 11, strict mode.  A hand-written label map of two
textureless column bands and a 70 % random mask give finite planes for both regions and a finite filled depth map.

1. every entry that takes `mem`, once with numpy buffers and once with torch device tensors from the same starting state: the same bytes;
2. the refinement chain, weak-texture detection and SLIC against the CPU oracle at this size;
3. every combination of optional outputs returns what the full call returns;
4. one context, many operators: the arena from empty through both overflows, the rebuild, fitting calls and one further growth;
5. a refused call leaves a working context.
NaN equals NaN whatever its sign (test_gpu_ransac_edges._same).  Where the binding always passes TSAR_MEM_HOST the C ABI is called directly."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu

W, H, SEED = 53, 37, 12
HOST, DEVICE = "host", "device"
_shared = {}


# ---- buffers of either kind ---------------------------------------------------------------------------------------------------
def _put(kind, a):
    a = np.ascontiguousarray(a)
    if kind == HOST:
        return a.copy()
    import torch
    return torch.from_numpy(a.copy()).cuda()


def _new(kind, shape, dtype):
    """an output buffer pre-filled with a pattern, so that a copy that never happens shows"""
    a = np.full(shape, 0x5A, np.uint8) if dtype == np.uint8 else np.full(shape, -77, dtype)
    return _put(kind, a)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _p(a):
    return api._ptr(a)[0]


def _mem(kind):
    return api.MEM_HOST if kind == HOST else api.MEM_DEVICE


def _ptr_array(bufs):
    arr = (C.c_void_p * len(bufs))()
    for i, b in enumerate(bufs):
        arr[i] = _p(b) if b is not None else None
    return arr


def _ok(m, rc):
    assert rc == api.TSAR_OK, (rc, m.L.tsar_last_error(m._ctx).decode())


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        return u
    return a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))


def _same_dict(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not _same(a[k], b[k])]
    assert not bad, bad


# ---- the scene and what the oracle makes of it ----------------------------------------------------------------------------------
def _oracle(sc, **kw):
    return ol.Oracle([im.cpu().numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, **kw)


def _case():
    """built once: the scene, the oracle's state after init + 2 iterations, labels, mask, maps for the other entries"""
    if not _shared:
        sc = synth.make_scene(W, H, 3, seed=7)
        orc = _oracle(sc, seed=SEED)
        orc.pm_init()
        orc.pm_iterate(2)
        rng = np.random.default_rng(5)
        x = np.broadcast_to(np.arange(W), (H, W))
        labels = np.where(x < 20, 1, np.where(x < 40, 2, 0)).astype(np.int32)
        mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.float32)
        text = np.array([1.0, -1.0, -1.0], np.float32)
        size = np.array([0.0, 36.0, 36.0], np.float32)
        gt = sc.gt_depth.numpy().astype(np.float32)
        scf = synth.make_scene(W, H, 3, seed=7, all_gt=True)          # the same scene with every view's ground truth (fusion, geometric term)
        n = len(sc.images)
        depths = [np.ascontiguousarray(d.numpy(), np.float32) for d, _ in scf.meta["gt_all"]]
        for v in range(n):
            depths[v] = depths[v] * (1 + rng.normal(0, 0.004, depths[v].shape).astype(np.float32))
            depths[v][rng.uniform(size=depths[v].shape) < 0.05] = 0
        normals = [np.ascontiguousarray((nc.numpy() @ scf.R[v]).astype(np.float32)) for v, (_, nc) in enumerate(scf.meta["gt_all"])]
        yy, xx = np.mgrid[0:2 * H, 0:2 * W]
        bgra = np.zeros((2 * H, 2 * W, 4), np.uint8)
        bgra[..., 0] = (127 + 100 * np.sin(xx / 7.0) * np.cos(yy / 9.0)).astype(np.uint8)
        bgra[..., 1] = ((xx * 3 + yy * 2) % 256).astype(np.uint8)
        bgra[..., 2] = (rng.integers(0, 30, size=(2 * H, 2 * W)) + 100 * ((xx // 12 + yy // 10) % 2)).astype(np.uint8)
        _shared.update(sc=sc, norm4=orc.norm4.copy(), c=orc.c.copy(), labels=labels, mask=mask, text=text, size=size, gt=gt,
                       pixel_text=np.where(labels > 0, -1.0, 1.0).astype(np.float32), depths=depths, normals=normals,
                       grays=[im.numpy().astype(np.float32) for im in sc.images], bgra=np.ascontiguousarray(bgra[:H, :W]), bgra_big=bgra,
                       pairs={v: [s for s in range(n) if s != v] for v in range(n)})
    return _shared


def _matcher(flags=0):
    cs = _case()
    return api.matcher_from_scene(cs["sc"], seed=SEED, flags=flags | api.FLAG_STRICT_DIV)


def _prepare(m):
    """the state before the refinement operators: the oracle's planes, getview, the mask, the hand-written regions"""
    cs = _case()
    m.set_plane(cs["norm4"], cs["c"])
    m.getview()
    m.set_reliable_mask(cs["mask"])
    m.set_regions(cs["labels"], cs["text"], cs["size"])


# ---- the entries, with buffers of one kind --------------------------------------------------------------------------------------
def _get_plane(m, kind, want=("planes", "cost", "beview", "ratio")):
    b = {"planes": _new(kind, (H, W, 4), np.float32), "cost": _new(kind, (H, W), np.float32), "beview": _new(kind, (H, W), np.int32),
         "ratio": _new(kind, (H, W), np.float32)}
    _ok(m, m.L.tsar_get_plane(m._ctx, *[_p(b[k]) if k in want else None for k in ("planes", "cost", "beview", "ratio")], _mem(kind)))
    return {k: _np(b[k]) for k in want}


def _set_plane(m, kind, planes, cost):
    p, c = _put(kind, planes), _put(kind, cost)
    _ok(m, m.L.tsar_set_plane(m._ctx, _p(p), _p(c), _mem(kind)))


def _get_result(m, kind, want=("depth", "normal", "cost", "confid")):
    shapes = {"depth": (H, W), "normal": (H, W, 3), "cost": (H, W), "confid": (H, W)}
    b = {k: _new(kind, shapes[k], np.float32) for k in want}
    _ok(m, m.L.tsar_get_result(m._ctx, *[_p(b[k]) if k in want else None for k in ("depth", "normal", "cost", "confid")], _mem(kind)))
    return {k: _np(b[k]) for k in want}


def _cost_planes(m, kind, planes, want=("beview", "ratio")):
    pl = _put(kind, planes)
    cost, bv, rt = _new(kind, (H, W), np.float32), _new(kind, (H, W), np.int32), _new(kind, (H, W), np.float32)
    _ok(m, m.L.tsar_pm_cost_planes(m._ctx, _p(pl), _mem(kind), _p(cost), _p(bv) if "beview" in want else None, _p(rt) if "ratio" in want else None))
    out = {"cost": _np(cost)}
    if "beview" in want:
        out["beview"] = _np(bv)
    if "ratio" in want:
        out["ratio"] = _np(rt)
    return out


def _geom_check(m, kind, depth, want=("count", "depth"), min_consistent=2):
    prm = api.GeomCheckParams(2.0, 0.01, min_consistent)
    d = _put(kind, depth) if depth is not None else None
    count, dout = _new(kind, (H, W), np.uint8), _new(kind, (H, W), np.float32)
    rc = m.L.tsar_geom_check(m._ctx, _p(d) if d is not None else None, C.byref(prm), _p(count) if "count" in want else None,
                             _p(dout) if "depth" in want else None, _mem(kind))
    _ok(m, rc)
    out = {"mask": m.get_reliable_mask()}
    if "count" in want:
        out["count"] = _np(count)
    if "depth" in want:
        out["depth"] = _np(dout)
    return out


def _set_geom(m, kind, maps):
    bufs = [None if (v == 0 or d is None) else _put(kind, d) for v, d in enumerate(maps)]
    _ok(m, m.L.tsar_set_geom_depths(m._ctx, len(bufs), _ptr_array(bufs), _mem(kind), 0.0, 3.0))


def _mask_roundtrip(m, kind, mask):
    s, o = _put(kind, mask), _new(kind, (H, W), np.float32)
    _ok(m, m.L.tsar_set_reliable_mask(m._ctx, _p(s), _mem(kind)))
    _ok(m, m.L.tsar_get_reliable_mask(m._ctx, _p(o), _mem(kind)))
    return _np(o)


def _set_regions(m, kind, labels, text, size):
    lb, tx, sz = _put(kind, labels), _put(kind, text), _put(kind, size)
    rc = m.L.tsar_set_regions(m._ctx, _p(lb), len(text), _p(tx), _p(sz), _mem(kind))
    if rc == api.TSAR_OK:
        m.n_regions = len(text)
    return rc


def _fake_depth(m, kind):
    o = _new(kind, (H, W), np.float32)
    _ok(m, m.L.tsar_fake_depth(m._ctx, _p(o), _mem(kind)))
    return _np(o)


def _detect(m, kind, want_labels=True, cap=1 << 12):
    lb = _new(kind, (H, W), np.int32)
    text, size = np.full(cap, -77, np.float32), np.full(cap, -77, np.float32)
    n = C.c_int(0)
    _ok(m, m.L.tsar_detect_weak_texture(m._ctx, _p(lb) if want_labels else None, _mem(kind), C.byref(n), _p(text), _p(size), cap))
    m.n_regions = n.value
    out = {"n": np.array([n.value]), "text": text, "size": size}            # (whole arrays: nothing past min(n, cap) may be written)
    if want_labels:
        out["labels"] = _np(lb)
    return out


def _slic(m, kind, bgra, S=8):
    img = _put(kind, bgra)
    h, w = bgra.shape[:2]
    lb = _new(kind, (h, w), np.int32)
    st = api.SlicSettings(S, 5, 5.0, 1, 0)
    rc = m.L.tsar_slic(m._ctx, _p(img), w, h, C.byref(st), _p(lb), _mem(kind))
    return rc, _np(lb)


def _fuse(m, kind, pairs=None):
    cs = _case()
    put = (lambda a: a) if kind == HOST else (lambda a: _put(kind, a))
    sc = cs["sc"]
    pts, n = api.fuse([put(a) for a in cs["depths"]], [put(a) for a in cs["normals"]], [put(a) for a in cs["grays"]], sc.K, sc.R, sc.t,
                      pairs or cs["pairs"], api.FusionParams(1, 2.0, 0.01, 15.0, 1), matcher=m, return_count=True)
    return {"points": _np(pts), "n": np.array([n])}


def _view_image(m, kind, view):
    o = _new(kind, (H, W), np.float32)
    _ok(m, m.L.tsar_get_view_image(m._ctx, view, _p(o), _mem(kind)))
    return _np(o)


def _set_views(m, kind, u8):
    sc = _case()["sc"]
    bufs = [_put(kind, im.numpy().astype(np.uint8 if u8 else np.float32)) for im in sc.images]
    n = len(bufs)
    cams = (api.Camera * n)()
    for i in range(n):
        cams[i].K[:] = np.asarray(sc.K[i], np.float32).ravel().tolist()
        cams[i].R[:] = np.asarray(sc.R[i], np.float32).ravel().tolist()
        cams[i].t[:] = np.asarray(sc.t[i], np.float32).ravel().tolist()
    _ok(m, (m.L.tsar_set_views_u8 if u8 else m.L.tsar_set_views)(m._ctx, n, W, H, _ptr_array(bufs), _mem(kind), cams))
    m.w, m.h, m.n_views = W, H, n


def _every_entry(kind):
    """every entry that takes `mem`, with buffers of one kind, from a fresh context: name -> output as a numpy array"""
    cs = _case()
    sc = cs["sc"]
    out = {}

    def keep(prefix, d):
        out.update({prefix + "." + k: v for k, v in d.items()})
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV, seed=SEED))
    for u8 in (False, True):                                     # the setters: what the next getter or operator returns
        _set_views(m, kind, u8)
        out["views%d.image" % u8] = _view_image(m, kind, 2)
        keep("views%d.cost_planes" % u8, _cost_planes(m, kind, cs["norm4"]))
    _set_plane(m, kind, cs["norm4"], cs["c"])
    keep("set_plane", _get_plane(m, kind))
    t = _put(kind, cs["pixel_text"])
    _ok(m, m.L.tsar_pm_iterate_final(m._ctx, 1, _p(t), _mem(kind)))
    keep("iterate_final", _get_plane(m, kind))
    d, nw = _put(kind, cs["depths"][0] + np.float32(0.5)), _put(kind, cs["normals"][0])
    _ok(m, m.L.tsar_load_planes(m._ctx, _p(d), _p(nw), _mem(kind)))
    keep("load_planes", _get_plane(m, kind, ("planes", "cost")))
    _set_plane(m, kind, cs["norm4"], cs["c"])
    r = _put(kind, np.ascontiguousarray(cs["norm4"][::-1]))
    _ok(m, m.L.tsar_compute_disp_final(m._ctx, _p(r), _p(t), _mem(kind)))
    keep("disp_final", _get_result(m, kind))
    coarse = api.Matcher()
    coarse.pyramid_from(m)
    coarse.pm_init()
    m.upsample_planes(coarse)
    _ok(m, m.L.tsar_compute_disp_final_upsampled(m._ctx, _p(t), _mem(kind)))
    keep("disp_final_upsampled", _get_result(m, kind))
    coarse.close()
    _set_geom(m, kind, cs["depths"])
    keep("geom_check", _geom_check(m, kind, cs["gt"]))
    m.clear_geom()
    _set_plane(m, kind, cs["norm4"], cs["c"])
    m.getview()
    out["mask"] = _mask_roundtrip(m, kind, cs["mask"])
    _ok(m, _set_regions(m, kind, cs["labels"], cs["text"], cs["size"]))
    planes, ratio = m.ransac_regions()
    out["ransac.planes"], out["ransac.ratio"] = planes[1:], ratio
    out["fake_depth"] = _fake_depth(m, kind)
    m.fill_textureless()
    keep("filled", _get_result(m, kind))
    keep("detect", _detect(m, kind))
    rc, out["slic"] = _slic(m, kind, cs["bgra"])
    _ok(m, rc)
    keep("fuse", _fuse(m, kind))
    m.close()
    return out


def _entries(kind):
    key = "entries_" + kind
    if key not in _shared:
        _shared[key] = _every_entry(kind)
    return _shared[key]


# ---- 1. both memory kinds ---------------------------------------------------------------------------------------------------------
def test_host_and_device_buffers_give_the_same_bytes():
    host, dev = _entries(HOST), _entries(DEVICE)
    _same_dict(host, dev)
    assert len(host["fuse.points"]) > 0 and np.isfinite(host["ransac.planes"]).all() and np.isfinite(host["filled.depth"]).all()
    assert np.array_equal(host["views0.image"], host["views1.image"]) and np.array_equal(host["views0.image"], _case()["grays"][2])
    assert _same(host["set_plane.planes"], _case()["norm4"]) and _same(host["set_plane.cost"], _case()["c"]) and _same(host["mask"], _case()["mask"])


# ---- 2. anchored to the oracle -----------------------------------------------------------------------------------------------------
def test_refinement_chain_is_the_oracles():
    cs = _case()
    sc = cs["sc"]
    orc = _oracle(sc, seed=SEED)
    orc.norm4[:] = cs["norm4"]
    orc.c[:] = cs["c"]
    orc.getview()
    orc.scale[:] = cs["mask"]
    orc.set_regions(cs["labels"], cs["text"], cs["size"])
    planes_ref, ratio_ref = orc.ransac_regions()
    orc.fake_depth()
    fake_ref = orc.fakedepth.copy()
    orc.update_scale()
    depth_ref = orc.compute_disp()[..., 3].copy()
    m = _matcher()
    _prepare(m)
    weak = cs["text"] == -1.0
    for call in range(2):                                       # (the second call takes recycled, unzeroed arena memory)
        planes, ratio = m.ransac_regions()
        assert _same(planes[weak], planes_ref[weak]) and _same(ratio, ratio_ref), call
    assert _same(m.fake_depth(), fake_ref)
    m.fill_textureless()
    assert _same(m.get_result(("depth",))["depth"], depth_ref)
    assert np.isfinite(planes_ref[weak]).all() and np.isfinite(depth_ref).all()
    m.close()
    for kind in (HOST, DEVICE):                                 # what test 1 compared between the kinds is the oracle's too
        e = _entries(kind)
        assert _same(e["ransac.planes"], planes_ref[1:]) and _same(e["ransac.ratio"], ratio_ref) and _same(e["filled.depth"], depth_ref)
        assert _same(e["fake_depth"], fake_ref)


def test_weak_texture_and_slic_are_the_oracles():
    cs = _case()
    ref = ol.weak_texture(cs["grays"][0].astype(np.uint8), connect="true", close_lines=True)
    slic_ref = ol.slic(cs["bgra"], 8, 5, 5.0, 1, 0)
    for kind in (HOST, DEVICE):
        e = _entries(kind)
        n = int(e["detect.n"][0])
        assert n == len(ref["text"]) and np.array_equal(e["detect.labels"], ref["labels"])
        assert np.array_equal(e["detect.text"][:n], ref["text"]) and np.array_equal(e["detect.size"][:n], ref["size"])
        assert np.array_equal(e["slic"], slic_ref)
    m = _matcher()                                              # and through the binding, twice in one context
    for _ in range(2):
        labels, text, size = m.detect_weak_texture()
        assert np.array_equal(labels, ref["labels"]) and np.array_equal(text, ref["text"]) and np.array_equal(size, ref["size"])
        assert np.array_equal(m.slic(cs["bgra"], api.SlicSettings(8, 5, 5.0, 1, 0)), slic_ref)
    m.close()


# ---- 3. every combination of optional outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [HOST, DEVICE])
def test_get_result_with_every_subset_of_its_outputs(kind):
    m = _matcher()
    _prepare(m)
    m.ransac_regions()
    m.fill_textureless()
    names = ("depth", "normal", "cost", "confid")
    full = _get_result(m, kind)
    for bits in range(1, 16):
        want = tuple(k for i, k in enumerate(names) if bits >> i & 1)
        got = _get_result(m, kind, want)
        assert set(got) == set(want) and all(_same(got[k], full[k]) for k in want), want
    m.close()


@pytest.mark.parametrize("kind", [HOST, DEVICE])
def test_geom_check_with_every_subset_of_its_outputs(kind):
    cs = _case()
    m = _matcher()
    _set_geom(m, kind, cs["depths"])
    full = _geom_check(m, kind, cs["gt"])
    assert int((full["count"] >= 2).sum()) > 0
    for want in (("count",), ("depth",)):
        got = _geom_check(m, kind, cs["gt"], want)
        assert all(_same(got[k], full[k]) for k in want + ("mask",)), want
    m.set_plane(cs["norm4"], cs["c"])                            # depth == NULL: the context's own result
    m.compute_disp()
    own = m.get_result(("depth",))["depth"]
    ref = _geom_check(m, kind, own)
    for want in (("count", "depth"), ("count",), ("depth",)):
        got = _geom_check(m, kind, None, want)
        assert all(_same(got[k], ref[k]) for k in want + ("mask",)), want
    m.close()


def test_ransac_regions_with_either_or_both_outputs_null():
    cs = _case()
    m = _matcher()
    _prepare(m)
    planes, ratio = m.ransac_regions()
    fake = m.fake_depth()
    for want_planes, want_ratio in ((True, False), (False, True), (False, False)):
        m.set_regions(cs["labels"], cs["text"], cs["size"])     # (zeroes the region planes: fake_depth below reads this call's fit)
        p, r = np.full((3, 4), -77, np.float32), np.full(3, -77, np.float32)
        _ok(m, m.L.tsar_ransac_regions(m._ctx, _p(p) if want_planes else None, _p(r) if want_ratio else None))
        assert not want_planes or _same(p[1:], planes[1:])
        assert not want_ratio or _same(r, ratio)
        assert _same(m.fake_depth(), fake)
    m.close()


@pytest.mark.parametrize("kind", [HOST, DEVICE])
def test_detect_weak_texture_without_labels_and_with_a_small_cap(kind):
    m = _matcher()
    full = _detect(m, kind)
    n = int(full["n"][0])
    assert n >= 2
    got = _detect(m, kind, want_labels=False)
    assert _same(got["text"], full["text"]) and _same(got["size"], full["size"]) and got["n"][0] == n
    small = _detect(m, kind, cap=n - 1)
    assert small["n"][0] == n and _same(small["labels"], full["labels"])
    assert _same(small["text"], full["text"][:n - 1]) and _same(small["size"], full["size"][:n - 1])
    m.close()


@pytest.mark.parametrize("kind", [HOST, DEVICE])
def test_cost_planes_with_optional_outputs_null(kind):
    cs = _case()
    m = _matcher()
    full = _cost_planes(m, kind, cs["norm4"])
    for want in (("beview",), ("ratio",), ()):
        got = _cost_planes(m, kind, cs["norm4"], want)
        assert set(got) == set(want) | {"cost"} and all(_same(got[k], full[k]) for k in got), want
    m.close()


# ---- 4. one arena, many operators -------------------------------------------------------------------------------------------------
def test_one_arena_serves_every_operator_round_after_round():
    cs = _case()
    m = _matcher()
    rounds = []
    for rnd in range(3):
        out = {}
        rc, out["slic"] = _slic(m, HOST, cs["bgra"])
        _ok(m, rc)
        out.update({"detect." + k: v for k, v in _detect(m, HOST).items()})
        _prepare(m)
        planes, ratio = m.ransac_regions()
        out["ransac.planes"], out["ransac.ratio"] = planes[1:], ratio
        m.wmf(1, False)
        out["wmf.mask"] = m.get_reliable_mask()
        out.update({"wmf." + k: v for k, v in _get_plane(m, HOST, ("planes", "cost")).items()})
        out.update({"fuse." + k: v for k, v in _fuse(m, HOST).items()})
        if rnd == 1:                                            # the calls that must not grow the arena, between two rounds
            out_cost = _cost_planes(m, HOST, cs["norm4"])
            m.set_plane(cs["norm4"], cs["c"])
            m.compute_disp_final(cs["norm4"][::-1], cs["pixel_text"])
            out_final = _get_result(m, HOST, ("depth", "normal", "cost"))
        rounds.append(out)
    for rnd in (1, 2):
        _same_dict(rounds[rnd], rounds[0])
    e = _entries(HOST)
    assert all(_same(out_cost[k], e["views1.cost_planes." + k]) for k in out_cost)
    assert all(_same(out_final[k], e["disp_final." + k]) for k in out_final)
    _same_dict({k: v for k, v in rounds[0].items() if k.startswith(("fuse.", "slic", "detect."))},
               {k: v for k, v in e.items() if k.startswith(("fuse.", "slic", "detect."))})
    rc, big = _slic(m, HOST, cs["bgra_big"])                    # four times the pixels: the arena grows once more
    _ok(m, rc)
    assert np.array_equal(big, ol.slic(cs["bgra_big"], 8, 5, 5.0, 1, 0))
    rc, again = _slic(m, HOST, cs["bgra"])
    _ok(m, rc)
    assert np.array_equal(again, rounds[0]["slic"])
    m.close()


# ---- 5. a refused call leaves a working context -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [HOST, DEVICE])
def test_a_refused_call_leaves_a_working_context(kind):
    cs = _case()
    m = _matcher()
    n = len(cs["depths"])
    # tsar_fuse_ctx with a source index of n_views: refused after staging has begun
    good = _fuse(m, kind)
    bad_pairs = dict(cs["pairs"])
    bad_pairs[n - 1] = [0, n]
    with pytest.raises(api.TsarError) as ei:
        _fuse(m, kind, bad_pairs)
    assert ei.value.code == api.TSAR_ERR_INVALID and "source index is out of range" in str(ei.value)
    _same_dict(_fuse(m, kind), good)
    # tsar_set_regions with a label equal to n_regions: the regions installed before still serve ransac_regions
    _prepare(m)
    planes, ratio = m.ransac_regions()
    bad = cs["labels"].copy()
    bad[H - 1, W - 1] = 3
    assert _set_regions(m, kind, bad, cs["text"], cs["size"]) == api.TSAR_ERR_INVALID
    assert "outside [0, n_regions)" in m.L.tsar_last_error(m._ctx).decode()
    m.set_reliable_mask(cs["mask"])
    p2, r2 = m.ransac_regions()
    assert _same(p2[1:], planes[1:]) and _same(r2, ratio)
    # tsar_slic with a superpixel size of 3
    rc, good_slic = _slic(m, kind, cs["bgra"])
    _ok(m, rc)
    rc, _ = _slic(m, kind, cs["bgra"], S=3)
    assert rc == api.TSAR_ERR_INVALID and "bad SLIC settings" in m.L.tsar_last_error(m._ctx).decode()
    rc, after = _slic(m, kind, cs["bgra"])
    assert rc == api.TSAR_OK and _same(after, good_slic)
    # tsar_wmf with iters 0
    _prepare(m)
    with pytest.raises(api.TsarError) as ei:
        m.wmf(0, False)
    assert ei.value.code == api.TSAR_ERR_INVALID and "iters must be 1..4" in str(ei.value)
    m.wmf(1, False)
    wmf_mask, wmf_planes = m.get_reliable_mask(), _get_plane(m, kind, ("planes",))["planes"]
    _prepare(m)
    m.wmf(1, False)
    assert _same(m.get_reliable_mask(), wmf_mask) and _same(_get_plane(m, kind, ("planes",))["planes"], wmf_planes)
    # tsar_geom_check without a term
    prm = api.GeomCheckParams(2.0, 0.01, 2)
    d, cnt = _put(kind, cs["gt"]), _new(kind, (H, W), np.uint8)
    assert m.L.tsar_geom_check(m._ctx, _p(d), C.byref(prm), _p(cnt), None, _mem(kind)) == api.TSAR_ERR_STATE
    assert "no geometric-consistency term installed" in m.L.tsar_last_error(m._ctx).decode()
    assert (_np(cnt) == 0x5A).all()
    _set_geom(m, kind, cs["depths"])
    _same_dict(_geom_check(m, kind, cs["gt"]), {k[len("geom_check."):]: v for k, v in _entries(kind).items() if k.startswith("geom_check.")})
    m.close()

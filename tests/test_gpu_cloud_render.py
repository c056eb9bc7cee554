"""tsar_cloud_render and tsar_depth_compare on the GPU against the numpy restatement (tests/cloud_render_ref.py): depth, count, index, n_splats
and every count of the comparison exactly, every element — in host and device memory, with strides 3, 4 and 9 (the extra columns hold NaN),
through a strict and a fast context that hold views and a plane state, and context-free; contention on one pixel, footprints at max_px on
every border pixel, point counts around the wave size, the shuffled cloud, determinism, every refusal; api.evaluate_depth_maps on the maps of
a PatchMatch run, and the built tsar_evaluate_maps on the same maps."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from cloud_render_ref import back_project, cloud_render_ref, depth_compare_ref, evaluate_depth_maps_ref, landings, ratios, scene, thinned_cloud
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("strict", False, 3), ("fast", True, 9), ("fast", False, 4))       # (context, device memory, stride)
WANT = ("depth", "count", "index")


@pytest.fixture(scope="module")
def ctxs(small_scene):
    """a strict and a fast context, each holding views and a plane state: the operators must run on them and leave them alone"""
    ms = {}
    for name, flags in (("strict", api.FLAG_STRICT_DIV), ("fast", 0)):
        m = api.matcher_from_scene(small_scene, seed=5, flags=flags)
        m.pm_init()
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


def padded(a, stride):
    out = np.full((len(a), stride), np.nan, F)
    out[:, :3] = a[:, :3]
    return out


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def camera(w, h):
    """a camera of w x h pixels off the world's axes (synth's first source view)"""
    Ks, Rs, ts = synth.make_cameras(w, h, 1, seed=3, step=0.2)
    return Ks[1], Rs[1], ts[1]


def points_at(cam, u, v, z):
    """the world points that project to pixel coordinates (u, v) at depth z in `cam`, rounded to float32 (so they land there or next to it)"""
    Kc, Rc, tc = (np.asarray(a, np.float64) for a in cam)
    pix = np.stack([np.asarray(u, np.float64), np.asarray(v, np.float64), np.ones(len(u))], 0)
    return np.ascontiguousarray((Rc.T @ (np.linalg.inv(Kc) @ pix * np.asarray(z, np.float64)[None, :] - tc.reshape(3, 1))).T.astype(F))


def random_cloud(rng, n, cam, w, h, zlo=3.0, zhi=7.0):
    """n points all over the image and a little beyond its borders, with some non-finite records"""
    c = points_at(cam, rng.uniform(-2.0, w + 1.0, n), rng.uniform(-2.0, h + 1.0, n), rng.uniform(zlo, zhi, n))
    if n >= 20:
        c[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = [np.nan, np.inf, -np.inf]
    return c


def same(got, ref, what=""):
    assert got["n_splats"] == ref["n_splats"], what
    for k in WANT:
        g = host(got[k])
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, (k, g.dtype, g.shape)
        bits = (lambda a: a.view(np.uint32)) if k == "depth" else (lambda a: a)
        assert np.array_equal(bits(g), bits(ref[k])), "%s differs in %d of %d pixels (%s)" % (k, np.count_nonzero(bits(g) != bits(ref[k])), g.size, what)


def check(ctxs, cloud, cam, w, h, modes=MODES, **kw):
    """the operator against the restatement, every output, every element"""
    ref = cloud_render_ref(cloud, cam[0], cam[1], cam[2], w, h, **kw)
    assert not ref["refused"]
    for name, on_device, stride in modes:
        c = padded(cloud, stride)
        if on_device:
            c = torch.from_numpy(c).cuda()
        r = api.cloud_render(c, cam[0], cam[1], cam[2], w, h, want=WANT, matcher=ctxs[name], **kw)
        assert all(torch.is_tensor(r[k]) and r[k].is_cuda for k in WANT) if on_device else all(isinstance(r[k], np.ndarray) for k in WANT)
        same(r, ref, "%s, device %s, stride %d, %s" % (name, on_device, stride, kw))
    return ref


# ---- the render ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacings", [0.0, 1.5])
def test_the_scene_cloud(ctxs, spacings):
    sc, cloud, spacing = scene()
    cam = (sc.K[0], sc.R[0], sc.t[0])
    ref = check(ctxs, cloud, cam, sc.w, sc.h, radius=F(spacings * spacing))
    assert len(cloud) == 57600 and ref["landed"].mean() > 0.9 and (ref["n_splats"] > 4 * len(cloud)) == (spacings > 0)
    if spacings:
        assert 0 < np.count_nonzero(ref["landed"] & ~ref["visible"]) and ref["count"].max() > 1
        thin = check(ctxs, thinned_cloud(), cam, sc.w, sc.h, radius=F(spacings * spacing), modes=MODES[:2])
        gt = sc.gt_depth.numpy()
        have = thin["depth"] > 0
        assert np.count_nonzero((thin["depth"][have] - gt[have]) / gt[have] > 1e-2) == 0          # the holes of the foreground are closed


def test_an_image_wider_than_one_row_of_lanes(ctxs):
    rng = np.random.default_rng(1)
    cam = camera(67, 45)
    cloud = random_cloud(rng, 20000, cam, 67, 45)
    ref = check(ctxs, cloud, cam, 67, 45, radius=0.4, max_px=5, min_points=2, depth_diff=0.05)
    assert ref["landed"].mean() > 0.99 and 0 < np.count_nonzero(ref["depth"]) < 67 * 45 and ref["count"].max() > 3
    check(ctxs, cloud, cam, 67, 45)
    check(ctxs, cloud, cam, 1, 1, radius=0.05)
    check(ctxs, cloud, cam, 300, 2, radius=0.05, max_px=16)


def test_contention_on_one_pixel(ctxs):
    rng = np.random.default_rng(2)
    cam = camera(33, 21)
    z = rng.permutation(np.linspace(4.0, 6.0, 10000))
    cloud = points_at(cam, np.full(10000, 16.0), np.full(10000, 10.0), z)
    lands, xi, yi, p2, _ = landings(cloud, cam[0], cam[1], cam[2], 33, 21)
    assert lands.all() and (xi == 16).all() and (yi == 10).all() and len(np.unique(p2)) > 9000
    ref = check(ctxs, cloud, cam, 33, 21, radius=0.5, depth_diff=0.1)
    assert ref["index"][10, 16] == int(np.argmin(p2)) and ref["count"][10, 16] == 255 and ref["support"][10, 16] > 1000
    front = points_at(cam, [16.0], [10.0], [3.5])
    cloud[rng.choice(10000, 1000, replace=False)] = front[0]                 # a thousand equal front-most depths
    ref = check(ctxs, cloud, cam, 33, 21, radius=0.5, depth_diff=1e-4)
    first = int(np.flatnonzero((cloud == front[0]).all(axis=1))[0])
    assert ref["index"][10, 16] == first and ref["support"][10, 16] == 1000 and ref["count"][10, 16] == 255
    assert check(ctxs, cloud, cam, 33, 21, min_points=255, depth_diff=1e-4)["depth"][10, 16] == ref["depth"][10, 16]


def test_maximal_footprints_on_every_border_pixel(ctxs):
    w, h = 40, 33
    cam = camera(w, h)
    border = [(u, v) for u in range(w) for v in (0, h - 1)] + [(u, v) for v in range(1, h - 1) for u in (0, w - 1)]
    rng = np.random.default_rng(3)
    u, v = np.array(border, np.float64).T
    cloud = points_at(cam, u, v, rng.uniform(4.0, 6.0, len(border)))
    ref = check(ctxs, cloud, cam, w, h, radius=10.0, max_px=16)
    lands, xi, yi, _, s = landings(cloud, cam[0], cam[1], cam[2], w, h, radius=10.0, max_px=16)
    assert lands.all() and (s == 16).all() and len(set(zip(xi.tolist(), yi.tolist()))) == len(border)
    assert ref["n_splats"] < 33 * 33 * len(border) and np.isfinite(ref["Zo"]).all()             # clipped; together they cover the image
    check(ctxs, cloud, cam, w, h, radius=10.0, max_px=1)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 64 * 1024 + 1])
def test_point_counts(ctxs, n):
    rng = np.random.default_rng(100 + n)
    cam = camera(50, 37)
    cloud = random_cloud(rng, n, cam, 50, 37)
    ref = check(ctxs, cloud, cam, 50, 37, radius=0.3)
    assert (n == 0) == (ref["n_splats"] == 0)
    own = api.cloud_render(cloud, cam[0], cam[1], cam[2], 50, 37, radius=0.3, want=WANT)      # a context of the call's own
    same(own, ref, "context-free")


def test_a_shuffled_cloud_and_two_runs(ctxs):
    sc, cloud, spacing = scene()
    cam = (sc.K[0], sc.R[0], sc.t[0])
    kw = dict(radius=F(1.5 * spacing), want=WANT)
    a = api.cloud_render(cloud, *cam, sc.w, sc.h, matcher=ctxs["fast"], **kw)
    b = api.cloud_render(cloud, *cam, sc.w, sc.h, matcher=ctxs["fast"], **kw)
    d = api.cloud_render(torch.from_numpy(cloud).cuda(), *cam, sc.w, sc.h, matcher=ctxs["strict"], **kw)
    for r in (b, d):
        same(r, a, "a second run")
    perm = np.random.default_rng(4).permutation(len(cloud))
    s = api.cloud_render(cloud[perm], *cam, sc.w, sc.h, matcher=ctxs["fast"], **kw)
    assert np.array_equal(s["depth"].view(np.uint32), a["depth"].view(np.uint32)) and np.array_equal(s["count"], a["count"]) and s["n_splats"] == a["n_splats"]
    kept = a["index"] >= 0
    assert np.array_equal(s["index"] >= 0, kept) and kept.sum() > 10000
    p2 = landings(cloud, *cam, sc.w, sc.h)[3]
    assert np.array_equal(p2[perm[s["index"][kept]]], p2[a["index"][kept]])                      # a point of the same depth, whatever its new index
    assert np.array_equal(p2[a["index"][kept]].view(np.uint32), a["depth"][kept].view(np.uint32))


def test_want_names_the_outputs(ctxs):
    rng = np.random.default_rng(5)
    cam = camera(50, 37)
    cloud = random_cloud(rng, 5000, cam, 50, 37)
    ref = cloud_render_ref(cloud, *cam, 50, 37, radius=0.3, min_points=2)
    for want in (("depth",), ("index",), ("count",), ("depth", "index")):                        # min_points 2: the support pass runs without count_out too
        r = api.cloud_render(cloud, *cam, 50, 37, radius=0.3, min_points=2, want=want, matcher=ctxs["fast"])
        assert sorted(r) == sorted(want + ("n_splats",)) and all(np.array_equal(r[k], ref[k]) for k in want)
    r = api.cloud_render(cloud, *cam, 50, 37, radius=0.3, want=("depth",), matcher=ctxs["fast"])        # min_points 1 without count: no support pass
    assert np.array_equal(r["depth"], cloud_render_ref(cloud, *cam, 50, 37, radius=0.3)["depth"])


def raw_render(m, cloud, cam, w, h, on_device=False, **fields):
    c = np.ascontiguousarray(cloud, F)
    bufs = [np.full((h, w), -7, F), np.full((h, w), 77, np.uint8), np.full((h, w), -7, np.int32)]
    if on_device:
        c, bufs = torch.from_numpy(c).cuda(), [torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
    ptr = (lambda a: C.c_void_p(a.data_ptr())) if on_device else (lambda a: a.ctypes.data_as(C.c_void_p))
    p = api.CloudRenderParams()
    m.L.tsar_default_cloud_render_params(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    n_splats = C.c_int64(-1)
    rc = m.L.tsar_cloud_render_ctx(m._ctx, ptr(c), len(c), c.shape[1], api._cameras(cam[0][None], cam[1][None], cam[2][None], 1), w, h, C.byref(p), ptr(bufs[0]), ptr(bufs[1]),
                                   ptr(bufs[2]), C.byref(n_splats), api.MEM_DEVICE if on_device else api.MEM_HOST)
    return rc, m.L.tsar_last_error(m._ctx).decode(), n_splats.value, [host(b) for b in bufs]


@pytest.mark.parametrize("on_device", [False, True])
def test_max_splats_refuses_before_anything_is_written(ctxs, on_device):
    rng = np.random.default_rng(6)
    cam = camera(50, 37)
    cloud = random_cloud(rng, 3000, cam, 50, 37)
    n_splats = cloud_render_ref(cloud, *cam, 50, 37, radius=0.3)["n_splats"]
    rc, msg, got, bufs = raw_render(ctxs["fast"], cloud, cam, 50, 37, on_device, radius=0.3, max_splats=n_splats - 1)
    assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_render:") and "max_splats" in msg and got == n_splats
    assert (bufs[0] == -7).all() and (bufs[1] == 77).all() and (bufs[2] == -7).all()
    rc, _, got, bufs = raw_render(ctxs["fast"], cloud, cam, 50, 37, on_device, radius=0.3, max_splats=n_splats)
    assert rc == api.TSAR_OK and got == n_splats and (bufs[1] != 77).any()
    with pytest.raises(api.TsarError) as e:
        api.cloud_render(cloud, *cam, 50, 37, radius=0.3, max_splats=10, matcher=ctxs["strict"])
    assert e.value.code == api.TSAR_ERR_INVALID and e.value.n_splats == n_splats


def test_every_refusal_and_the_context_works_afterwards(ctxs):
    m = ctxs["strict"]
    L = m.L
    rng = np.random.default_rng(7)
    cam = camera(50, 37)
    cloud = random_cloud(rng, 500, cam, 50, 37)
    cp = cloud.ctypes.data_as(C.c_void_p)
    out = np.full(50 * 37, -7, np.int32)
    op = out.ctypes.data_as(C.c_void_p)
    cams = api._cameras(cam[0][None], cam[1][None], cam[2][None], 1)

    def params(**fields):
        p = api.CloudRenderParams()
        L.tsar_default_cloud_render_params(C.byref(p))
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def refused(fragment, c=cp, n=500, stride=3, camera_=cams, w=50, h=37, prm=params(), outs=(op, None, None), mem=api.MEM_HOST):
        rc = L.tsar_cloud_render_ctx(m._ctx, c, n, stride, camera_, w, h, C.byref(prm) if prm is not None else None, outs[0], outs[1], outs[2], None, mem)
        msg = L.tsar_last_error(m._ctx).decode()
        assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_render:") and fragment in msg, (rc, msg)
        assert (out == -7).all()                                              # a refused call writes nothing

    refused("params is NULL", prm=None)
    refused("cam is NULL", camera_=None)
    refused("mem must be", mem=7)
    refused("n must be", n=-1)
    refused("n must be", n=1 << 31)
    refused("stride", stride=2)
    refused("cloud is NULL", c=None)
    refused("all NULL", outs=(None, None, None))
    for w, h in ((0, 37), (50, 0), (-1, 37), ((1 << 23) - 2, 1), (1, (1 << 23) - 2), (50000, 50000)):
        refused("w and h must be", w=w, h=h)
    for r in (-1.0, np.inf, -np.inf, np.nan):
        refused("radius must be finite and >= 0", prm=params(radius=r))
    refused("K[0] * radius", prm=params(radius=3e38))
    for v in (0, 17, -1):
        refused("max_px must be in 1..16", prm=params(max_px=v))
    for v in (-0.5, np.inf, np.nan):
        refused("occlusion_diff must be finite and >= 0", prm=params(occlusion_diff=v))
        refused("depth_diff must be finite and >= 0", prm=params(depth_diff=v))
    for v in (0, 256, -3):
        refused("min_points must be in 1..255", prm=params(min_points=v))
    refused("max_splats must be >= 0", prm=params(max_splats=-1))
    refused("more than max_splats", prm=params(max_splats=3))
    assert cloud_render_ref(cloud, *cam, 50, 37)["n_splats"] > 3
    with pytest.raises(AssertionError):
        api.cloud_render(cloud[:, :2], *cam, 50, 37, matcher=m)
    assert L.tsar_depth_compare_ctx(m._ctx, cp, cp, None, 10, 1, (C.c_float * 1)(0.1), None, None, None, None, None, None, 7) == api.TSAR_ERR_INVALID
    tol = (C.c_float * 17)(*([0.1] * 17))
    for kw in (dict(n=-1), dict(n=1 << 31), dict(d=None), dict(g=None), dict(n_tol=0), dict(n_tol=17), dict(t=None), dict(t=(C.c_float * 1)(-0.1)),
               dict(t=(C.c_float * 1)(np.nan)), dict(t=(C.c_float * 1)(np.inf))):
        a = dict(d=cp, g=cp, n=10, n_tol=1, t=tol)
        a.update(kw)
        rc = L.tsar_depth_compare_ctx(m._ctx, a["d"], a["g"], None, a["n"], a["n_tol"], a["t"], None, None, None, None, None, op, api.MEM_HOST)
        assert rc == api.TSAR_ERR_INVALID and L.tsar_last_error(m._ctx).decode().startswith("tsar_depth_compare:") and (out == -7).all(), kw
    check(ctxs, cloud, cam, 50, 37, radius=0.3)                              # and the contexts still work


def test_the_contexts_are_left_as_they_were(ctxs):
    """get_plane before and after is bit-equal, after calls that succeed and calls that are refused, and the matcher goes on"""
    sc, cloud, spacing = scene()
    cam = (sc.K[0], sc.R[0], sc.t[0])
    bits = lambda planes: [np.asarray(a).view(np.uint32).copy() for a in planes]
    for m in ctxs.values():
        before = bits(m.get_plane())
        r = api.cloud_render(cloud, *cam, sc.w, sc.h, radius=F(1.5 * spacing), matcher=m)
        api.cloud_render(torch.from_numpy(cloud).cuda(), *cam, sc.w, sc.h, matcher=m)
        with pytest.raises(api.TsarError):
            api.cloud_render(cloud, *cam, sc.w, sc.h, radius=1.0, max_splats=5, matcher=m)
        api.depth_compare(r["depth"], sc.gt_depth.numpy(), [0.01], want_error=True, matcher=m)
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(m.get_plane())))
        m.pm_iterate(1)


# ---- depth_compare ---------------------------------------------------------------------------------------------------------------------------
def some_maps(rng, shape):
    """a ground truth and a map with values of every kind: near, far, zero, negative, NaN, +inf, exactly on a tolerance"""
    gt = rng.uniform(2.0, 8.0, shape).astype(F)
    d = (gt * (1 + rng.normal(scale=5e-3, size=shape))).astype(F)
    for a in (gt, d):
        kind = rng.integers(0, 16, size=shape)
        a[kind == 0] = 0
        a[kind == 1] = np.nan
        a[kind == 2] = np.inf
        a[kind == 3] = -1
    on = rng.integers(0, 8, size=shape) == 0
    d[on] = (gt[on] + F(0.01) * gt[on]).astype(F)
    return d, gt, (rng.integers(0, 3, size=shape) > 0).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1,), (63,), (64 * 256 + 7,), (120, 160)])
@pytest.mark.parametrize("masked", [False, True])
def test_depth_compare(ctxs, shape, masked):
    rng = np.random.default_rng(sum(shape))
    d, gt, mask = some_maps(rng, shape)
    tol = [0.01, 0.001, 0.05]
    ref = depth_compare_ref(d, gt, tol, mask if masked else None)
    for name, on_device in (("strict", False), ("fast", True)):
        args = [torch.from_numpy(a).cuda() for a in (d, gt, mask)] if on_device else [d, gt, mask]
        r = api.depth_compare(args[0], args[1], tol, args[2] if masked else None, want_error=True, matcher=ctxs[name])
        for k in ("n_gt", "n_both", "n_front", "n_behind"):
            assert r[k] == ref[k], k
        assert r["within"].dtype == np.int64 and r["within"].tolist() == ref["within"].tolist()
        err = host(r["error"])
        assert err.shape == shape and np.array_equal(np.isnan(err), np.isnan(ref["error"])) and np.array_equal(err[~np.isnan(err)].view(np.uint32), ref["error"][~np.isnan(err)].view(np.uint32))
        q = ratios(ref)
        assert r["accuracy"].tolist() == q["accuracy"].tolist() and r["completeness"].tolist() == q["completeness"].tolist() and r["cover"] == q["cover"]
        assert "error" not in api.depth_compare(args[0], args[1], tol, matcher=ctxs[name])
    if len(shape) == 2:
        assert 0 < ref["n_front"] and 0 < ref["n_behind"] and 0 < ref["within"][1] < ref["within"][0] < ref["within"][2] <= ref["n_both"] < ref["n_gt"]      # (0.05 is ten sigma of the noise)
        own = api.depth_compare(d, gt, tol, mask if masked else None)                             # context-free
        assert own["within"].tolist() == ref["within"].tolist() and own["n_gt"] == ref["n_gt"]
        full = api.depth_compare(d, gt, [0.01] * 16, matcher=ctxs["fast"])                        # the most tolerances
        assert full["within"].tolist() == [int(ref["within"][0])] * 16 if not masked else True


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matched():
    """the small scene with every view's ground truth, the cloud of those maps, and the depth map of a strict three-iteration PatchMatch per view"""
    sc = synth.make_scene(96, 64, 3, seed=7, all_gt=True)
    n = len(sc.images)
    cloud = np.concatenate([back_project(sc.meta["gt_all"][v][0].numpy(), sc.K[v], sc.R[v], sc.t[v]) for v in range(n)])
    maps = []
    for ref in range(n):
        order = [ref] + [v for v in range(n) if v != ref]
        m = api.Matcher()
        m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max, seed=3 + ref, flags=api.FLAG_STRICT_DIV))
        m.set_views([sc.images[v] for v in order], sc.K[order], sc.R[order], sc.t[order])
        m.pm_init()
        m.pm_iterate(3)
        m.compute_disp()
        maps.append(m.get_result(("depth",))["depth"].copy())
        m.close()
    return sc, np.ascontiguousarray(cloud), maps, F(1.5 * 5.0 / float(sc.K[0][0, 0]))


def same_counts(got, ref):
    for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats"):
        assert got[k] == ref[k], k
    assert list(got["within"]) == ref["within"].tolist()
    q = ratios(ref)
    assert list(got["accuracy"]) == q["accuracy"].tolist() and list(got["completeness"]) == q["completeness"].tolist() and got["cover"] == q["cover"]


def test_evaluate_depth_maps_equals_the_composition(matched, ctxs):
    sc, cloud, maps, radius = matched
    tol = [0.001, 0.01]
    masks = [np.asarray(m > 0, np.uint8) for m in maps[::-1]]
    for mk, kw in ((None, {}), (masks, dict(max_px=4, min_points=2))):
        views_ref, total_ref = evaluate_depth_maps_ref(maps, cloud, sc.K, sc.R, sc.t, tol, radius, masks=mk, **kw)
        views, total = api.evaluate_depth_maps(maps, cloud, sc.K, sc.R, sc.t, tol, radius, masks=mk, matcher=ctxs["fast"], **kw)
        assert len(views) == 4
        for got, ref in zip(views, views_ref):
            same_counts(got, ref)
        same_counts(total, total_ref)
    assert 0 < total_ref["within"][0] < total_ref["within"][1] < total_ref["n_both"] <= total_ref["n_gt"]       # PatchMatch found something, not everything
    fused9 = padded(cloud, 9)                                                                    # a fused cloud's records go in as they are, on the device too
    views, total = api.evaluate_depth_maps(maps, torch.from_numpy(fused9).cuda(), sc.K, sc.R, sc.t, tol, radius, **kw)
    same_counts(total, total_ref)


def test_the_built_tool_equals_evaluate_depth_maps(matched, tmp_path):
    sc, cloud, maps, radius = matched
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    for v, d in enumerate(maps):
        os.makedirs(root + "APD/%08d" % v)
        tio.write_dmb(root + "APD/%08d/TSAR_disp.dmb" % v, d)
    tio.write_ply(root + "gt.ply", cloud)
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate_maps")
    out = subprocess.run([tool, root, root + "gt.ply", "--tolerances=0.001,0.01", "--radius=%.9g" % radius, "--write_gt=scan"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    views, total = api.evaluate_depth_maps(maps, cloud, sc.K, sc.R, sc.t, [0.001, 0.01], radius)
    assert [v["id"] for v in rec["views"]] == [0, 1, 2, 3] and rec["skipped"] == []
    for got, want in zip(rec["views"] + [rec["total"]], views + [total]):
        for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "cover"):
            assert got[k] == want[k], k
        assert got["within"] == want["within"].tolist() and got["accuracy"] == want["accuracy"].tolist() and got["completeness"] == want["completeness"].tolist()
    for v in range(4):
        r = api.cloud_render(cloud, sc.K[v], sc.R[v], sc.t[v], 96, 64, radius=radius, want=("depth",))
        assert np.array_equal(tio.read_dmb(root + "APD/%08d/scan_disp.dmb" % v).view(np.uint32), r["depth"].view(np.uint32))

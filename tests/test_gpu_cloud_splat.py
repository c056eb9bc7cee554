"""tsar_cloud_render_oriented on the GPU against the numpy restatement (tests/cloud_splat_ref.py): depth, count, index, occluder, n_splats and
n_covered exactly, every element — in host and device memory, with the normals as a separate array and inside 9-float records, through a
strict and a fast context that hold views and a plane state, and context-free; the slanted scene, normals estimated on the GPU, normals that
orient nothing against tsar_cloud_render itself, maximal footprints on every border pixel, contention on one pixel, degenerate images, point
counts around the wave size, the shuffled cloud, determinism, TSAR_RENDER_SKIP=0 in a child process, every refusal; api.evaluate_depth_maps
with normals, and the built tsar_evaluate_maps --oriented."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cloud_render_ref import cloud_render_ref, depth_compare_ref, landings, ratios, scene, thinned_cloud
from cloud_splat_ref import SLANT_H, SLANT_W, cloud_render_oriented_ref, slant_spacing, slanted_scene
from tsar_mvs_amd import api, synth
from tsar_mvs_amd import io as tio

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("depth", "count", "index", "occluder")
MODES = (("strict", False, "array"), ("fast", True, "record"), ("fast", True, "array"), ("strict", False, "record"))      # (context, device memory, where the normals are)


@pytest.fixture(scope="module")
def ctxs(small_scene):
    """a strict and a fast context, each holding views and a plane state: the operator must run on them and leave them alone"""
    ms = {}
    for name, flags in (("strict", api.FLAG_STRICT_DIV), ("fast", 0)):
        m = api.matcher_from_scene(small_scene, seed=5, flags=flags)
        m.pm_init()
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def records(cloud, normals):
    """9-float records like tsar_fuse's: x y z, the normal, and three floats nothing reads (NaN)"""
    out = np.full((len(cloud), 9), np.nan, F)
    out[:, :3], out[:, 3:6] = cloud[:, :3], normals[:, :3]
    return out


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


def random_normals(rng, n):
    """random directions; of twenty or more, some zero, some not finite"""
    nrm = rng.normal(size=(n, 3)).astype(F)
    if n >= 20:
        nrm[::5] = 0
        nrm[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = [np.nan, np.inf, -np.inf]
    return nrm


def same(got, ref, what="", planes=PLANES):
    assert got["n_splats"] == ref["n_splats"] and got["n_covered"] == ref["n_covered"], (what, got["n_splats"], ref["n_splats"], got["n_covered"], ref["n_covered"])
    for k in planes:
        g, r = host(got[k]), host(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, g.shape)
        bits = (lambda a: a.view(np.uint32)) if g.dtype == F else (lambda a: a)
        assert np.array_equal(bits(g), bits(r)), "%s differs in %d of %d pixels (%s)" % (k, np.count_nonzero(bits(g) != bits(r)), g.size, what)


def check(ctxs, cloud, normals, cam, w, h, modes=MODES, **kw):
    """the operator against the restatement, every output, every element"""
    ref = cloud_render_oriented_ref(cloud, normals, cam[0], cam[1], cam[2], w, h, **kw)
    assert not ref["refused"]
    for name, on_device, where in modes:
        c, nr = (records(cloud, normals), "record") if where == "record" else (np.ascontiguousarray(cloud[:, :3]), np.ascontiguousarray(normals[:, :3]))
        if on_device:
            c, nr = torch.from_numpy(c).cuda(), nr if where == "record" else torch.from_numpy(nr).cuda()
        r = api.cloud_render(c, cam[0], cam[1], cam[2], w, h, want=PLANES, matcher=ctxs[name], normals=nr, **kw)
        assert all(torch.is_tensor(r[k]) and r[k].is_cuda for k in PLANES) if on_device else all(isinstance(r[k], np.ndarray) for k in PLANES)
        same(r, ref, "%s, device %s, normals %s, %s" % (name, on_device, where, kw))
    return ref


# ---- the render ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0, 2, 4])
def test_the_slanted_scene(ctxs, slope):
    cloud, K, R, t = slanted_scene(slope)
    ref = check(ctxs, cloud[:, :3], cloud[:, 3:6], (K, R, t), SLANT_W, SLANT_H, radius=F(3 * slant_spacing(slope)), max_px=16)
    assert 0 < ref["n_covered"] < ref["n_splats"] and ref["landed"].mean() > 0.7
    one = cloud_render_ref(cloud[:, :3], K, R, t, SLANT_W, SLANT_H, max_px=16)
    fg = (one["index"] >= 0) & (one["index"] < 6000)
    assert fg.sum() > 1900 and np.count_nonzero(fg & (ref["depth"] == 0)) <= fg.sum() / 100         # the surface does not hide itself


def test_the_scene_cloud_with_normals_estimated_on_the_gpu(ctxs):
    sc, _, spacing = scene()
    thin = thinned_cloud()
    nrm = api.cloud_normals(thin, radius=F(8 * spacing), k=16, want=("normal",), matcher=ctxs["fast"])
    assert nrm["n_normals"] > 0.9 * len(thin)
    cam = (sc.K[0], sc.R[0], sc.t[0])
    ref = check(ctxs, thin, nrm["normal"], cam, sc.w, sc.h, radius=F(3 * spacing), min_points=2, depth_diff=0.002)
    assert 0 < ref["n_covered"] < ref["n_splats"] and ref["count"].max() > 1
    # the normals stay on the device from one operator to the next
    dev = torch.from_numpy(thin).cuda()
    on = api.cloud_normals(dev, radius=F(8 * spacing), k=16, want=("normal",), matcher=ctxs["fast"])["normal"]
    r = api.cloud_render(dev, *cam, sc.w, sc.h, radius=F(3 * spacing), min_points=2, depth_diff=0.002, want=PLANES, normals=on, matcher=ctxs["fast"])
    same(r, ref, "normals from the device")


def test_normals_that_orient_nothing_give_the_square_render(ctxs):
    """a differential against the entry that is tested already: tsar_cloud_render itself"""
    sc, cloud, spacing = scene()
    cam = (sc.K[0], sc.R[0], sc.t[0])
    for radius in (0.0, F(1.5 * spacing), F(3 * spacing)):
        kw = dict(radius=radius, min_points=2, depth_diff=0.002)
        sq = api.cloud_render(cloud, *cam, sc.w, sc.h, want=("depth", "count", "index"), matcher=ctxs["strict"], **kw)
        for nrm in (np.zeros_like(cloud), np.full_like(cloud, np.nan)):
            r = api.cloud_render(cloud, *cam, sc.w, sc.h, want=PLANES, matcher=ctxs["strict"], normals=nrm, **kw)
            assert r["n_splats"] == sq["n_splats"] == r["n_covered"]
            assert all(np.array_equal(r[k].view(np.uint32) if k == "depth" else r[k], sq[k].view(np.uint32) if k == "depth" else sq[k]) for k in ("depth", "count", "index"))
            assert np.array_equal(r["occluder"] > 0, cloud_render_ref(cloud, *cam, sc.w, sc.h, radius=radius)["Zo"] > 0)


def test_an_image_wider_than_one_row_of_lanes_and_degenerate_images(ctxs):
    rng = np.random.default_rng(1)
    cam = camera(67, 45)
    cloud, nrm = random_cloud(rng, 20000, cam, 67, 45), random_normals(rng, 20000)
    ref = check(ctxs, cloud, nrm, cam, 67, 45, radius=0.4, max_px=5, min_points=2, depth_diff=0.05)
    assert ref["landed"].mean() > 0.99 and 0 < np.count_nonzero(ref["depth"]) < 67 * 45 and ref["count"].max() > 3 and ref["n_covered"] < ref["n_splats"]
    check(ctxs, cloud, nrm, cam, 67, 45, modes=MODES[:2])                    # radius 0: the one-pixel render
    check(ctxs, cloud, nrm, cam, 1, 1, radius=0.05, modes=MODES[:2])
    check(ctxs, cloud, nrm, cam, 300, 2, radius=0.05, max_px=16, modes=MODES[:2])


def test_contention_on_one_pixel(ctxs):
    rng = np.random.default_rng(2)
    cam = camera(33, 21)
    z = rng.permutation(np.linspace(4.0, 6.0, 200))
    cloud = points_at(cam, np.full(200, 16.0), np.full(200, 10.0), z)
    nrm = rng.normal(size=(200, 3)).astype(F)
    lands, xi, yi, p2, _ = landings(cloud, cam[0], cam[1], cam[2], 33, 21)
    assert lands.all() and (xi == 16).all() and (yi == 10).all() and len(np.unique(p2)) > 190
    ref = check(ctxs, cloud, nrm, cam, 33, 21, radius=0.5, depth_diff=0.1, max_px=8)
    assert ref["index"][10, 16] == int(np.argmin(p2)) and ref["support"][10, 16] > 20 and ref["occluder"][10, 16] <= ref["depth"][10, 16]
    assert len(np.unique(ref["occluder"][ref["occluder"] > 0])) > 5           # discs of many orientations meet the neighbouring rays at many depths


def test_maximal_footprints_on_every_border_pixel_with_tilted_normals(ctxs):
    w, h = 40, 33
    cam = camera(w, h)
    border = [(u, v) for u in range(w) for v in (0, h - 1)] + [(u, v) for v in range(1, h - 1) for u in (0, w - 1)]
    rng = np.random.default_rng(3)
    u, v = np.array(border, np.float64).T
    cloud = points_at(cam, u, v, rng.uniform(4.0, 6.0, len(border)))
    nrm = (np.asarray(cam[1], np.float64).T @ np.stack([rng.uniform(-1, 1, len(border)), rng.uniform(-1, 1, len(border)), np.ones(len(border))])).T.astype(F)   # up to 55 degrees off the axis
    ref = check(ctxs, cloud, nrm, cam, w, h, radius=10.0, max_px=16)
    lands, xi, yi, _, s = landings(cloud, cam[0], cam[1], cam[2], w, h, radius=10.0, max_px=16)
    assert lands.all() and (s == 16).all() and len(set(zip(xi.tolist(), yi.tolist()))) == len(border)
    assert ref["n_splats"] < 33 * 33 * len(border) and 0 < ref["n_covered"] <= ref["n_splats"]               # clipped squares under discs wider than them
    check(ctxs, cloud, nrm, cam, w, h, radius=10.0, max_px=1, modes=MODES[:2])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_point_counts(ctxs, n):
    rng = np.random.default_rng(100 + n)
    cam = camera(50, 37)
    cloud, nrm = random_cloud(rng, n, cam, 50, 37), random_normals(rng, n)
    ref = check(ctxs, cloud, nrm, cam, 50, 37, radius=0.3)
    assert (n == 0) == (ref["n_splats"] == 0) and (n == 0) == (ref["n_covered"] == 0)
    own = api.cloud_render(cloud, cam[0], cam[1], cam[2], 50, 37, radius=0.3, want=PLANES, normals=nrm)      # a context of the call's own
    same(own, ref, "context-free")


def test_a_shuffled_cloud_and_two_runs(ctxs):
    cloud, K, R, t = slanted_scene(2)
    kw = dict(radius=F(3 * slant_spacing(2)), max_px=16, want=PLANES, normals="record")
    a = api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, matcher=ctxs["fast"], **kw)
    b = api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, matcher=ctxs["fast"], **kw)
    d = api.cloud_render(torch.from_numpy(cloud).cuda(), K, R, t, SLANT_W, SLANT_H, matcher=ctxs["strict"], **kw)
    for r in (b, d):
        same(r, a, "a second run")
    perm = np.random.default_rng(4).permutation(len(cloud))
    s = api.cloud_render(np.ascontiguousarray(cloud[perm]), K, R, t, SLANT_W, SLANT_H, matcher=ctxs["fast"], **kw)
    same(s, a, "shuffled", planes=("depth", "count", "occluder"))
    kept = a["index"] >= 0
    p2 = landings(cloud[:, :3], K, R, t, SLANT_W, SLANT_H)[3]
    assert np.array_equal(s["index"] >= 0, kept) and kept.sum() > 10000 and np.array_equal(p2[perm[s["index"][kept]]], p2[a["index"][kept]])


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from cloud_splat_ref import SLANT_H, SLANT_W, slant_spacing, slanted_scene
from tsar_mvs_amd import api
cloud, K, R, t = slanted_scene(2)
r = api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, radius=np.float32(3 * slant_spacing(2)), max_px=16, want=("depth", "count", "index", "occluder"), normals="record")
np.savez(sys.argv[1], **r)
"""


def test_without_the_skipping_load_the_bits_are_the_same(ctxs, tmp_path):
    cloud, K, R, t = slanted_scene(2)
    a = api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, radius=F(3 * slant_spacing(2)), max_px=16, want=PLANES, normals="record", matcher=ctxs["fast"])
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(tmp_path / "r.npz")], env=dict(os.environ, TSAR_RENDER_SKIP="0"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    b = dict(np.load(str(tmp_path / "r.npz")))
    same({k: (int(v) if v.ndim == 0 else v) for k, v in b.items()}, a, "TSAR_RENDER_SKIP=0")


def test_want_names_the_outputs(ctxs):
    rng = np.random.default_rng(5)
    cam = camera(50, 37)
    cloud, nrm = random_cloud(rng, 5000, cam, 50, 37), random_normals(rng, 5000)
    ref = cloud_render_oriented_ref(cloud, nrm, *cam, 50, 37, radius=0.3, min_points=2)
    for want in (("depth",), ("index",), ("count",), ("occluder",), ("depth", "occluder")):
        r = api.cloud_render(cloud, *cam, 50, 37, radius=0.3, min_points=2, want=want, matcher=ctxs["fast"], normals=nrm)
        assert sorted(r) == sorted(want + ("n_splats", "n_covered")) and all(np.array_equal(r[k], ref[k]) for k in want)
    with pytest.raises(AssertionError):
        api.cloud_render(cloud, *cam, 50, 37, radius=0.3, want=("occluder",), matcher=ctxs["fast"])         # the square render has no such plane
    assert sorted(api.cloud_render(cloud, *cam, 50, 37, radius=0.3, matcher=ctxs["fast"])) == ["count", "depth", "n_splats"]      # and its result is what it was


def raw_render(m, cloud, normals, cam, w, h, on_device=False, **fields):
    c, nr = np.ascontiguousarray(cloud, F), np.ascontiguousarray(normals, F)
    bufs = [np.full((h, w), -7, F), np.full((h, w), 77, np.uint8), np.full((h, w), -7, np.int32), np.full((h, w), -7, F)]
    if on_device:
        c, nr, bufs = torch.from_numpy(c).cuda(), torch.from_numpy(nr).cuda(), [torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
    ptr = (lambda a: C.c_void_p(a.data_ptr())) if on_device else (lambda a: a.ctypes.data_as(C.c_void_p))
    p = api.CloudRenderParams()
    m.L.tsar_default_cloud_render_params(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    n_splats, n_covered = C.c_int64(-1), C.c_int64(-1)
    rc = m.L.tsar_cloud_render_oriented_ctx(m._ctx, ptr(c), len(c), c.shape[1], ptr(nr), nr.shape[1], api._cameras(cam[0][None], cam[1][None], cam[2][None], 1), w, h,
                                            C.byref(p), *(ptr(b) for b in bufs), C.byref(n_splats), C.byref(n_covered), api.MEM_DEVICE if on_device else api.MEM_HOST)
    return rc, m.L.tsar_last_error(m._ctx).decode(), n_splats.value, n_covered.value, [host(b) for b in bufs]


@pytest.mark.parametrize("on_device", [False, True])
def test_max_splats_refuses_before_anything_is_written(ctxs, on_device):
    rng = np.random.default_rng(6)
    cam = camera(50, 37)
    cloud, nrm = random_cloud(rng, 3000, cam, 50, 37), random_normals(rng, 3000)
    ref = cloud_render_oriented_ref(cloud, nrm, *cam, 50, 37, radius=0.3)
    rc, msg, got, covered, bufs = raw_render(ctxs["fast"], cloud, nrm, cam, 50, 37, on_device, radius=0.3, max_splats=ref["n_splats"] - 1)
    assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_render_oriented:") and "max_splats" in msg and got == ref["n_splats"] and covered == -1
    assert (bufs[0] == -7).all() and (bufs[1] == 77).all() and (bufs[2] == -7).all() and (bufs[3] == -7).all()
    rc, _, got, covered, bufs = raw_render(ctxs["fast"], cloud, nrm, cam, 50, 37, on_device, radius=0.3, max_splats=ref["n_splats"])
    assert rc == api.TSAR_OK and (got, covered) == (ref["n_splats"], ref["n_covered"]) and (bufs[1] != 77).any() and ref["n_covered"] < ref["n_splats"]
    with pytest.raises(api.TsarError) as e:
        api.cloud_render(cloud, *cam, 50, 37, radius=0.3, max_splats=10, matcher=ctxs["strict"], normals=nrm)
    assert e.value.code == api.TSAR_ERR_INVALID and e.value.n_splats == ref["n_splats"]


def test_every_refusal_and_the_context_works_afterwards(ctxs):
    m = ctxs["strict"]
    L = m.L
    rng = np.random.default_rng(7)
    cam = camera(50, 37)
    cloud, nrm = random_cloud(rng, 500, cam, 50, 37), random_normals(rng, 500)
    cp, nrp = cloud.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)
    out = np.full(50 * 37, -7, np.int32)
    op = out.ctypes.data_as(C.c_void_p)
    cams = api._cameras(cam[0][None], cam[1][None], cam[2][None], 1)

    def params(**fields):
        p = api.CloudRenderParams()
        L.tsar_default_cloud_render_params(C.byref(p))
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def refused(fragment, c=cp, n=500, stride=3, nr=nrp, nstride=3, camera_=cams, w=50, h=37, prm=params(), outs=(op, None, None, None), mem=api.MEM_HOST):
        rc = L.tsar_cloud_render_oriented_ctx(m._ctx, c, n, stride, nr, nstride, camera_, w, h, C.byref(prm) if prm is not None else None, *outs, None, None, mem)
        msg = L.tsar_last_error(m._ctx).decode()
        assert rc == api.TSAR_ERR_INVALID and msg.startswith("tsar_cloud_render_oriented:") and fragment in msg, (rc, msg)
        assert (out == -7).all()                                              # a refused call writes nothing

    refused("params is NULL", prm=None)
    refused("cam is NULL", camera_=None)
    refused("mem must be", mem=7)
    refused("n must be", n=-1)
    refused("n must be", n=1 << 31)
    refused("stride", stride=2)
    refused("cloud is NULL", c=None)
    refused("all NULL", outs=(None, None, None, None))
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
    refused("examine", prm=params(max_splats=3, radius=0.3))
    # the oriented entry's own
    refused("the stride must be at least 6", nr=None, nstride=0)
    refused("the stride must be at least 6", nr=None, nstride=0, stride=5)
    refused("normal_stride must be at least 3", nstride=2)
    singular = api._cameras(cam[0][None], np.zeros((1, 3, 3), F), cam[2][None], 1)
    refused("singular", camera_=singular)
    flat = np.array(cam[0], F)
    flat[1] = flat[0]                                                         # two equal rows of K: det (K R) == 0 or next to it
    flat[2] = [0, 0, 1e-39]
    refused("singular", camera_=api._cameras(flat[None], cam[1][None], cam[2][None], 1))
    # what is allowed: only the occluder plane; a radius of 0
    occ = np.full((37, 50), -7, F)
    rc = L.tsar_cloud_render_oriented_ctx(m._ctx, cp, 500, 3, nrp, 3, cams, 50, 37, C.byref(params(radius=0.3)), None, None, None, occ.ctypes.data_as(C.c_void_p), None, None,
                                          api.MEM_HOST)
    assert rc == api.TSAR_OK and np.array_equal(occ, cloud_render_oriented_ref(cloud, nrm, *cam, 50, 37, radius=0.3)["occluder"])
    with pytest.raises(api.TsarError):
        api.cloud_render(cloud, *cam, 50, 37, matcher=m, normals="record")                                   # records of three floats hold no normal
    with pytest.raises(AssertionError):
        api.cloud_render(cloud, *cam, 50, 37, matcher=m, normals=nrm[:-1])
    with pytest.raises(AssertionError):
        api.cloud_render(cloud, *cam, 50, 37, matcher=m, normals="records")
    check(ctxs, cloud, nrm, cam, 50, 37, radius=0.3)                          # and the contexts still work


def test_the_contexts_are_left_as_they_were(ctxs):
    """get_plane before and after is bit-equal, after calls that succeed and calls that are refused, and the matcher goes on"""
    cloud, K, R, t = slanted_scene(2)
    bits = lambda planes: [np.asarray(a).view(np.uint32).copy() for a in planes]
    for m in ctxs.values():
        before = bits(m.get_plane())
        api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, radius=F(3 * slant_spacing(2)), max_px=16, matcher=m, normals="record")
        api.cloud_render(torch.from_numpy(cloud).cuda(), K, R, t, SLANT_W, SLANT_H, matcher=m, normals="record")
        with pytest.raises(api.TsarError):
            api.cloud_render(cloud, K, R, t, SLANT_W, SLANT_H, radius=1.0, max_splats=5, matcher=m, normals="record")
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(m.get_plane())))
        m.pm_iterate(1)


# ---- use -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps_and_normals():
    """scene()'s ground-truth maps of views 0 and 1 with noise and holes, the thinned cloud, and normals of every kind for it"""
    sc, _, spacing = scene()
    rng = np.random.default_rng(3)
    maps = []
    for v in (0, 1):
        d = sc.meta["gt_all"][v][0].numpy().astype(F)
        d = (d * (1 + rng.normal(scale=2e-3, size=d.shape))).astype(F)
        d[rng.random(d.shape) < 0.05] = 0
        maps.append(d)
    thin = thinned_cloud()
    nrm = rng.normal(size=(len(thin), 3)).astype(F)
    nrm[::5] = 0
    return sc, maps, thin, nrm, F(3 * spacing)


def composition(sc, maps, thin, nrm, radius, tol, **kw):
    views = []
    for v, d in enumerate(maps):
        r = cloud_render_oriented_ref(thin, nrm, sc.K[v], sc.R[v], sc.t[v], d.shape[1], d.shape[0], radius, **kw)
        c = depth_compare_ref(d, r["depth"], tol)
        c.update(n_splats=r["n_splats"], n_covered=r["n_covered"])
        views.append(c)
    total = {k: sum(c[k] for c in views) for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered")}
    total["within"] = np.sum([c["within"] for c in views], axis=0).astype(np.int64)
    return views, total


def same_counts(got, ref):
    for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered"):
        assert got[k] == ref[k], k
    assert list(got["within"]) == ref["within"].tolist()
    q = ratios(ref)
    assert list(got["accuracy"]) == q["accuracy"].tolist() and list(got["completeness"]) == q["completeness"].tolist() and got["cover"] == q["cover"]


def test_evaluate_depth_maps_with_normals_equals_the_composition(maps_and_normals, ctxs):
    sc, maps, thin, nrm, radius = maps_and_normals
    tol = [0.001, 0.01]
    views_ref, total_ref = composition(sc, maps, thin, nrm, radius, tol, max_px=4)
    views, total = api.evaluate_depth_maps(maps, thin, sc.K[:2], sc.R[:2], sc.t[:2], tol, radius, matcher=ctxs["fast"], normals=nrm, max_px=4)
    for got, ref in zip(views, views_ref):
        same_counts(got, ref)
    same_counts(total, total_ref)
    assert 0 < total_ref["within"][0] < total_ref["within"][1] <= total_ref["n_both"] < total_ref["n_gt"] and 0 < total_ref["n_covered"] < total_ref["n_splats"]
    views, total = api.evaluate_depth_maps(maps, torch.from_numpy(records(thin, nrm)).cuda(), sc.K[:2], sc.R[:2], sc.t[:2], tol, radius, normals="record", max_px=4)
    same_counts(total, total_ref)
    _, square = api.evaluate_depth_maps(maps, thin, sc.K[:2], sc.R[:2], sc.t[:2], tol, radius, matcher=ctxs["fast"], max_px=4)
    assert "n_covered" not in square and square["n_splats"] == total_ref["n_splats"]


def test_the_built_tool_equals_evaluate_depth_maps(maps_and_normals, tmp_path):
    sc, maps, thin, nrm, radius = maps_and_normals
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    for v, d in enumerate(maps):
        os.makedirs(root + "APD/%08d" % v)
        tio.write_dmb(root + "APD/%08d/TSAR_disp.dmb" % v, d)
    tio.write_ply(root + "gt.ply", thin, normals=nrm)
    tool = os.path.join(ROOT, "tsar-mvs_amd", "tsar_evaluate_maps")
    args = [tool, root, root + "gt.ply", "--tolerances=0.001,0.01", "--radius=%.9g" % radius, "--views=0,1", "--oriented"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    views, total = api.evaluate_depth_maps(maps, thin, sc.K[:2], sc.R[:2], sc.t[:2], [0.001, 0.01], radius, normals=nrm)
    assert rec["oriented"] is True and [v["id"] for v in rec["views"]] == [0, 1]
    for got, want in zip(rec["views"] + [rec["total"]], views + [total]):
        for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered", "cover"):
            assert got[k] == want[k], k
        assert got["within"] == want["within"].tolist() and got["accuracy"] == want["accuracy"].tolist()
    # normals estimated by the tool, once, on the device: what api.cloud_normals gives
    k, nradius = 12, F(8 * float(radius) / 3)
    out = subprocess.run(args + ["--normals=%d" % k, "--normal_radius=%.9g" % nradius, "--normal_min_neighbors=4"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    est = api.cloud_normals(thin, radius=nradius, k=k, min_neighbors=4, want=("normal",))
    _, total = api.evaluate_depth_maps(maps, thin, sc.K[:2], sc.R[:2], sc.t[:2], [0.001, 0.01], radius, normals=est["normal"])
    assert rec["n_gt_normals"] == est["n_normals"] > 0 and (rec["normals"]["k"], F(rec["normals"]["radius"]), rec["normals"]["min_neighbors"]) == (k, nradius, 4)
    for key in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered"):
        assert rec["total"][key] == total[key], key

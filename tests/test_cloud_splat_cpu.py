"""tsar_cloud_render_oriented without a GPU: the numpy restatement (tests/cloud_splat_ref.py) held to answers computed by hand and, with
normals that orient nothing, to cloud_render_ref; what the oriented occluder is for, on the slanted scene; the brute-force host stand-in
(tests/cli_stub/tsar_stub_splat.cpp) held to the restatement through ctypes; and host/tsar_evaluate_maps.cpp --oriented, linked against the
stand-in: its JSON equals the restatement's composition, the refusals, and the output without the switch."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_render_ref import cloud_render_ref, depth_compare_ref, evaluate_depth_maps_ref, ratios, scene, thinned_cloud
from cloud_splat_ref import (SLANT_H, SLANT_N_FG, SLANT_W, cloud_render_oriented_ref, slant_figures, slant_spacing, slanted_scene, splat_view)
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate_maps.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_splat.cpp")
OLD_STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_render.cpp")
F = np.float32
PLANES = ("depth", "count", "index", "occluder")

# test_cloud_render_cpu.py's camera: f = 8, principal point (4, 3), identity pose, 9 x 7 pixels.  The ray of pixel (u, v) is
# ((u - 4) / 8, (v - 3) / 8, 1): M = [[1/8, 0, -1/2], [0, 1/8, -3/8], [0, 0, 1]] and C = 0, all exact in float32
W, H = 9, 7
K = np.array([[8, 0, 4], [0, 8, 3], [0, 0, 1]], F)
R = np.eye(3, dtype=F)
T = np.zeros(3, F)


def at(u, v, Z):
    return [(u - 4) * Z / 8, (v - 3) * Z / 8, Z]


def render(pts, normals, **kw):
    return cloud_render_oriented_ref(np.array(pts, F).reshape(-1, 3), np.array(normals, F).reshape(-1, 3), K, R, T, W, H, **kw)


def same_planes(got, ref, planes=PLANES):
    for k in planes:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b), k


# ---- known answers -----------------------------------------------------------------------------------------------------------------------
def test_the_host_side_inverts_k_r():
    M, Cc = splat_view(K, R, T)
    assert np.array_equal(M, np.array([[0.125, 0, -0.5], [0, 0.125, -0.375], [0, 0, 1]], F)) and np.array_equal(Cc, np.zeros(3, F))
    rng = np.random.default_rng(0)
    Kr, Rr, tr = (rng.random((3, 3)) + np.eye(3)).astype(F), (rng.random((3, 3)) + np.eye(3)).astype(F), rng.random(3).astype(F)
    M, Cc = splat_view(Kr, Rr, tr)
    assert M.dtype == F and Cc.dtype == F
    assert np.allclose(M, np.linalg.inv(Kr.astype(np.float64) @ Rr.astype(np.float64)), rtol=1e-5, atol=1e-6)
    assert np.allclose(Cc, -Rr.astype(np.float64).T @ tr.astype(np.float64), rtol=1e-6)
    assert splat_view(Kr, np.zeros((3, 3), F), tr) is None                     # det == 0
    assert splat_view(np.diag([1e-39, 1, 1]).astype(F), np.eye(3, dtype=F), tr) is None                     # M[0][0] = 1e39 is no float32


def test_a_frontal_disc_covers_the_pixels_within_radius_at_p2():
    """fr = 4, s = 2: the square is 5 x 5.  z = 2 on every ray, the ray's point is ((u - 4) / 4, (v - 3) / 4, 2): q = (du^2 + dv^2) / 16
    against r2 = 1/4 keeps du^2 + dv^2 <= 4, the 13 pixels within two pixels of the centre, the corners of the 3 x 3 included"""
    r = render([at(4, 3, 2.0)], [[0, 0, 1]], radius=0.5)
    v, u = np.mgrid[0:H, 0:W]
    want = (u - 4) ** 2 + (v - 3) ** 2 <= 4
    assert want.sum() == 13 and np.array_equal(np.isfinite(r["Zo"]), want) and (r["Zo"][want] == 2.0).all()
    assert np.array_equal(r["occluder"], np.where(want, F(2), F(0)))
    assert r["n_covered"] == 13 and r["n_splats"] == 25 and r["depth"][3, 4] == 2.0 and np.count_nonzero(r["depth"]) == 1
    # the square allows less than the disc asks for: max_px cuts it
    r = render([at(4, 3, 2.0)], [[0, 0, 1]], radius=0.5, max_px=1)
    assert r["n_covered"] == 9 and r["n_splats"] == 9


def test_a_disc_tilted_about_the_vertical_axis_narrows_and_follows_its_plane():
    """n = (1, 0, 1) at (0, 0, 2): the plane x + z = 2 meets the ray of pixel u at z = 2 / (u / 8 + 1 / 2) = 16 / (u + 4).  With r2 = 1 / 4:
    u = 5: z = 16/9, e = (2/9, ., -2/9), q = 8/81 covers;  u = 6: z = 1.6, q = 0.32 does not;  u = 3: z = 16/7, q = 8/49 covers;  u = 2: not.
    Along the axis the disc keeps its width: v = 3 +- 2 gives e_1 = +-1/2, q = 1/4 = r2 exactly"""
    r = render([at(4, 3, 2.0)], [[1, 0, 1]], radius=0.5)
    Zo = r["Zo"]
    assert np.isfinite(Zo[3]).tolist() == [False, False, False, True, True, True, False, False, False]
    assert np.isfinite(Zo[:, 4]).tolist() == [False, True, True, True, True, True, False]
    assert Zo[3, 4] == 2.0 and Zo[3, 5] == F(2) / (F(0.125) * F(5) + F(0.5)) and Zo[3, 3] == F(2) / (F(0.125) * F(3) + F(0.5))
    assert abs(float(Zo[3, 5]) - 16 / 9) < 1e-6 and abs(float(Zo[3, 3]) - 16 / 7) < 1e-6 and (Zo[[1, 2, 4, 5], 4] == 2.0).all()
    frontal = render([at(4, 3, 2.0)], [[0, 0, 1]], radius=0.5)
    assert np.isfinite(frontal["Zo"][3]).sum() == 5 and r["n_covered"] < frontal["n_covered"]
    # a neighbour on the plane is seen, one on the frontal plane through the point is hidden by the nearer disc: 0.22 > 0.02 * 16/9
    on_plane, frontal_pt = at(5, 3, 16 / 9), at(5, 3, 2.0)
    assert render([at(4, 3, 2.0), on_plane], [[1, 0, 1]] * 2, radius=0.5)["depth"][3, 5] == F(16 / 9)
    assert render([at(4, 3, 2.0), frontal_pt], [[1, 0, 1], [0, 0, 0]], radius=0.5)["depth"][3, 5] == 0
    assert render([at(4, 3, 2.0), frontal_pt], [[0, 0, 1], [0, 0, 1]], radius=0.5)["depth"][3, 5] == 2.0


def test_rays_along_the_plane_and_planes_behind_the_camera_do_not_cover():
    """n = (8, 0, -1) at (0, 0, 2): g = (1, 0, -5), num = -2, den = u - 5.  u = 5: den == 0, z = -inf;  u = 6: z = -2, behind the camera;
    u = 3: z = 1, the ray's point (-1/8, ., 1) is 1.008 from the point: outside the disc;  u = 4: den = -1, z = 2: the centre's column lies in
    the plane, and its five pixels of the square are within the radius.  Nothing else covers"""
    r = render([at(4, 3, 2.0)], [[8, 0, -1]], radius=0.5)
    want = np.zeros((H, W), bool)
    want[1:6, 4] = True
    assert r["n_covered"] == 5 and np.array_equal(np.isfinite(r["Zo"]), want) and (r["Zo"][want] == 2.0).all() and r["n_splats"] == 25
    # 0 / 0: the plane through the camera centre, on the ray it contains
    r = render([at(4, 3, 2.0)], [[1, 0, 0]], radius=0.5)                      # num = 0, den = (u - 4) / 8: z = 0 off the centre column, NaN on it
    assert r["n_covered"] == 1
    # a large radius does not help a ray that misses the plane in front of the camera
    r = render([at(4, 3, 2.0)], [[8, 0, -1]], radius=50.0, max_px=16)
    assert np.isnan(r["Zo"][3, 5:]).all() and r["Zo"][3, 3] == 1.0 and r["Zo"][3, 4] == 2.0


def test_the_sign_of_the_normal_does_not_matter():
    cloud, Kc, Rc, tc = slanted_scene(2)
    rng = np.random.default_rng(1)
    nrm = rng.normal(size=(len(cloud), 3)).astype(F)
    kw = dict(radius=F(3 * slant_spacing(2)), max_px=16)
    a = cloud_render_oriented_ref(cloud[:, :3], nrm, Kc, Rc, tc, SLANT_W, SLANT_H, **kw)
    b = cloud_render_oriented_ref(cloud[:, :3], -nrm, Kc, Rc, tc, SLANT_W, SLANT_H, **kw)
    same_planes(a, b)
    assert a["n_covered"] == b["n_covered"] and 0 < a["n_covered"] < a["n_splats"]


@pytest.mark.parametrize("bad", [[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 1], [1, 0, -np.inf], [-0.0, 0.0, -0.0]])
def test_a_normal_that_orients_nothing_covers_the_square_at_p2(bad):
    pts = [at(4, 3, 2.0), at(0, 0, 3.0), at(5, 3, 2.05)]
    got = render(pts, [bad] * 3, radius=0.5)
    ref = cloud_render_ref(np.array(pts, F), K, R, T, W, H, radius=0.5)
    same_planes(got, ref, ("depth", "count", "index"))
    assert np.array_equal(got["Zo"].view(np.uint32), ref["Zo"].view(np.uint32)) and got["n_covered"] == got["n_splats"] == ref["n_splats"] == 25 + 4 + 25


@pytest.mark.parametrize("spacings", [1.5, 3.0])
def test_with_zero_normals_every_plane_is_the_square_render(spacings):
    sc, cloud, spacing = scene()
    kw = dict(radius=F(spacings * spacing), max_px=8, min_points=2, depth_diff=0.002)
    got = cloud_render_oriented_ref(cloud, np.zeros_like(cloud), sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw)
    ref = cloud_render_ref(cloud, sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw)
    same_planes(got, ref, ("depth", "count", "index", "Zc", "Zo", "visible", "support"))
    assert got["n_splats"] == ref["n_splats"] == got["n_covered"]
    assert np.array_equal(got["occluder"], np.where(np.isfinite(ref["Zo"]), ref["Zo"], 0))


def test_radius_zero_is_the_one_pixel_render():
    cloud, Kc, Rc, tc = slanted_scene(2)
    got = cloud_render_oriented_ref(cloud, None, Kc, Rc, tc, SLANT_W, SLANT_H, radius=0.0)
    ref = cloud_render_ref(cloud[:, :3], Kc, Rc, tc, SLANT_W, SLANT_H, radius=0.0)
    same_planes(got, ref, ("depth", "count", "index"))
    assert got["n_covered"] == got["n_splats"] == ref["n_splats"] and np.array_equal(got["occluder"], np.where(ref["landed"], ref["Zc"], 0))


def test_a_refused_max_splats():
    pts, nrm = [at(4, 3, 2.0), at(0, 0, 2.0)], [[0, 0, 1]] * 2
    assert render(pts, nrm, radius=0.5)["n_splats"] == 25 + 9
    assert render(pts, nrm, radius=0.5, max_splats=33) == {"n_splats": 34, "refused": True}
    assert not render(pts, nrm, radius=0.5, max_splats=34)["refused"]


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------
def slant_renders(slope):
    cloud, Kc, Rc, tc = slanted_scene(slope)
    kw = dict(max_px=16, occlusion_diff=0.02)
    radius = F(3 * slant_spacing(slope))
    one = cloud_render_ref(cloud[:, :3], Kc, Rc, tc, SLANT_W, SLANT_H, radius=0.0, **kw)
    square = cloud_render_ref(cloud[:, :3], Kc, Rc, tc, SLANT_W, SLANT_H, radius=radius, **kw)
    oriented = cloud_render_oriented_ref(cloud, None, Kc, Rc, tc, SLANT_W, SLANT_H, radius=radius, **kw)
    return one, square, oriented


def test_a_slanted_surface_hides_itself_behind_squares_and_not_behind_discs():
    """At slope 2 and a radius of 3 point spacings, measured with the two restatements (the camera is rotated, translated and skewed):
    2036 foreground pixels; the square render hides 1919 of them, the oriented render 0; inside the analytic silhouette the one-pixel render
    shows 223 background pixels, both footprints 0.  The bars: at least half hidden by the square, at most 1 % by the disc,
    and no more background through the disc than through the square"""
    one, square, oriented = slant_renders(2)
    fg, hidden_sq, through_sq = slant_figures(one, square, 2)
    _, hidden_or, through_or = slant_figures(one, oriented, 2)
    _, _, through_one = slant_figures(one, one, 2)
    print("slope 2, radius 3 spacings: %d foreground pixels; hidden by the square render %d, by the oriented render %d; background inside the silhouette: one-pixel %d, "
          "square %d, oriented %d; n_covered / n_splats = %d / %d" % (fg, hidden_sq, hidden_or, through_one, through_sq, through_or, oriented["n_covered"], oriented["n_splats"]))
    assert fg >= 1900 and through_one >= 100                                   # the case says something
    assert hidden_sq >= fg / 2
    assert hidden_or <= fg / 100
    assert through_or <= through_sq
    assert oriented["n_covered"] < oriented["n_splats"] and oriented["n_splats"] == square["n_splats"]


@pytest.mark.parametrize("slope", [0, 4])
def test_the_other_slopes(slope):
    one, square, oriented = slant_renders(slope)
    fg, hidden_sq, through_sq = slant_figures(one, square, slope)
    _, hidden_or, through_or = slant_figures(one, oriented, slope)
    print("slope %d: %d foreground pixels; hidden %d / %d; background inside the silhouette %d / %d" % (slope, fg, hidden_sq, hidden_or, through_sq, through_or))
    assert hidden_or <= fg / 100 and through_or <= through_sq
    assert hidden_sq == 0 if slope == 0 else hidden_sq >= fg / 2


# ---- the stand-in against the restatement, and the tool ------------------------------------------------------------------------------------
class Params(C.Structure):
    _fields_ = [("radius", C.c_float), ("max_px", C.c_int32), ("occlusion_diff", C.c_float), ("depth_diff", C.c_float), ("min_points", C.c_int32), ("max_splats", C.c_int64)]


class Camera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3)]


def build(d, stub):
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", stub],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate_maps", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_splat")), STUB)


@pytest.fixture(scope="module")
def built_old(tmp_path_factory):
    """the tool against a library from before the entry: the square render's stand-in"""
    return build(str(tmp_path_factory.mktemp("cli_stub_render_old")), OLD_STUB)


def stub_render(lib, cloud, normals, Kv, Rv, tv, w, h, **kw):
    L = C.CDLL(lib)
    L.tsar_last_error.restype = C.c_char_p
    ctx = C.c_void_p()
    assert L.tsar_create(0, C.byref(ctx)) == 0
    p = Params()
    L.tsar_default_cloud_render_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    cam = Camera.from_buffer_copy(np.concatenate([np.asarray(Kv, F).reshape(-1), np.asarray(Rv, F).reshape(-1), np.asarray(tv, F).reshape(-1)]).tobytes())
    c = np.ascontiguousarray(cloud, F)
    nr = None if normals is None else np.ascontiguousarray(normals, F)
    res = {"depth": np.full((h, w), -7, F), "count": np.full((h, w), 77, np.uint8), "index": np.full((h, w), -7, np.int32), "occluder": np.full((h, w), -7, F)}
    n_splats, n_covered = C.c_int64(-1), C.c_int64(-1)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.tsar_cloud_render_oriented_ctx(ctx, ptr(c), C.c_int64(len(c)), c.shape[1], ptr(nr), 0 if nr is None else nr.shape[1], C.byref(cam), w, h, C.byref(p),
                                          *(ptr(res[k]) for k in PLANES), C.byref(n_splats), C.byref(n_covered), 0)
    msg = L.tsar_last_error(ctx).decode()
    L.tsar_destroy(ctx)
    res.update(n_splats=n_splats.value, n_covered=n_covered.value)
    return rc, msg, res


def mixed_normals(n, seed):
    """random directions, every fifth one zero and every seventh one NaN"""
    nrm = np.random.default_rng(seed).normal(size=(n, 3)).astype(F)
    nrm[::5] = 0
    nrm[::7, 1] = np.nan
    return nrm


def test_the_stand_in_equals_the_restatement(built):
    lib = built + "/libtsar_hip.so"
    for slope in (0, 2, 4):
        cloud, Kc, Rc, tc = slanted_scene(slope)
        kw = dict(radius=F(3 * slant_spacing(slope)), max_px=16)
        ref = cloud_render_oriented_ref(cloud, None, Kc, Rc, tc, SLANT_W, SLANT_H, **kw)
        for c, nrm in ((cloud, None), (cloud[:, :3], np.ascontiguousarray(cloud[:, 3:6]))):
            rc, _, got = stub_render(lib, c, nrm, Kc, Rc, tc, SLANT_W, SLANT_H, **kw)
            assert rc == 0 and (got["n_splats"], got["n_covered"]) == (ref["n_splats"], ref["n_covered"])
            same_planes(got, ref)
    sc, _, spacing = scene()
    thin = thinned_cloud()
    nrm = np.concatenate([mixed_normals(len(thin), 2), np.full((len(thin), 2), np.nan, F)], axis=1)             # a stride of 5
    kw = dict(radius=F(3 * spacing), max_px=3, min_points=2, depth_diff=F(0.002))
    rc, _, got = stub_render(lib, thin, nrm, sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw)
    ref = cloud_render_oriented_ref(thin, nrm, sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw)
    assert rc == 0 and (got["n_splats"], got["n_covered"]) == (ref["n_splats"], ref["n_covered"])
    same_planes(got, ref)
    rc, msg, got = stub_render(lib, np.array([at(4, 3, 2.0), at(0, 0, 2.0)], F), np.zeros((2, 3), F), K, R, T, W, H, radius=0.5, max_splats=33)
    assert rc != 0 and "max_splats" in msg and got["n_splats"] == 34 and got["n_covered"] == -1              # refused, the count still filled
    assert all((got[k] == (77 if k == "count" else -7)).all() for k in PLANES)                                  # and nothing written


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """the scene on disk with maps of views 0 and 1 (the ground truth with noise and holes), and the thinned cloud as a PLY with and without normals"""
    sc, cloud, spacing = scene()
    root = str(tmp_path_factory.mktemp("splat_scene")) + "/"
    tio.export_scene(sc, root)
    rng = np.random.default_rng(3)
    maps = {}
    for v in (0, 1):
        d = sc.meta["gt_all"][v][0].numpy().astype(F)
        d = (d * (1 + rng.normal(scale=2e-3, size=d.shape))).astype(F)
        d[rng.random(d.shape) < 0.05] = 0
        os.makedirs(root + "APD/%08d" % v)
        tio.write_dmb(root + "APD/%08d/TSAR_disp.dmb" % v, d)
        maps[v] = d
    thin = thinned_cloud()
    nrm = mixed_normals(len(thin), 4)
    nrm[::7, 1] = 0                                                          # (a PLY's text would keep a NaN, but keep the file plain)
    tio.write_ply(root + "gt.ply", thin)
    tio.write_ply(root + "gt_normals.ply", thin, normals=nrm)
    return root, maps, nrm


def run(built, *args):
    return subprocess.run([built + "/tsar_evaluate_maps", *args], capture_output=True, text=True, timeout=300)


def oriented_composition(maps, normals, radius, tolerances, **kw):
    """evaluate_depth_maps_ref with the oriented render in the square render's place"""
    sc, _, _ = scene()
    views = []
    for v, d in maps.items():
        r = cloud_render_oriented_ref(thinned_cloud(), normals, sc.K[v], sc.R[v], sc.t[v], d.shape[1], d.shape[0], radius, **kw)
        c = depth_compare_ref(d, r["depth"], tolerances)
        c.update(n_splats=r["n_splats"], n_covered=r["n_covered"])
        views.append(c)
    total = {k: sum(c[k] for c in views) for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered")}
    total["within"] = np.sum([c["within"] for c in views], axis=0).astype(np.int64)
    return views, total


def check_view(rec, ref):
    for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats", "n_covered"):
        assert rec[k] == ref[k], k
    assert rec["within"] == ref["within"].tolist()
    q = ratios(ref)
    assert rec["accuracy"] == q["accuracy"].tolist() and rec["completeness"] == q["completeness"].tolist() and rec["cover"] == q["cover"]


def test_the_tool_renders_with_the_ply_normals(built, exported, tmp_path):
    root, maps, nrm = exported
    _, _, spacing = scene()
    radius = F(3 * spacing)
    out = run(built, root, root + "gt_normals.ply", "--tolerances=0.001,0.01", "--radius=%.9g" % radius, "--views=0,1", "--oriented", "--json=" + str(tmp_path / "r.json"))
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    assert rec["oriented"] is True and "normals" not in rec and "n_gt_normals" not in rec and rec["n_points"] == len(nrm)
    views, total = oriented_composition(maps, nrm, radius, [0.001, 0.01])
    for got, ref in zip(rec["views"], views):
        check_view(got, ref)
    check_view(rec["total"], total)
    assert 0 < total["n_covered"] < total["n_splats"]
    # and the oriented occluder changes what is scored: the case says something
    _, square = evaluate_depth_maps_ref([maps[0], maps[1]], thinned_cloud(), scene()[0].K[[0, 1]], scene()[0].R[[0, 1]], scene()[0].t[[0, 1]], [0.001, 0.01], radius)
    assert total["n_gt"] != square["n_gt"]


def test_the_tool_estimates_the_normals_once_on_the_device(built, exported):
    """the stand-in's tsar_cloud_normals_ctx hands back what it was given: the normal (K, N, R), and none for every third point"""
    root, maps, _ = exported
    _, _, spacing = scene()
    radius = F(3 * spacing)
    out = run(built, root, root + "gt.ply", "--tolerances=0.01", "--radius=%.9g" % radius, "--views=0,1", "--oriented", "--normals=8", "--normal_radius=0.75",
              "--normal_min_neighbors=4")
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    n = len(thinned_cloud())
    nrm = np.tile(np.array([8, 4, 0.75], F), (n, 1))
    nrm[::3] = 0
    assert rec["oriented"] is True and rec["normals"] == {"k": 8, "radius": 0.75, "min_neighbors": 4} and rec["n_gt_normals"] == n - len(nrm[::3])
    views, total = oriented_composition(maps, nrm, radius, [0.01])
    check_view(rec["total"], total)
    # the defaults: K = 16, N = 5; and a PLY with normals is estimated afresh when a radius is given
    out = run(built, root, root + "gt_normals.ply", "--tolerances=0.01", "--radius=%.9g" % radius, "--views=0", "--oriented", "--normal_radius=0.5")
    rec = json.loads(out.stdout.splitlines()[-1])
    assert out.returncode == 0 and rec["normals"] == {"k": 16, "radius": 0.5, "min_neighbors": 5}
    nrm = np.tile(np.array([16, 5, 0.5], F), (n, 1))
    nrm[::3] = 0
    check_view(rec["total"], oriented_composition({0: maps[0]}, nrm, radius, [0.01])[1])


def test_without_the_switch_the_output_is_what_it_was(built, built_old, exported):
    root, maps, _ = exported
    _, _, spacing = scene()
    args = [root, root + "gt_normals.ply", "--tolerances=0.001,0.01", "--radius=%.9g" % F(1.5 * spacing)]
    new, old = run(built, *args), run(built_old, *args)
    assert new.returncode == 0 and old.returncode == 0 and new.stderr == old.stderr == ""
    strip = lambda s: re.sub(r'"ms": [0-9.]+', '"ms": 0', s)                  # (the wall-clock figure aside)
    assert strip(new.stdout) == strip(old.stdout)
    rec = json.loads(new.stdout.splitlines()[-1])
    assert "oriented" not in rec and "n_covered" not in rec["total"] and "n_covered" not in rec["views"][0]


NEEDS = "--normals=, --normal_radius= and --normal_min_neighbors= need --oriented"


@pytest.mark.parametrize("ply,args,message", [
    ("gt.ply", ["--oriented"], "--oriented: {gt} has no nx ny nz: give --normal_radius=R (and --normals=K) to estimate them from its points"),
    ("gt.ply", ["--normals=8", "--normal_radius=0.5"], NEEDS), ("gt.ply", ["--normal_radius=0.5"], NEEDS), ("gt.ply", ["--normal_min_neighbors=4"], NEEDS),
    ("gt.ply", ["--oriented", "--normals=8"], "--normals=K and --normal_min_neighbors=N need --normal_radius=R"),
    ("gt.ply", ["--oriented", "--normal_min_neighbors=4"], "--normals=K and --normal_min_neighbors=N need --normal_radius=R"),
    ("gt.ply", ["--oriented", "--normals=2", "--normal_radius=0.5"], "--normals=K must be an integer in 3..32"),
    ("gt.ply", ["--oriented", "--normals=33", "--normal_radius=0.5"], "--normals=K must be an integer in 3..32"),
    ("gt.ply", ["--oriented", "--normal_radius=0"], "--normal_radius=R must be a finite number > 0"),
    ("gt.ply", ["--oriented", "--normal_radius=nan"], "--normal_radius=R must be a finite number > 0"),
    ("gt.ply", ["--oriented", "--normals=4", "--normal_radius=0.5", "--normal_min_neighbors=5"], "--normal_min_neighbors=N must be an integer in 2..K"),
    ("gt.ply", ["--oriented", "--normal_radius=0.5", "--normal_min_neighbors=1"], "--normal_min_neighbors=N must be an integer in 2..K"),
    ("gt.ply", ["--oriented=1"], "unknown option --oriented=1"),
])
def test_command_line_refusals(built, exported, ply, args, message):
    root, _, _ = exported
    out = run(built, root, root + ply, "--tolerances=0.1", "--radius=0.1", *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message.format(gt=root + ply) + "\n"


def test_a_library_without_the_entry_is_named_in_one_line(built_old, exported):
    root, _, _ = exported
    out = run(built_old, root, root + "gt_normals.ply", "--tolerances=0.1", "--radius=0.1", "--oriented")
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "--oriented: this libtsar_hip.so has no tsar_cloud_render_oriented\n"
    assert "--oriented" in run(built_old, "--help").stdout

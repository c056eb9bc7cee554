"""tsar_cloud_render and tsar_depth_compare without a GPU: the numpy restatement (tests/cloud_render_ref.py) held to answers computed by hand;
the brute-force host stand-in (tests/cli_stub/tsar_stub_render.cpp) held to the restatement through ctypes; what the two-buffer render is for,
on the thinned scene cloud; and host/tsar_evaluate_maps.cpp, linked against the stand-in, on an exported scene: its JSON counts equal the
restatement's, --views, a missing map, --write_gt and every refusal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cloud_render_ref import (cloud_render_ref, depth_compare_ref, evaluate_depth_maps_ref, landings, projection, ratios, scene, thinned_cloud)
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate_maps.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_render.cpp")
F = np.float32

# a camera whose arithmetic is exact by hand: f = 8, principal point (4, 3), identity pose, 9 x 7 pixels.  Pixel (u, v) at depth Z is the
# point ((u - 4) Z / 8, (v - 3) Z / 8, Z): p_0 = 8 X + 4 Z, p_1 = 8 Y + 3 Z, p_2 = Z
W, H = 9, 7
K = np.array([[8, 0, 4], [0, 8, 3], [0, 0, 1]], F)
R = np.eye(3, dtype=F)
T = np.zeros(3, F)


def at(u, v, Z):
    return [(u - 4) * Z / 8, (v - 3) * Z / 8, Z]


def render(pts, **kw):
    return cloud_render_ref(np.array(pts, F).reshape(-1, 3), K, R, T, W, H, **kw)


# ---- the render: known answers ------------------------------------------------------------------------------------------------------------
def test_projection_is_k_times_r_t():
    rng = np.random.default_rng(0)
    Kr, Rr, tr = rng.random((3, 3)).astype(F), rng.random((3, 3)).astype(F), rng.random(3).astype(F)
    P = projection(Kr, Rr, tr)
    want = Kr.astype(np.float64) @ np.concatenate([Rr, tr[:, None]], axis=1).astype(np.float64)
    assert P.dtype == F and np.allclose(P, want, rtol=1e-6)
    assert np.array_equal(projection(K, R, T), np.array([[8, 0, 4, 0], [0, 8, 3, 0], [0, 0, 1, 0]], F))


def test_one_point_lands_on_its_pixel_at_its_depth():
    r = render([[0.5, -0.25, 2.0]])                                         # p = (12, 4, 2): x' = 6, y' = 2
    want = np.zeros((H, W), F)
    want[2, 6] = 2.0
    assert np.array_equal(r["depth"], want) and r["n_splats"] == 1
    assert r["count"][2, 6] == 1 and r["count"].sum() == 1
    assert r["index"][2, 6] == 0 and (np.delete(r["index"].reshape(-1), 2 * W + 6) == -1).all()
    r = render([[0.5 + 0.124, -0.25 - 0.124, 2.0]])                         # x' = 6.496, y' = 1.504: still (6, 2)
    assert r["depth"][2, 6] == 2.0
    r = render([[0.5 + 0.126, -0.25 - 0.126, 2.0]])                         # x' = 6.504 -> 7, y' = 1.496 -> 1
    assert r["depth"][1, 7] == 2.0 and r["depth"][2, 6] == 0


def test_the_front_point_wins_and_the_count_follows_depth_diff():
    for far, count in ((2.5, 2), (float(np.nextafter(F(2.5), F(3))), 1)):   # depth_diff * Zc = 0.25 * 2 = 0.5 exactly: the band's edge is 2.5
        for order in ((0, 1), (1, 0)):
            pts = [at(4, 3, 2.0), at(4, 3, far)]
            r = render([pts[order[0]], pts[order[1]]], depth_diff=0.25)
            assert r["depth"][3, 4] == 2.0 and r["index"][3, 4] == order.index(0) and r["count"][3, 4] == count
    # the band is two-sided by definition, though no landing lies in front of the front-most: a point on the pixel further than the band does not count
    assert render([at(4, 3, 2.0), at(4, 3, 1.5), at(4, 3, 1.0)], depth_diff=0.25)["count"][3, 4] == 1     # Zc = 1: |1.5 - 1| > 0.25


def test_equal_depths_the_smallest_index_wins():
    r = render([at(4, 3, 3.0), at(4, 3, 2.0), at(4, 3, 2.0), at(4, 3, 2.0)])
    assert r["index"][3, 4] == 1 and r["count"][3, 4] == 3 and r["depth"][3, 4] == 2.0


def test_footprint_half_width_around_the_rounding_points():
    """fr = 8 * 0.25 = 2: s = floor(2 / p_2 + 0.5) is 1 at p_2 = 4 and 0 just behind it; 2 up to p_2 = fl(4 / 3) = 1.33333337, where the
    quotient 1.49999996 still rounds to 1.5, and 1 at the next float, 1.33333349, where it rounds to 1.49999988"""
    up = lambda z: float(np.nextafter(F(z), F(np.inf)))
    third = F(4) / F(3)
    zs = [4.0, up(4.0), 8.0, 2.0, float(third), up(third), 0.01, 0.2]
    lands, xi, yi, p2, s = landings(np.array([at(4, 3, z) for z in zs], F), K, R, T, W, H, radius=0.25, max_px=8)
    assert lands.all() and (xi == 4).all() and (yi == 3).all()
    assert s.tolist() == [1, 0, 0, 1, 2, 1, 8, 8]                             # 200.5 and 10.5 clamp at max_px
    assert landings(np.array([at(4, 3, 0.01)], F), K, R, T, W, H, radius=0.25, max_px=16)[4].tolist() == [16]
    assert landings(np.array([at(4, 3, 0.01)], F), K, R, T, W, H, radius=0.25, max_px=1)[4].tolist() == [1]
    assert landings(np.array([at(4, 3, 0.01)], F), K, R, T, W, H, radius=0.0)[4].tolist() == [0]


@pytest.mark.parametrize("u,v,cover", [(0, 0, (0, 2, 0, 2)), (8, 6, (6, 8, 4, 6)), (4, 0, (2, 6, 0, 2)), (4, 6, (2, 6, 4, 6)), (0, 3, (0, 2, 1, 5)), (8, 3, (6, 8, 1, 5)),
                                         (4, 3, (2, 6, 1, 5)), (8, 0, (6, 8, 0, 2))])
def test_footprints_are_clipped_at_the_borders(u, v, cover):
    r = render([at(u, v, 2.0)], radius=0.5)                                  # fr = 4: s = floor(2 + 0.5) = 2
    x0, x1, y0, y1 = cover
    want = np.zeros((H, W), bool)
    want[y0:y1 + 1, x0:x1 + 1] = True
    assert np.array_equal(np.isfinite(r["Zo"]), want) and (r["Zo"][want] == 2.0).all()
    assert r["n_splats"] == (x1 - x0 + 1) * (y1 - y0 + 1) and r["depth"][v, u] == 2.0 and np.count_nonzero(r["depth"]) == 1


def test_points_that_take_no_part():
    pts = [at(4, 3, -2.0), [np.nan, 0, 2], [0, np.inf, 2], [0, 0, -np.inf], [0, 0, np.nan], at(-1, 3, 2.0), at(9, 3, 2.0), at(4, -1, 2.0), at(4, 7, 2.0), [0, 0, 0]]
    for radius in (0.0, 0.5):
        r = render(pts, radius=radius)
        assert r["n_splats"] == 0 and not r["landed"].any() and not np.isfinite(r["Zo"]).any()       # an off-image centre's footprint does not reach in
        assert (r["depth"] == 0).all() and (r["count"] == 0).all() and (r["index"] == -1).all()
    assert render([at(-0.49, 3, 2.0)])["depth"][3, 0] == 2.0 and render([at(8.49, 3, 2.0)])["depth"][3, 8] == 2.0    # just inside


def test_a_background_point_beside_a_foreground_point():
    fg, bg = at(4, 3, 2.0), at(5, 3, 4.0)
    r = render([fg, bg], radius=0.25)                                        # s = 1 for both: the foreground covers (5, 3)
    assert r["depth"][3, 4] == 2.0 and r["depth"][3, 5] == 0 and r["index"][3, 5] == -1 and r["count"][3, 5] == 1 and not r["visible"][3, 5]
    r = render([fg, bg], radius=0.0)
    assert r["depth"][3, 5] == 4.0 and r["index"][3, 5] == 1
    r = render([fg, at(5, 3, 2.03)], radius=0.25)                            # 0.03 <= 0.02 * 2: the same surface
    assert r["depth"][3, 5] == F(2.03) and r["visible"][3, 5]
    r = render([fg, at(5, 3, 2.05)], radius=0.25)
    assert r["depth"][3, 5] == 0
    assert render([fg, at(5, 3, 2.05)], radius=0.25, occlusion_diff=0.03)["depth"][3, 5] == F(2.05)
    assert render([fg, at(6, 3, 4.0)], radius=0.25)["depth"][3, 6] == 4.0     # beyond the footprint


def test_min_points():
    pts = [at(4, 3, 2.0), at(4, 3, 2.001), at(5, 3, 2.0)]
    r = render(pts, min_points=2)
    assert r["depth"][3, 4] == 2.0 and r["depth"][3, 5] == 0 and r["index"][3, 5] == -1 and r["count"][3, 5] == 1 and r["count"][3, 4] == 2
    assert render(pts, min_points=3)["depth"].max() == 0
    many = render([at(4, 3, 2.0)] * 300)
    assert many["count"][3, 4] == 255 and many["support"][3, 4] == 300 and many["index"][3, 4] == 0   # saturated


def test_a_refused_max_splats():
    pts = [at(4, 3, 2.0), at(0, 0, 2.0)]
    assert render(pts, radius=0.5)["n_splats"] == 25 + 9
    r = render(pts, radius=0.5, max_splats=33)
    assert r == {"n_splats": 34, "refused": True}
    assert not render(pts, radius=0.5, max_splats=34)["refused"]


# ---- depth_compare: known answers ----------------------------------------------------------------------------------------------------------
def test_depth_compare_known_answers():
    gt = np.array([2, 2, 2, 2, 2, 0, np.nan, np.inf, -1, 2, 2, 2, 2], F)
    d = np.array([2, 2.25, 1.75, 2.5, 1.0, 2, 2, 2, 2, 0, np.nan, np.inf, -2], F)
    r = depth_compare_ref(d, gt, [0.125, 0.25])                               # tol * G = 0.25 and 0.5, exactly
    assert (r["n_gt"], r["n_both"]) == (9, 5) and r["within"].tolist() == [3, 4] and (r["n_front"], r["n_behind"]) == (1, 1)
    assert np.array_equal(r["error"][:5], np.array([0, 0.125, -0.125, 0.25, -0.5], F)) and np.isnan(r["error"][5:]).all()
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1], np.uint8)
    r = depth_compare_ref(d, gt, [0.125, 0.25], mask)
    assert (r["n_gt"], r["n_both"]) == (6, 3) and r["within"].tolist() == [2, 3] and (r["n_front"], r["n_behind"]) == (0, 1) and np.isnan(r["error"][1])
    q = ratios(r)
    assert q["accuracy"].tolist() == [2 / 3, 1.0] and q["completeness"].tolist() == [2 / 6, 3 / 6] and q["cover"] == 0.5
    empty = depth_compare_ref(np.zeros(4, F), np.zeros(4, F), [0.1])
    assert empty["n_gt"] == 0 and ratios(empty)["cover"] == 0.0 and ratios(empty)["accuracy"].tolist() == [0.0]


# ---- what it is for --------------------------------------------------------------------------------------------------------------------------
def test_the_footprint_closes_the_holes_and_keeps_the_depth():
    sc, _, spacing = scene()
    thin = thinned_cloud()
    gt = sc.gt_depth.numpy()
    figures = {}
    for name, radius in (("one pixel", 0.0), ("footprint", 1.5 * spacing)):
        r = cloud_render_ref(thin, sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, radius=radius, occlusion_diff=0.02)
        have = (r["depth"] > 0) & (gt > 0)
        rel = (r["depth"][have] - gt[have]) / gt[have]
        figures[name] = {"pixels": int(have.sum()), "cover": float(have.sum() / np.count_nonzero(gt > 0)), "within_1e-3": float(np.mean(np.abs(rel) <= 1e-3)),
                         "behind_1e-2": int(np.count_nonzero(rel > 1e-2))}
    print("thinned cloud (%d points, seed in cloud_render_ref.THIN_SEED) rendered into view 0:" % len(thin), json.dumps(figures))
    one, foot = figures["one pixel"], figures["footprint"]
    assert one["behind_1e-2"] >= 20                                          # the background seen through the holes of the foreground
    assert foot["behind_1e-2"] <= one["behind_1e-2"] / 10
    assert foot["cover"] >= 0.9 * one["cover"]
    assert foot["within_1e-3"] >= one["within_1e-3"]


# ---- the stand-in against the restatement, and the tool ---------------------------------------------------------------------------------------
class Params(C.Structure):
    _fields_ = [("radius", C.c_float), ("max_px", C.c_int32), ("occlusion_diff", C.c_float), ("depth_diff", C.c_float), ("min_points", C.c_int32), ("max_splats", C.c_int64)]


class Camera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_stub_render"))
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", STUB],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate_maps", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d


def stub_render(lib, cloud, Kv, Rv, tv, w, h, sentinel=False, **kw):
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
    depth, count, index = np.full((h, w), -7, F), np.full((h, w), 77, np.uint8), np.full((h, w), -7, np.int32)
    n_splats = C.c_int64(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.tsar_cloud_render_ctx(ctx, ptr(c), C.c_int64(len(c)), c.shape[1], C.byref(cam), w, h, C.byref(p), ptr(depth), ptr(count), ptr(index), C.byref(n_splats), 0)
    msg = L.tsar_last_error(ctx).decode()
    L.tsar_destroy(ctx)
    return rc, msg, {"depth": depth, "count": count, "index": index, "n_splats": n_splats.value}


def same_render(got, ref):
    assert got["n_splats"] == ref["n_splats"]
    assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32)) and np.array_equal(got["count"], ref["count"]) and np.array_equal(got["index"], ref["index"])


def test_the_stand_in_equals_the_restatement(built):
    lib = built + "/libtsar_hip.so"
    sc, cloud, spacing = scene()
    padded = np.full((len(cloud), 5), np.nan, F)
    padded[:, :3] = cloud
    for c, kw in ((cloud, {}), (padded, dict(radius=F(1.5 * spacing))), (thinned_cloud(), dict(radius=F(3 * spacing), max_px=3, min_points=2, depth_diff=F(0.002)))):
        rc, _, got = stub_render(lib, c, sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw)
        assert rc == 0
        same_render(got, cloud_render_ref(c[:, :3], sc.K[0], sc.R[0], sc.t[0], sc.w, sc.h, **kw))
    rc, msg, got = stub_render(lib, np.array([at(4, 3, 2.0), at(0, 0, 2.0)], F), K, R, T, W, H, radius=0.5, max_splats=33)
    assert rc != 0 and "max_splats" in msg and got["n_splats"] == 34                                  # refused, the count still filled
    assert (got["depth"] == -7).all() and (got["count"] == 77).all() and (got["index"] == -7).all()   # and nothing written


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """the scene on disk, with maps of three of its four views (view 2 has none): the ground truth with noise, holes and non-finite values"""
    sc, cloud, spacing = scene()
    root = str(tmp_path_factory.mktemp("maps_scene")) + "/"
    tio.export_scene(sc, root)
    rng = np.random.default_rng(3)
    maps = {}
    for v in (0, 1, 3):
        d = sc.meta["gt_all"][v][0].numpy().astype(F)
        d = (d * (1 + rng.normal(scale=2e-3, size=d.shape))).astype(F)
        d[rng.random(d.shape) < 0.05] = 0
        d[0, :5] = [np.nan, np.inf, -1, 0, 1e30]
        os.makedirs(root + "APD/%08d" % v)
        tio.write_dmb(root + "APD/%08d/TSAR_disp.dmb" % v, d)
        maps[v] = d
    tio.write_dmb(root + "APD/%08d/other_disp.dmb" % 1, maps[1][:60, :80])                              # another stem, another size
    os.makedirs(root + "APD/%08d" % 2)
    gt = root + "gt.ply"
    tio.write_ply(gt, thinned_cloud())
    return root, gt, maps


def run(built, *args):
    return subprocess.run([built + "/tsar_evaluate_maps", *args], capture_output=True, text=True, timeout=300)


def check_view(rec, ref):
    for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats"):
        assert rec[k] == ref[k], k
    assert rec["within"] == ref["within"].tolist()
    q = ratios(ref)
    assert rec["accuracy"] == q["accuracy"].tolist() and rec["completeness"] == q["completeness"].tolist() and rec["cover"] == q["cover"]


def test_the_tool_json_equals_the_restatement(built, exported, tmp_path):
    root, gt, maps = exported
    sc, _, spacing = scene()
    radius = F(1.5 * spacing)
    out = run(built, root, gt, "--tolerances=0.001,0.01", "--radius=%.9g" % radius, "--json=" + str(tmp_path / "r.json"))
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "view 00000002: no APD/00000002/TSAR_disp.dmb, skipped" and lines[1].split()[:3] == ["view", "n_gt", "n_both"] and len(lines) == 1 + 1 + 3 + 1 + 1
    rec = json.loads(lines[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    assert [F(t) for t in rec["tolerances"]] == [F(0.001), F(0.01)] and F(rec["radius"]) == radius and rec["maps"] == "TSAR" and rec["skipped"] == [2]
    assert (rec["max_px"], F(rec["occlusion_diff"]), F(rec["depth_diff"]), rec["min_points"], rec["n_points"]) == (8, F(0.02), F(0.01), 1, len(thinned_cloud()))
    ids = [0, 1, 3]
    views, total = evaluate_depth_maps_ref([maps[v] for v in ids], thinned_cloud(), sc.K[ids], sc.R[ids], sc.t[ids], [0.001, 0.01], radius)
    assert [v["id"] for v in rec["views"]] == ids and all((v["w"], v["h"]) == (160, 120) for v in rec["views"])
    for got, ref in zip(rec["views"], views):
        check_view(got, ref)
    check_view(rec["total"], total)
    assert 0 < total["within"][0] < total["within"][1] < total["n_both"] < total["n_gt"] and total["n_front"] > 0 and total["n_behind"] > 0   # the case says something
    assert lines[-2].split()[0] == "total" and int(lines[-2].split()[1]) == total["n_gt"]


def test_views_maps_and_the_render_switches(built, exported):
    root, gt, maps = exported
    sc, _, spacing = scene()
    out = run(built, root, gt, "--tolerances=0.01", "--radius=0", "--views=3,0")
    rec = json.loads(out.stdout.splitlines()[-1])
    assert out.returncode == 0 and [v["id"] for v in rec["views"]] == [3, 0] and rec["skipped"] == []
    views, total = evaluate_depth_maps_ref([maps[3], maps[0]], thinned_cloud(), sc.K[[3, 0]], sc.R[[3, 0]], sc.t[[3, 0]], [0.01], 0.0)
    check_view(rec["total"], total)
    kw = dict(max_px=2, occlusion_diff=F(0.05), depth_diff=F(0.002), min_points=2)
    out = run(built, root, gt, "--tolerances=0.01", "--radius=%.9g" % F(4 * spacing), "--views=1", "--maps=other", "--max_px=2", "--occlusion_diff=0.05", "--depth_diff=0.002",
              "--min_points=2")
    rec = json.loads(out.stdout.splitlines()[-1])
    assert out.returncode == 0 and (rec["views"][0]["w"], rec["views"][0]["h"]) == (80, 60) and rec["maps"] == "other"      # rendered at the map's own size
    views, total = evaluate_depth_maps_ref([maps[1][:60, :80]], thinned_cloud(), sc.K[[1]], sc.R[[1]], sc.t[[1]], [0.01], F(4 * spacing), **kw)
    check_view(rec["views"][0], views[0])
    out = run(built, root, gt, "--tolerances=0.01", "--radius=0", "--views=2")
    assert out.returncode != 0 and out.stdout == "view 00000002: no APD/00000002/TSAR_disp.dmb, skipped\n" and out.stderr.startswith("no view has a map")


def test_write_gt_writes_the_rendered_maps(built, exported):
    root, gt, maps = exported
    sc, _, spacing = scene()
    radius = F(1.5 * spacing)
    out = run(built, root, gt, "--tolerances=0.01", "--radius=%.9g" % radius, "--write_gt=scan")
    assert out.returncode == 0 and json.loads(out.stdout.splitlines()[-1])["write_gt"] == "scan", out.stderr
    for v in (0, 1, 3):
        ref = cloud_render_ref(thinned_cloud(), sc.K[v], sc.R[v], sc.t[v], 160, 120, radius=radius)
        got = tio.read_dmb(root + "APD/%08d/scan_disp.dmb" % v)
        assert got.shape == (120, 160) and np.array_equal(got.view(np.uint32), ref["depth"].view(np.uint32))
    assert not os.path.exists(root + "APD/00000002/scan_disp.dmb")
    # the written maps are maps: scored against the same render they are all within every tolerance
    rec = json.loads(run(built, root, gt, "--tolerances=1e-6", "--radius=%.9g" % radius, "--maps=scan").stdout.splitlines()[-1])
    assert rec["total"]["within"] == [rec["total"]["n_gt"]] and rec["total"]["cover"] == 1.0 and rec["total"]["n_gt"] > 20000


TOL_MSG = "--tolerances=T1[,T2...]: 1 to 16 tolerances, every one a finite number > 0"


@pytest.mark.parametrize("args,message", [
    (["--radius=0"], "--tolerances=T1[,T2...] is required"),
    (["--tolerances=0.01"], "--radius=R is required (world units; 0 renders without a footprint)"),
    (["--tolerances=", "--radius=0"], TOL_MSG), (["--tolerances=0.1,", "--radius=0"], TOL_MSG), (["--tolerances=0.1,x", "--radius=0"], TOL_MSG),
    (["--tolerances=0", "--radius=0"], TOL_MSG), (["--tolerances=-1", "--radius=0"], TOL_MSG), (["--tolerances=nan", "--radius=0"], TOL_MSG),
    (["--tolerances=inf", "--radius=0"], TOL_MSG), (["--tolerances=" + ",".join(["0.1"] * 17), "--radius=0"], TOL_MSG),
    (["--tolerances=0.1", "--radius=-1"], "--radius=R must be a finite number >= 0"), (["--tolerances=0.1", "--radius=inf"], "--radius=R must be a finite number >= 0"),
    (["--tolerances=0.1", "--radius=nan"], "--radius=R must be a finite number >= 0"), (["--tolerances=0.1", "--radius=x"], "--radius=R must be a finite number >= 0"),
    (["--tolerances=0.1", "--radius=0", "--max_px=0"], "--max_px=N must be an integer in 1..16"), (["--tolerances=0.1", "--radius=0", "--max_px=17"], "--max_px=N must be an integer in 1..16"),
    (["--tolerances=0.1", "--radius=0", "--occlusion_diff=-1"], "--occlusion_diff=REL must be a finite number >= 0"),
    (["--tolerances=0.1", "--radius=0", "--depth_diff=nan"], "--depth_diff=REL must be a finite number >= 0"),
    (["--tolerances=0.1", "--radius=0", "--min_points=0"], "--min_points=N must be an integer in 1..255"),
    (["--tolerances=0.1", "--radius=0", "--min_points=256"], "--min_points=N must be an integer in 1..255"),
    (["--tolerances=0.1", "--radius=0", "--views=1,x"], "--views=id[,id...]: every id must be an integer >= 0"),
    (["--tolerances=0.1", "--radius=0", "--views="], "--views=id[,id...]: every id must be an integer >= 0"),
    (["--tolerances=0.1", "--radius=0", "--views=9"], "--views: view 9 is not in pair.txt"),
    (["--tolerances=0.1", "--radius=0", "--maps="], "--maps=STEM must not be empty or contain a path separator"),
    (["--tolerances=0.1", "--radius=0", "--write_gt="], "--write_gt=STEM must not be empty or contain a path separator"),
    (["--tolerances=0.1", "--radius=0", "--write_gt=a/b"], "--write_gt=STEM must not be empty or contain a path separator"),
    (["--tolerances=0.1", "--radius=0", "--write_gt=TSAR"], "--write_gt=TSAR would overwrite the matcher's own maps"),
    (["--tolerances=0.1", "--radius=0", "--write_gt=TSAR_geom"], "--write_gt=TSAR_geom would overwrite the matcher's own maps"),
    (["--tolerances=0.1", "--radius=0", "--write_gt=TSAR_filtered"], "--write_gt=TSAR_filtered would overwrite the matcher's own maps"),
    (["--tolerances=0.1", "--radius=0", "--maps=other", "--write_gt=other"], "--write_gt=other would overwrite the maps it is compared with"),
    (["--tolerances=0.1", "--radius=0", "--device=x"], "--device=D must be an integer >= 0"),
    (["--tolerances=0.1", "--radius=0", "--frobnicate"], "unknown option --frobnicate"),
])
def test_command_line_refusals(built, exported, args, message):
    root, gt, _ = exported
    out = run(built, root, gt, *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message + "\n"


def test_missing_inputs_and_the_usage_line(built, exported, tmp_path):
    root, gt, _ = exported
    out = run(built, root, str(tmp_path / "none.ply"), "--tolerances=0.1", "--radius=0")
    assert out.returncode != 0 and out.stderr == "cannot open " + str(tmp_path / "none.ply") + "\n"
    out = run(built, str(tmp_path) + "/", gt, "--tolerances=0.1", "--radius=0")
    assert out.returncode != 0 and out.stderr == "cannot read " + str(tmp_path) + "/pair.txt\n"
    out = run(built, root)
    assert out.returncode != 0 and out.stderr.startswith("usage: tsar_evaluate_maps D/ GT.ply --tolerances=")
    assert "not ETH3D's or DTU's program" in out.stderr
    out = run(built, "--help")
    assert out.returncode == 0 and "not ETH3D's or DTU's program" in out.stdout

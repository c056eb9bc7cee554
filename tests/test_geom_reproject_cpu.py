"""The cross-view depth render (include/tsar.h tsar_geom_reproject, geom_reproject_kernels.hip) restated in numpy float32, operation for
operation, and that restatement held to a known answer, to the float64 closed form of the same render and to ground truth; inputs that
exercise the z-test and the support edge; tsar_gipuma's refusals around --geom_cross_view; the binding; the register budget of the new
kernels.  No GPU: tests/test_gpu_geom_reproject.py holds the kernels to reproject_ref bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_geom_check_cpu import CLI, ROOT, _run, gt_case
from test_geom_cpu import matrices64, relative_pose
from tsar_mvs_amd import api

F32 = np.float32
EMPTY = np.uint32(0xFFFFFFFF)


def landings(Bv, depth_v):
    """(lands, at, p_2) of every pixel of view v's map: steps 1-6 of include/tsar.h, each numpy float32 operation one IEEE operation"""
    Bv = np.asarray(Bv, F32)
    Dv = np.asarray(depth_v, F32)
    h, w = Dv.shape
    r, c = np.mgrid[0:h, 0:w]
    C, R = c.astype(F32), r.astype(F32)
    with np.errstate(all="ignore"):
        candidate = (Dv > 0) & (Dv < np.inf)
        cd, rd = C * Dv, R * Dv
        p0, p1, p2 = (((Bv[k, 0] * cd + Bv[k, 1] * rd) + Bv[k, 2] * Dv) + Bv[k, 3] for k in range(3))
        xq, yq = p0 / p2, p1 / p2
        xi, yi = np.floor(xq + F32(0.5)), np.floor(yq + F32(0.5))
        lands = candidate & (p2 > 0) & (p2 < np.inf) & (xi >= 0) & (xi <= F32(w - 1)) & (yi >= 0) & (yi <= F32(h - 1))
    at = np.where(lands, yi, 0).astype(np.int64) * w + np.where(lands, xi, 0).astype(np.int64)
    return lands.ravel(), at.ravel(), np.ascontiguousarray(p2.astype(F32)).ravel()


def reproject_ref(B, maps, depth_diff, min_views, shape=None, want_landings=False):
    """tsar_geom_reproject in numpy float32.  B[v]: view v's float32 3 x 4 back-projection (Matcher.get_geom_matrices; entry 0 unused);
    maps[v]: view v's depth map [h, w] or None (entry 0 ignored); shape = (h, w) where no map says it.  Returns (depth float32, count
    uint8), and with want_landings the number of landings per reference pixel as well."""
    if shape is None:
        shape = next(np.asarray(m).shape for m in maps[1:] if m is not None)
    h, w = shape
    z = np.full(h * w, EMPTY, np.uint32)
    mask = np.zeros(h * w, np.uint64)
    hits = np.zeros(h * w, np.int64)
    land = {v: landings(B[v], maps[v]) for v in range(1, len(maps)) if maps[v] is not None}
    for v, (lands, at, p2) in land.items():                     # pass 1: positive finite floats order like their bits
        np.minimum.at(z, at[lands], p2.view(np.uint32)[lands])
        np.add.at(hits, at[lands], 1)
    for v, (lands, at, p2) in land.items():                     # pass 2
        with np.errstate(all="ignore"):
            Z = z[at].view(F32)
            supports = lands & (np.abs(p2 - Z) <= F32(depth_diff) * Z)
        np.bitwise_or.at(mask, at[supports], np.uint64(1) << np.uint64(v))
    landed = z != EMPTY
    count = np.zeros(h * w, np.int64)
    for v in land:
        count += ((mask >> np.uint64(v)) & np.uint64(1)).astype(np.int64)
    count = np.where(landed, count, 0)
    depth = np.where(landed & (count >= int(min_views)), z.view(F32), F32(0)).astype(F32)
    out = (depth.reshape(h, w), count.astype(np.uint8).reshape(h, w))
    return out + (hits.reshape(h, w),) if want_landings else out


def closed_form_render64(K, R, t, maps, depth_diff):
    """the same render in float64 from the float64 geometry: every source pixel with a depth, back-projected, moved into the reference
    camera and projected; the front-most depth per reference pixel and the number of views with a landing within depth_diff of it"""
    h, w = next(np.asarray(m).shape for m in maps[1:] if m is not None)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    z = np.full(h * w, np.inf)
    per_view = {}
    for v in range(1, len(maps)):
        if maps[v] is None:
            continue
        K0, Kv, Rr, tr = relative_pose(K, R, t, v)
        Dv = np.asarray(maps[v], np.float64)
        Q = Dv[..., None] * (np.stack([c, r, np.ones_like(c)], -1) @ np.linalg.inv(Kv).T)
        P = ((Q - tr) @ Rr) @ K0.T
        with np.errstate(all="ignore"):
            xi = np.floor(P[..., 0] / P[..., 2] + 0.5)
            yi = np.floor(P[..., 1] / P[..., 2] + 0.5)
            lands = (Dv > 0) & np.isfinite(Dv) & (P[..., 2] > 0) & np.isfinite(P[..., 2]) & (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        at = (np.where(lands, yi, 0).astype(np.int64) * w + np.where(lands, xi, 0).astype(np.int64)).ravel()
        lands, p2 = lands.ravel(), P[..., 2].ravel()
        np.minimum.at(z, at[lands], p2[lands])
        per_view[v] = (lands, at, p2)
    count = np.zeros(h * w, np.int64)
    for v, (lands, at, p2) in per_view.items():
        with np.errstate(all="ignore"):
            sup = lands & (np.abs(p2 - z[at]) <= depth_diff * z[at])
        got = np.zeros(h * w, bool)
        got[at[sup]] = True
        count += got
    return np.where(np.isfinite(z), z, 0.0).reshape(h, w), count.reshape(h, w)


SHAPES = [(64, 48, 3), (101, 67, 4)]


def layered(maps):
    """every source map multiplied by 1.0 / 1.2 on a pixel checkerboard: two surfaces behind one another in every view, the true one in
    front"""
    out = [maps[0]]
    for m in maps[1:]:
        h, w = m.shape
        ys, xs = np.mgrid[0:h, 0:w]
        out.append(np.where((xs + ys) % 2 == 0, m, m * F32(1.2)).astype(F32))
    return out


def support_edge(maps):
    """view v's map scaled to either side of the depth_diff = 0.01 edge"""
    scales = [F32(1.009), F32(0.991), F32(1.011), F32(0.989)]
    return [maps[0]] + [(m * scales[v % 4]).astype(F32) for v, m in enumerate(maps) if v >= 1]


def test_known_answer_on_a_fronto_parallel_plane():
    """test_the_depth_test_cuts_at_depth_diff's scene: a plane at depth Z, the source camera moved 3 px of disparity along x.  Source
    pixel (c, r) lands on (c + 3, r) at depth exactly Z: columns 3..79 hold Z with count 1, columns 0..2 nothing"""
    w, h, f, Z = 80, 60, 100.0, 5.0
    K = np.array([[f, 0, 40.0], [0, f, 30.0], [0, 0, 1]])
    Ks, R, t = np.stack([K, K]), np.stack([np.eye(3), np.eye(3)]), np.array([[0.0, 0, 0], [-3.0 * Z / f, 0, 0]])
    B = [matrices64(Ks, R, t, v)[1].astype(F32) for v in range(2)]
    depth, count = reproject_ref(B, [None, np.full((h, w), Z, F32)], 0.01, 1)
    assert np.all(depth[:, 3:] == F32(Z)) and np.all(count[:, 3:] == 1)
    assert np.all(depth[:, :3] == 0) and np.all(count[:, :3] == 0)
    assert not reproject_ref(B, [None, np.full((h, w), Z, F32)], 0.01, 2)[0].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_the_float64_closed_form_and_renders_ground_truth(shape):
    sc, F, B, maps = gt_case(*shape)
    gt = maps[0]
    depth1, count = reproject_ref(B, maps, 0.01, 1)
    z64, c64 = closed_form_render64(sc.K, sc.R, sc.t, maps, 0.01)
    # the two differ only where float32 rounding moves a landing across a pixel boundary or a depth across the support edge
    with np.errstate(all="ignore"):
        same = (count == c64) & ((depth1 == 0) == (z64 == 0)) & (np.abs(depth1 - z64) <= 1e-5 * z64 + (z64 == 0))
    print("%dx%d: float32 render equals the float64 closed form on %.4f of the pixels" % (shape[0], shape[1], same.mean()))
    assert same.mean() >= 0.995, float(same.mean())
    depth2, _ = reproject_ref(B, maps, 0.01, 2)
    covered = depth2 > 0
    close = np.abs(depth2 - gt)[covered] < F32(1e-2) * gt[covered]
    print("%dx%d: coverage at min_views = 2: %.4f; rendered depths within 1e-2 of ground truth: %.4f" % (shape[0], shape[1], covered.mean(), close.mean()))
    assert covered.mean() >= 0.95                               # measured 0.967 / 0.982
    assert close.mean() >= 0.99                                 # measured 0.995 / 0.996
    assert np.array_equal(covered, count >= 2) and np.array_equal(depth2[covered], depth1[covered])


@pytest.mark.parametrize("shape", SHAPES)
def test_inputs_exercise_the_z_test_and_the_support_edge(shape):
    sc, F, B, maps = gt_case(*shape)
    gt = maps[0]
    depth, count, hits = reproject_ref(B, layered(maps), 0.01, 1, want_landings=True)
    several = float((hits >= 2).mean())
    covered = depth > 0
    front = float((np.abs(depth - gt)[covered] < F32(1e-2) * gt[covered]).mean())
    print("%dx%d, layered: %.4f of the pixels receive two or more landings; %.4f of the covered ones are within 1e-2 of ground truth" % (shape[0], shape[1], several, front))
    assert several >= 0.90                                      # measured 0.943 / 0.953
    # the front layer wins wherever one of its pixels lands; the layer behind shows through where none does
    assert front >= 0.75                                        # measured 0.795 / 0.883
    _, count_edge = reproject_ref(B, support_edge(maps), 0.01, 1)
    assert len(np.unique(count_edge)) >= 3, np.unique(count_edge)


def test_non_candidates_missing_maps_and_min_views():
    sc, F, B, maps = gt_case(64, 48, 3)
    h, w = maps[0].shape
    n = len(maps)
    for bad in (0.0, -0.0, -1.5, np.nan, np.inf, -np.inf):
        assert not landings(B[1], np.full((h, w), bad, F32))[0].any(), bad
        depth, count = reproject_ref(B, [None] + [np.full((h, w), bad, F32)] * (n - 1), 0.01, 1)
        assert not depth.any() and not count.any()
    # sprinkled into a map they take their own landings away and nothing else
    rng = np.random.default_rng(3)
    pick = rng.integers(0, 12, (h, w))
    holes = maps[1].copy()
    for k, val in enumerate([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf]):
        holes[pick == k] = val
    lands, at, p2 = landings(B[1], holes)
    full = landings(B[1], maps[1])
    keep = (pick >= 6).ravel()
    assert not lands[~keep].any() and np.array_equal(lands[keep], full[0][keep]) and np.array_equal(at[lands], full[1][lands])
    # a view without a map, and no maps at all
    one_less = reproject_ref(B, [None, maps[1], None, maps[3]], 0.01, 1)
    assert one_less[1].max() == 2 and one_less[0].any()
    nothing = reproject_ref(B, [None] * n, 0.01, 1, shape=(h, w))
    assert not nothing[0].any() and not nothing[1].any() and nothing[0].shape == (h, w)
    # min_views = n is more than the n - 1 sources can give
    depth_n, count_n = reproject_ref(B, maps, 0.01, n)
    assert not depth_n.any() and count_n.max() == n - 1
    for k in range(1, n):
        dk, ck = reproject_ref(B, maps, 0.01, k)
        assert np.array_equal(ck, count_n) and np.array_equal(dk > 0, count_n >= k)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,message", [
    (["--geom_cross_view"], "work with --geom_consistency only"),
    (["--geom_cross_view=2"], "work with --geom_consistency only"),
    (["--geom_cross_view_depth_diff=0.02"], "work with --geom_consistency only"),
    (["--geom_consistency", "--geom_cross_view=0"], "--geom_cross_view=K must be an integer in 1..63"),
    (["--geom_consistency", "--geom_cross_view=64"], "--geom_cross_view=K must be an integer in 1..63"),
    (["--geom_consistency", "--geom_cross_view=1.5"], "--geom_cross_view=K must be an integer in 1..63"),
    (["--geom_consistency", "--geom_cross_view=x"], "--geom_cross_view=K must be an integer in 1..63"),
    (["--geom_consistency", "--geom_cross_view="], "--geom_cross_view=K must be an integer in 1..63"),
    (["--geom_consistency", "--geom_cross_view_depth_diff=0.02"], "--geom_cross_view_depth_diff needs --geom_cross_view"),
    (["--geom_consistency", "--geom_cross_view", "--geom_cross_view_depth_diff=0"], "--geom_cross_view_depth_diff must be finite and > 0"),
    (["--geom_consistency", "--geom_cross_view", "--geom_cross_view_depth_diff=-0.01"], "--geom_cross_view_depth_diff must be finite and > 0"),
    (["--geom_consistency", "--geom_cross_view", "--geom_cross_view_depth_diff=inf"], "--geom_cross_view_depth_diff must be finite and > 0"),
    (["--geom_consistency", "--geom_cross_view", "--geom_cross_view_depth_diff=nan"], "--geom_cross_view_depth_diff must be finite and > 0"),
])
def test_refusals(tmp_path, args, message):
    out = _run(tmp_path, *args)
    assert out.returncode != 0
    assert message in out.stdout + out.stderr


def test_usage_names_the_switches():
    out = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--geom_cross_view[=K]" in out.stdout and "--geom_cross_view_depth_diff=REL" in out.stdout


def test_api_binds_the_two_entries():
    import ctypes as C
    assert "tsar_geom_reproject" in api.ABI_SYMBOLS and "tsar_pm_merge_depths" in api.ABI_SYMBOLS and "tsar_default_geom_reproject_params" in api.ABI_SYMBOLS
    assert C.sizeof(api.GeomReprojectParams) == 8
    assert [f[0] for f in api.GeomReprojectParams._fields_] == ["depth_diff", "min_views"]
    L = api.load_library()
    assert len(L.tsar_geom_reproject.argtypes) == 5 and len(L.tsar_pm_merge_depths.argtypes) == 4
    p = api.GeomReprojectParams()
    L.tsar_default_geom_reproject_params(C.byref(p))           # host code: runs without a device
    assert F32(p.depth_diff) == F32(0.01) and p.min_views == 1
    assert callable(api.Matcher.geom_reproject) and callable(api.Matcher.merge_depths)
    import inspect
    for fn in (api.run_geom_pass, api.run_geom_pass_multiscale):
        sig = inspect.signature(fn).parameters
        assert sig["cross_view"].default == 0 and sig["cross_view_depth_diff"].default == 0.01


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_new_kernels_keep_the_register_budget(tmp_path):
    """one lane per pixel, nothing kept between the passes: no scratch, no LDS, far inside the 128 VGPRs of four waves per SIMD"""
    out = tmp_path / "geom_reproject_kernels.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "geom_reproject_kernels.hip"), str(out)], check=True,
                   capture_output=True, timeout=600)
    txt = out.read_text()
    seen = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        seen.append(name)
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs"
    # the two scatter passes, the resolve, and the two kernels of tsar_pm_merge_depths
    assert len(seen) == 5 and sum("geom_reproject_scatter_kernel" in s for s in seen) == 2, seen
    assert any("geom_reproject_resolve_kernel" in s for s in seen) and any("merge_candidate_kernel" in s for s in seen) and any("merge_select_kernel" in s for s in seen)

"""The geometric-consistency check (include/tsar.h tsar_geom_check, geom_check_kernels.hip) restated in numpy float32, operation for
operation, and that restatement held to the float64 closed form of the same reprojection and to ground truth; tsar_gipuma's refusals
around --consistency_filter; the mask PNG it writes, through --check-mask=; the register budget of the kernel.  No GPU:
tests/test_gpu_geom_check.py holds the kernel to geom_check_ref bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_geom_cpu import geom_term, matrices64, relative_pose
from tsar_mvs_amd import io as tio
from tsar_mvs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")
F32 = np.float32


def check_chain(F, B, depth_v, x, y, D):
    """(inside, D_v, p_2, e2) of the chain of tsar_set_geom_depths (include/tsar.h) for depths D at reference pixels (x, y) against view
    v's map: test_geom_cpu.geom_term's sequence up to e2, each numpy float32 operation one IEEE operation"""
    F = np.asarray(F, F32)
    B = np.asarray(B, F32)
    h, w = depth_v.shape
    D = np.asarray(D, F32)
    X = np.asarray(x).astype(F32)
    Y = np.asarray(y).astype(F32)
    with np.errstate(all="ignore"):
        xd, yd = X * D, Y * D
        a, b, s = (((F[r, 0] * xd + F[r, 1] * yd) + F[r, 2] * D) + F[r, 3] for r in range(3))
        u, v = a / s, b / s
        c, r = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        inside = (s > 0) & (c >= 0) & (c <= F32(w - 1)) & (r >= 0) & (r <= F32(h - 1))
        ci = np.where(inside, c, 0).astype(np.int64)
        ri = np.where(inside, r, 0).astype(np.int64)
        Dv = np.where(inside, depth_v[ri, ci], F32(0)).astype(F32)
        cd, rd = c * Dv, r * Dv
        p0, p1, p2 = (((B[k, 0] * cd + B[k, 1] * rd) + B[k, 2] * Dv) + B[k, 3] for k in range(3))
        xq, yq = p0 / p2, p1 / p2
        dx, dy = xq - X, yq - Y
        e2 = (dx * dx + dy * dy).astype(F32)
    return inside, Dv, p2.astype(F32), e2


def geom_check_ref(F, B, maps, depth, params):
    """tsar_geom_check in numpy float32.  F[v], B[v]: view v's float32 3 x 4 matrices (Matcher.get_geom_matrices; entry 0 unused);
    maps[v]: view v's depth map [h, w] or None; depth [h, w]: the reference view's map; params: (reproj_error, depth_diff,
    min_consistent).  Returns (count uint8, filtered depth float32, mask float32)."""
    reproj_error, depth_diff, min_consistent = params
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    y, x = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        candidate = (depth > 0) & (depth < np.inf)
        r2 = F32(reproj_error) * F32(reproj_error)
        dd = F32(depth_diff) * depth
        count = np.zeros((h, w), np.int32)
        for v in range(1, len(maps)):
            if maps[v] is None:
                continue
            inside, Dv, p2, e2 = check_chain(F[v], B[v], np.asarray(maps[v], F32), x, y, depth)
            count += inside & (Dv > 0) & (p2 > 0) & (e2 < r2) & (np.abs(p2 - depth) < dd)
    count = np.where(candidate, count, 0)
    keep = count >= int(min_consistent)
    return count.astype(np.uint8), np.where(keep, depth, F32(0)).astype(F32), keep.astype(F32)


def closed_form_count64(K, R, t, maps, depth, reproj_error, depth_diff):
    """the count in float64: the point D K_ref^-1 (x, y, 1) into view v, its nearest pixel, that pixel back with view v's depth into
    the reference camera; the distance to (x, y) below reproj_error and the depth there within depth_diff of D"""
    depth = np.asarray(depth, np.float64)
    h, w = depth.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    count = np.zeros((h, w), np.int32)
    for v in range(1, len(maps)):
        K0, Kv, Rr, tr = relative_pose(K, R, t, v)
        dv = np.asarray(maps[v], np.float64)
        P = depth[..., None] * (np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(K0).T)
        q = (P @ Rr.T + tr) @ Kv.T
        with np.errstate(all="ignore"):
            c = np.floor(q[..., 0] / q[..., 2] + 0.5)
            r = np.floor(q[..., 1] / q[..., 2] + 0.5)
            inside = (q[..., 2] > 0) & (c >= 0) & (c <= w - 1) & (r >= 0) & (r <= h - 1)
            Dv = np.where(inside, dv[np.where(inside, r, 0).astype(int), np.where(inside, c, 0).astype(int)], 0.0)
            Q = Dv[..., None] * (np.stack([c, r, np.ones_like(c)], -1) @ np.linalg.inv(Kv).T)
            Pb = ((Q - tr) @ Rr) @ K0.T
            e = np.hypot(Pb[..., 0] / Pb[..., 2] - x, Pb[..., 1] / Pb[..., 2] - y)
            count += inside & (Dv > 0) & (Pb[..., 2] > 0) & (e < reproj_error) & (np.abs(Pb[..., 2] - depth) < depth_diff * depth)
    return np.where((depth > 0) & np.isfinite(depth), count, 0)


def scene_matrices(sc):
    """F[v], B[v] from the float64 geometry, each entry rounded once to float32"""
    n = len(sc.images)
    FB = [tuple(m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, v)) for v in range(n)]
    return [fb[0] for fb in FB], [fb[1] for fb in FB]


def gt_maps(sc):
    return [g[0].numpy().astype(F32) for g in sc.meta["gt_all"]]


_SCENES = {}


def gt_case(w, h, n_src):
    key = (w, h, n_src)
    if key not in _SCENES:
        sc = synth.make_scene(w, h, n_src, seed=94, all_gt=True)
        F, B = scene_matrices(sc)
        _SCENES[key] = (sc, F, B, gt_maps(sc))
    return _SCENES[key]


DEFAULTS = (2.0, 0.01, 2)


def test_the_chain_is_the_terms_chain():
    """geom_check_ref's chain against test_geom_cpu.geom_term, which tests/test_gpu_geom.py holds the kernels to: the term rebuilt from
    (inside, D_v, p_2, e2) as include/tsar.h writes it equals geom_term bit for bit, on ground truth and on depths that break the chain"""
    sc, F, B, maps = gt_case(64, 48, 3)
    h, w = maps[0].shape
    y, x = np.mgrid[0:h, 0:w]
    tau = F32(3.0)
    for D in (maps[0], maps[0] * F32(1.2), -maps[0], np.full_like(maps[0], np.nan), np.zeros_like(maps[0])):
        for v in (1, 2, 3):
            inside, Dv, p2, e2 = check_chain(F[v], B[v], maps[v], x, y, D)
            with np.errstate(all="ignore"):
                root = np.sqrt(np.clip(np.nan_to_num(e2, nan=F32(2.0 ** -100)), F32(2.0 ** -100), F32(2.0 ** 100))).astype(F32)
                e = np.where(e2 < F32(2.0 ** -100), F32(0), root).astype(F32)
                ok = inside & (Dv > 0) & (p2 > 0) & (e2 < tau * tau)
                e = np.where(ok, np.minimum(e, tau), tau).astype(F32)
            want = geom_term(F[v], B[v], maps[v], x, y, D, 1.0, 3.0)
            assert np.array_equal(e.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", [(64, 48, 3), (101, 67, 4)])
def test_restatement_equals_the_float64_closed_form_on_ground_truth(shape):
    sc, F, B, maps = gt_case(*shape)
    count, _, _ = geom_check_ref(F, B, maps, maps[0], DEFAULTS)
    c64 = closed_form_count64(sc.K, sc.R, sc.t, maps, maps[0], 2.0, 0.01)
    # the two differ only where float32 rounding moves a comparison across its threshold (a projection within ~1e-4 px of a pixel
    # boundary at a depth edge, e2 at r2, the depth difference at dd): a fraction of a percent of the pixels at most
    assert (count == c64).mean() >= 0.995, float((count == c64).mean())
    # a depth off by 5 % is refused by both
    cnt5, _, _ = geom_check_ref(F, B, maps, maps[0] * F32(1.05), DEFAULTS)
    c645 = closed_form_count64(sc.K, sc.R, sc.t, maps, maps[0] * F32(1.05), 2.0, 0.01)
    assert (cnt5 == c645).mean() >= 0.995


def test_ground_truth_is_consistent_and_a_wrong_depth_is_not():
    sc, F, B, maps = gt_case(64, 48, 3)
    count, filtered, mask = geom_check_ref(F, B, maps, maps[0], DEFAULTS)
    share = float((count >= 2).mean())
    print("64x48, 3 sources: count >= 2 on %.4f of the pixels" % share)
    assert share >= 0.95                                        # measured 97.5 %
    assert np.array_equal(mask == 1, count >= 2) and np.array_equal(filtered, np.where(count >= 2, maps[0], 0))
    cnt5, _, _ = geom_check_ref(F, B, maps, maps[0] * F32(1.05), DEFAULTS)
    wrong = float((cnt5 >= 1).mean())
    print("the reference depth times 1.05: count >= 1 on %d of %d pixels" % (int((cnt5 >= 1).sum()), cnt5.size))
    assert wrong < 0.01                                         # measured 1 pixel of 3072


def test_ground_truth_is_consistent_on_an_odd_shape():
    sc, F, B, maps = gt_case(101, 67, 4)
    count, _, _ = geom_check_ref(F, B, maps, maps[0], DEFAULTS)
    share = float((count >= 2).mean())
    print("101x67, 4 sources: count >= 2 on %.4f of the pixels" % share)
    assert share >= 0.95                                        # measured 99.7 %


def test_non_candidates_maps_without_estimates_and_min_consistent():
    sc, F, B, maps = gt_case(64, 48, 3)
    D = maps[0].copy()
    D[0, :6] = [0.0, -1.0, np.nan, np.inf, -np.inf, -0.0]
    count, filtered, mask = geom_check_ref(F, B, maps, D, DEFAULTS)
    assert np.all(count[0, :6] == 0) and np.all(filtered[0, :6] == 0) and np.all(mask[0, :6] == 0)
    none = [maps[0], None, None, None]
    assert np.all(geom_check_ref(F, B, none, maps[0], DEFAULTS)[0] == 0)
    holes = [maps[0]] + [np.zeros_like(m) for m in maps[1:]]
    assert np.all(geom_check_ref(F, B, holes, maps[0], DEFAULTS)[0] == 0)
    one = [maps[0], maps[1], None, None]
    c1 = geom_check_ref(F, B, one, maps[0], (2.0, 0.01, 1))
    assert c1[0].max() == 1 and np.array_equal(c1[2] == 1, c1[0] >= 1)
    full = geom_check_ref(F, B, maps, maps[0], DEFAULTS)[0]
    for k in (1, 2, 3):
        ck, fk, mk = geom_check_ref(F, B, maps, maps[0], (2.0, 0.01, k))
        assert np.array_equal(ck, full) and np.array_equal(mk == 1, full >= k) and np.array_equal(fk > 0, full >= k)


def test_the_depth_test_cuts_at_depth_diff():
    """a fronto-parallel plane at depth Z seen by a source camera moved along x: whatever source pixel a hypothesis lands on, the point
    there has depth exactly Z in the reference camera (p_2 = D_v = Z), so a hypothesis 0.9 % off Z passes the 1 % test and one 1.1 % off
    fails it, each way, wherever it lands inside the source image; the reprojection bound is held wide open"""
    w, h, f, Z = 80, 60, 100.0, 5.0
    K = np.array([[f, 0, 40.0], [0, f, 30.0], [0, 0, 1]])
    Ks, R, t = np.stack([K, K]), np.stack([np.eye(3), np.eye(3)]), np.array([[0.0, 0, 0], [-3.0 * Z / f, 0, 0]])
    FB = [tuple(m.astype(F32) for m in matrices64(Ks, R, t, v)) for v in range(2)]
    F, B = [fb[0] for fb in FB], [fb[1] for fb in FB]
    maps = [None, np.full((h, w), Z, F32)]
    inner = np.zeros((h, w), bool)
    inner[:, 8:] = True                                         # the disparity is 3 px: these land inside view 1 at any of the depths
    for scale, passes in ((1.009, True), (0.991, True), (1.011, False), (0.989, False), (1.0, True)):
        count = geom_check_ref(F, B, maps, np.full((h, w), Z * scale, F32), (50.0, 0.01, 1))[0]
        assert np.all(count[inner] == (1 if passes else 0)), scale


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _run(tmp_path, *args, all_views=True):
    if not os.path.exists(CLI):
        pytest.fail("tsar_gipuma is not built (__graft_entry__.build())")
    common = ["-mslp_folder", str(tmp_path) + "/", "-images_folder", str(tmp_path) + "/images/"]
    return subprocess.run([CLI, *(["--all"] if all_views else []), *common, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,all_views,message", [
    (["--consistency_filter"], False, "--consistency_filter needs --all"),
    (["--consistency_filter=3"], False, "--consistency_filter needs --all"),
    (["--consistency_filter", "--mode=tsar"], True, "--consistency_filter does not work with --mode=tsar or --mode=load"),
    (["--consistency_filter", "--mode=load"], True, "--consistency_filter does not work with --mode=tsar or --mode=load"),
    (["--consistency_filter=0"], True, "--consistency_filter=K must be an integer in 1..31"),
    (["--consistency_filter=32"], True, "--consistency_filter=K must be an integer in 1..31"),
    (["--consistency_filter=x"], True, "--consistency_filter=K must be an integer in 1..31"),
    (["--consistency_filter="], True, "--consistency_filter=K must be an integer in 1..31"),
    (["--filter_reproj_error=1.5"], True, "work with --consistency_filter only"),
    (["--filter_depth_diff=0.02"], True, "work with --consistency_filter only"),
    (["--consistency_filter", "--filter_reproj_error=0"], True, "--filter_reproj_error in (0, 2^20] pixels"),
    (["--consistency_filter", "--filter_depth_diff=-0.01"], True, "--filter_depth_diff finite and > 0"),
])
def test_refusals(tmp_path, args, all_views, message):
    out = _run(tmp_path, *args, all_views=all_views)
    assert out.returncode != 0
    assert message in out.stdout + out.stderr


def test_usage_names_the_options():
    out = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--consistency_filter[=K]" in out.stdout and "--filter_reproj_error=PX" in out.stdout and "--filter_depth_diff=REL" in out.stdout


def test_mask_png_round_trip(tmp_path):
    """TSAR_consistent.png as the filter phase writes it (--encode-mask= runs that writer on a filtered depth map without a GPU):
    --check-mask=, the decoder of --mode=tsar's weak.png, reads back exactly the mask"""
    rng = np.random.default_rng(5)
    h, w = 37, 53                                               # odd in both directions
    depth = np.where(rng.random((h, w)) < 0.6, rng.uniform(1.0, 9.0, (h, w)), 0.0).astype(F32)
    depth[3, 4] = np.nan                                        # not kept: not > 0
    dmb, png = str(tmp_path / "TSAR_filtered_disp.dmb"), str(tmp_path / "TSAR_consistent.png")
    tio.write_dmb(dmb, depth)
    enc = subprocess.run([CLI, "--encode-mask=" + dmb + ":" + png], capture_output=True, text=True, timeout=60)
    assert enc.returncode == 0, enc.stdout + enc.stderr
    mask = (depth > 0).ravel()
    ones = int(mask.sum())
    checksum = int((np.flatnonzero(mask) % 9973).sum())
    assert f"mask {w} x {h} reliable {ones} " in enc.stdout
    chk = subprocess.run([CLI, "--check-mask=" + png], capture_output=True, text=True, timeout=60)
    assert chk.returncode == 0, chk.stdout + chk.stderr
    assert chk.stdout.strip() == f"mask {w} x {h} reliable {ones} checksum {checksum}"
    # 8-bit gray, 255 where kept and 0 elsewhere
    import struct
    import zlib
    raw = open(png, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    assert struct.unpack(">IIBBBBB", raw[16:29]) == (w, h, 8, 0, 0, 0, 0)
    pos, idat = 8, b""
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        if tag == b"IDAT":
            idat += raw[pos + 8:pos + 8 + n]
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    assert np.all(rows[:, 0] == 0) and np.array_equal(rows[:, 1:], np.where(depth > 0, 255, 0).astype(np.uint8))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_geom_check_kernel_keeps_the_register_budget(tmp_path):
    """one lane per pixel with nothing kept across views: no scratch, and far inside the 128 VGPRs of four waves per SIMD"""
    out = tmp_path / "geom_check_kernels.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "geom_check_kernels.hip"), str(out)], check=True,
                   capture_output=True, timeout=600)
    txt = out.read_text()
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        if "geom_check_kernel" not in name:
            continue
        seen += 1
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs"
    assert seen == 1, seen

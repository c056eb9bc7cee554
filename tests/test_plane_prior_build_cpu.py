"""The plane-prior builder (include/tsar.h tsar_build_plane_prior) restated in numpy, and held to known answers: the kernels
(tsar-mvs_amd/csrc/plane_prior_build_kernels.hip) are held to this restatement bit for bit by test_gpu_plane_prior_build.py.
Integers are int64, the solve is float64 with one numpy operation per operator of the header's statement (numpy fuses nothing; its
quotients and square roots are correctly rounded), rounded once to float32."""
import os
import subprocess

import numpy as np
import pytest

from tsar_mvs_amd import synth

F32, F64, I64, U64 = np.float32, np.float64, np.int64, np.uint64
EMPTY = U64(0xFFFFFFFFFFFFFFFF)
MAX_LEVELS = 16


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def candidates(depth, score=None):
    with np.errstate(invalid="ignore"):
        c = (depth > 0) & (depth < np.inf)
        if score is not None:
            c &= (score >= 0) & (score < np.inf)
    return c


def level_shapes(w, h, cell, max_levels=0):
    out = []
    for l in range(MAX_LEVELS):
        if max_levels and l >= max_levels:
            break
        s = cell << l
        gw, gh = -(-w // s), -(-h // s)
        if gw < 2 or gh < 2:
            break
        out.append((gw, gh))
    return out


def support_grids(depth, score, cell, max_levels=0):
    """per level the [gh][gw] uint64 keys (score bits << 32 | y << 16 | x: the order of (score, raster index)), EMPTY for an empty cell"""
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    ys, xs = np.mgrid[0:h, 0:w]
    sb = np.zeros((h, w), U64)
    if score is not None:
        sb = (np.asarray(score, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(U64)      # (-0.0 counts as +0.0)
    key = (sb << U64(32)) | (ys.astype(U64) << U64(16)) | xs.astype(U64)
    key = np.where(candidates(depth, None if score is None else np.asarray(score, F32)), key, EMPTY)
    grids = []
    for l, (gw, gh) in enumerate(level_shapes(w, h, cell, max_levels)):
        if l == 0:
            pad = np.full((gh * cell, gw * cell), EMPTY, U64)
            pad[:h, :w] = key
            grids.append(pad.reshape(gh, cell, gw, cell).min(axis=(1, 3)))
        else:
            f = grids[-1]
            pad = np.full((gh * 2, gw * 2), EMPTY, U64)
            pad[:f.shape[0], :f.shape[1]] = f
            grids.append(pad.reshape(gh, 2, gw, 2).min(axis=(1, 3)))
    return grids


def orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def inside(ax, ay, bx, by, cx, cy, x, y):
    a2 = orient(ax, ay, bx, by, cx, cy)
    e0, e1, e2 = orient(ax, ay, bx, by, x, y), orient(bx, by, cx, cy, x, y), orient(cx, cy, ax, ay, x, y)
    return ((a2 > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((a2 < 0) & (e0 <= 0) & (e1 <= 0) & (e2 <= 0))


def choose_triangles(grids, w, h, cell):
    """level [h][w] int64 (255 = none) and tri [h][w][6] int64 = (Ax, Ay, Bx, By, Cx, Cy) of the first triangle that contains the pixel;
    diag [h][w]: 0 none, 1 the quad was split along P00-P11, 2 along P10-P01"""
    ys, xs = (a.astype(I64) for a in np.mgrid[0:h, 0:w])
    level = np.full((h, w), 255, I64)
    tri = np.zeros((h, w, 6), I64)
    diag = np.zeros((h, w), I64)
    for l, g in enumerate(grids):
        gh, gw = g.shape
        s = cell << l
        i, j = xs // s, ys // s
        padded = np.full((gh + 2, gw + 2), EMPTY, U64)              # a cell outside the grid reads as empty
        padded[1:-1, 1:-1] = g
        for (a, b) in ((i - 1, j - 1), (i, j - 1), (i - 1, j), (i, j)):
            k = [padded[b + 1 + dj, a + 1 + di] for (di, dj) in ((0, 0), (1, 0), (0, 1), (1, 1))]      # P00, P10, P01, P11
            exists = (k[0] != EMPTY) & (k[1] != EMPTY) & (k[2] != EMPTY) & (k[3] != EMPTY)
            (x00, y00), (x10, y10), (x01, y01), (x11, y11) = [((q & U64(0xFFFF)).astype(I64), ((q >> U64(16)) & U64(0xFFFF)).astype(I64)) for q in k]
            o1, o2 = orient(x00, y00, x11, y11, x10, y10), orient(x00, y00, x11, y11, x01, y01)
            main = ((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))
            t1 = (x00, y00, x10, y10, np.where(main, x11, x01), np.where(main, y11, y01))
            t2 = (np.where(main, x00, x10), np.where(main, y00, y10), x11, y11, x01, y01)
            for t in (t1, t2):
                take = exists & (level == 255) & inside(*t, xs, ys)
                level[take] = l
                diag[take] = np.where(main, 1, 2)[take]
                for c in range(6):
                    tri[..., c][take] = t[c][take]
    return level, tri, diag


def solve_planes(depth, level, tri, K, R):
    """(depth_out, normal_world_out, level_out) from the chosen triangles: the header's float64 chain"""
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    ys, xs = (a.astype(I64) for a in np.mgrid[0:h, 0:w])
    has = level != 255
    ax, ay, bx, by, cx, cy = (tri[..., c] for c in range(6))
    K = np.asarray(K, F32).astype(F64).reshape(3, 3)
    R = np.asarray(R, F32).astype(F64).reshape(3, 3)
    with np.errstate(all="ignore"):
        one = F64(1)
        wA, wB, wC = (np.where(has, one / depth[py, px].astype(F64), one) for (px, py) in ((ax, ay), (bx, by), (cx, cy)))
        area2 = np.where(has, orient(ax, ay, bx, by, cx, cy), 1).astype(F64)
        dB, dC = wB - wA, wC - wA
        gx = (dB * (cy - ay).astype(F64) - dC * (by - ay).astype(F64)) / area2
        gy = (dC * (bx - ax).astype(F64) - dB * (cx - ax).astype(F64)) / area2
        wp = (wA + gx * (xs - ax).astype(F64)) + gy * (ys - ay).astype(F64)
        has = has & (wp > 0)
        c0 = (wA - gx * ax.astype(F64)) - gy * ay.astype(F64)
        m = [(K[0, k] * gx + K[1, k] * gy) + K[2, k] * c0 for k in range(3)]
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        q = [-m[k] / ln for k in range(3)]
        nw = np.stack([((R[0, k] * q[0] + R[1, k] * q[1]) + R[2, k] * q[2]).astype(F32) for k in range(3)], -1)
        d = (one / wp).astype(F32)
    return np.where(has, d, F32(0)), np.where(has[..., None], nw, F32(0)), np.where(has, level, 255).astype(np.uint8)


def build_plane_prior_ref(depth, score, K, R, cell, max_levels=0, details=False):
    """tsar_build_plane_prior on the CPU: depth, score [h][w] float32 (score may be None), K and R the reference camera's float32
    intrinsics and world->camera rotation.  Returns (depth_out, normal_world_out, level_out); details=True adds (tri, diag)."""
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    grids = support_grids(depth, score, cell, max_levels)
    assert grids, "the image is too small for one level"
    level, tri, diag = choose_triangles(grids, w, h, cell)
    out = solve_planes(depth, level, tri, K, R)
    return out + (tri, diag) if details else out


# ---- known answers -----------------------------------------------------------------------------------------------------------------
K0 = np.array([[40, 0, 31.5], [0, 40, 23.5], [0, 0, 1]], F32)
EYE = np.eye(3, dtype=F32)


def _lattice_box(level_shape, cell):
    """the bounding box of the level-0 support lattice when every pixel is a candidate (supports are the cells' first pixels)"""
    gw, gh = level_shape
    return (gw - 1) * cell, (gh - 1) * cell                          # pixels with x <= X and y <= Y are inside a quad


def test_fronto_parallel_map():
    h, w = 48, 64
    depth = np.full((h, w), 2.5, F32)
    d, n, lv = build_plane_prior_ref(depth, None, K0, EYE, 4)
    X, Y = _lattice_box(level_shapes(w, h, 4)[0], 4)
    ins = np.zeros((h, w), bool)
    ins[:Y + 1, :X + 1] = True
    assert (lv[ins] == 0).all() and (d[ins] == F32(2.5)).all()
    assert (n[ins] == np.array([0, 0, -1], F32)).all()
    assert (lv[~ins] == 255).all() and (d[~ins] == 0).all() and (n[~ins] == 0).all()


def test_coverage_with_every_pixel_a_candidate():
    """each pixel inside the level-0 lattice's bounding quads is covered at level 0, on a slanted map and partial cells"""
    h, w = 67, 101
    ys, xs = np.mgrid[0:h, 0:w]
    depth = (1.0 / (0.3 + 0.001 * xs + 0.002 * ys)).astype(F32)
    for cell in (8, 5):
        d, n, lv = build_plane_prior_ref(depth, None, K0, EYE, cell)
        X, Y = _lattice_box(level_shapes(w, h, cell)[0], cell)
        assert (lv[:Y + 1, :X + 1] == 0).all() and (d[:Y + 1, :X + 1] > 0).all()
        assert (lv[Y + 1:] == 255).all() and (lv[:, X + 1:] == 255).all()         # the strip outside the support lattice


def test_ground_truth_planar_region():
    """On the scene's back plane, with every pixel a candidate, the built depth and normal are the ground truth up to the float32
    rounding of the inputs.  With eps = 2^-24 (the relative rounding of a float32), each inverse depth w_k = 1 / D_k is off by at most
    eps * w_k.  Depth: wp is a convex combination of the w_k, so it is off by at most eps * w_max <= eps * wp * (w_max / w_min); the
    output and the ground truth are each rounded once more: |D - gt| <= gt * eps * (w_max / w_min + 2), first order; asserted with
    4 * eps (w_max / w_min < 1.5 over a triangle here, and float64's own rounding is 2^-29 of eps).  Normal: |dgx| <= 2 eps w_max
    (|Cy - Ay| + |By - Ay|) / |area2|, |dgy| likewise with x; m = K^T (gx, gy, c0) with m_2 = wA + gx (cx - Ax) + gy (cy - Ay) for this K, so
    |dm_0| <= fx |dgx|, |dm_1| <= fy |dgy|, |dm_2| <= eps w_max + |cx - Ax| |dgx| + |cy - Ay| |dgy|; the unit normal moves by at most
    |dm| / |m| (first order; asserted with a factor 1.01 for the second), and the output and the ground truth are float32: + 2 eps."""
    sc = synth.make_scene(64, 48, 2, seed=71, all_gt=True)
    gt = sc.gt_depth.numpy().astype(F32)
    prim = sc.gt_prim.numpy()
    K, R = sc.K[0], sc.R[0]
    d, nw, lv, tri, _ = build_plane_prior_ref(gt, None, K, R, 4, details=True)
    ax, ay, bx, by, cx, cy = (tri[..., c] for c in range(6))
    planar = (lv == 0) & (prim == 0) & (prim[ay, ax] == 0) & (prim[by, bx] == 0) & (prim[cy, cx] == 0)
    assert planar.sum() > 500
    eps = 2.0 ** -24
    g64 = gt.astype(F64)
    assert (np.abs(d.astype(F64) - g64)[planar] <= 4 * eps * g64[planar]).all()
    # the normal, in camera coordinates: R n_world
    ncam = nw.astype(F64) @ np.asarray(R, F64).T
    wv = np.stack([1 / g64[ay, ax], 1 / g64[by, bx], 1 / g64[cy, cx]])
    wmax = wv.max(0)
    a2 = np.abs(orient(ax, ay, bx, by, cx, cy)).astype(F64)
    a2[a2 == 0] = 1
    dgx = 2 * eps * wmax * (np.abs(cy - ay) + np.abs(by - ay)) / a2
    dgy = 2 * eps * wmax * (np.abs(bx - ax) + np.abs(cx - ax)) / a2
    fx, fy, pcx, pcy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    dm = np.sqrt((fx * dgx) ** 2 + (fy * dgy) ** 2 + (eps * wmax + np.abs(pcx - ax) * dgx + np.abs(pcy - ay) * dgy) ** 2)
    gtn = sc.gt_normal.numpy().astype(F64)
    # |m| from the ground-truth plane: m is parallel to the normal and m . K^-1 (x, y, 1) = wp
    ys, xs = np.mgrid[0:48, 0:64]
    ray = np.stack([(xs - pcx) / fx, (ys - pcy) / fy, np.ones_like(xs, F64)], -1)
    mlen = (1 / g64) / np.abs((gtn * ray).sum(-1))
    bound = 1.01 * dm / mlen + 2 * eps
    err = np.abs(ncam - gtn).max(-1)
    assert (err[planar] <= bound[planar]).all(), (err[planar] / bound[planar]).max()
    assert bound[planar].max() < 1e-4                                  # (the bound itself is tight enough to mean something)
    # the sign: facing the camera
    assert (ncam[planar][:, 2] < 0).all()


# The hand-made case: 12 x 12 pixels, cell 4, 3 x 3 cells with one candidate each (x, y).  The quad of cells (0..1, 0..1) has P00 = (3, 0),
# P10 = (4, 2), P01 = (0, 4), P11 = (7, 4): orient(P00, P11, P10) = (4)(2) - (4)(1) = 4 and orient(P00, P11, P01) = (4)(4) - (4)(-3) = 28 have
# the same sign (the quad is reflex at P10), so it is split along P10-P01 into (P00, P10, P01), area2 = (1)(4) - (2)(-3) = 10, and
# (P10, P11, P01), area2 = (3)(2) - (2)(-4) = 14.  Pixel (2, 3) is the middle of the shared edge P10-P01; pixel (7, 4) is P11 itself.
SUPPORTS = {(0, 0): (3, 0), (1, 0): (4, 2), (0, 1): (0, 4), (1, 1): (7, 4), (2, 0): (10, 0), (2, 1): (9, 6), (0, 2): (0, 11), (1, 2): (6, 9),
            (2, 2): (8, 8)}


def _hand_maps(supports, n=12):
    depth = np.zeros((n, n), F32)
    for (i, j), (x, y) in supports.items():
        assert i * 4 <= x < i * 4 + 4 and j * 4 <= y < j * 4 + 4
        depth[y, x] = F32(2.0 + 0.05 * x + 0.02 * y)
    return depth


def test_hand_made_case_second_diagonal_shared_edge_and_support_point():
    sup = SUPPORTS
    depth = _hand_maps(sup)
    d, n, lv, tri, diag = build_plane_prior_ref(depth, None, K0, EYE, 4, details=True)
    P00, P10, P01, P11 = sup[(0, 0)], sup[(1, 0)], sup[(0, 1)], sup[(1, 1)]
    o1, o2 = orient(*P00, *P11, *P10), orient(*P00, *P11, *P01)
    assert not (o1 * o2 < 0), "the hand case must force the second diagonal"
    # every covered pixel's triangle contains it (integers) and its vertices are support points
    pts = set(sup.values())
    h, w = depth.shape
    for y in range(h):
        for x in range(w):
            if lv[y, x] == 255:
                continue
            ax, ay, bx, by, cx, cy = (int(v) for v in tri[y, x])
            assert {(ax, ay), (bx, by), (cx, cy)} <= pts
            a2 = orient(ax, ay, bx, by, cx, cy)
            assert a2 != 0
            es = [orient(ax, ay, bx, by, x, y), orient(bx, by, cx, cy, x, y), orient(cx, cy, ax, ay, x, y)]
            assert all(e == 0 or (e > 0) == (a2 > 0) for e in es)
    first = [P00, P10, P01], [P10, P11, P01]
    # a pixel on the shared edge P10-P01 of the quad's two triangles: the first triangle of the documented order takes it
    ex, ey = _lattice_point_on_segment(P10, P01)
    assert lv[ey, ex] == 0 and diag[ey, ex] == 2
    assert [tuple(tri[ey, ex, 2 * k:2 * k + 2]) for k in range(3)] == [tuple(p) for p in first[0]]
    # a support point itself: P11 = the vertex of four quads; the quad with origin (i - 1, j - 1) = (0, 0) comes first, and of its
    # triangles only the second has P11
    x, y = P11
    assert lv[y, x] == 0 and [tuple(tri[y, x, 2 * k:2 * k + 2]) for k in range(3)] == [tuple(p) for p in first[1]]
    # at a support point the built depth is the support's depth up to float64 rounding of the solve, rounded to float32
    assert abs(float(d[y, x]) - float(depth[y, x])) <= 2.0 ** -22 * float(depth[y, x])


def _lattice_point_on_segment(a, b):
    (ax, ay), (bx, by) = a, b
    g = int(np.gcd(abs(bx - ax), abs(by - ay)))
    assert g >= 2, "the shared edge must pass through a pixel centre other than its ends"
    return ax + (bx - ax) // g, ay + (by - ay) // g


def test_empty_cell_sends_its_neighbours_to_level_1():
    h, w = 48, 64
    ys, xs = np.mgrid[0:h, 0:w]
    depth = (1.0 / (0.3 + 0.001 * xs + 0.002 * ys)).astype(F32)
    depth[16:20, 24:28] = 0                                            # level-0 cell (6, 4) of cell 4 is empty
    d, n, lv = build_plane_prior_ref(depth, None, K0, EYE, 4)
    # the four quads that need cell (6, 4) do not exist: the pixels only they cover (between the supports of cells 5..7 x 3..5) go up
    assert (lv[13:20, 21:28] == 1).all()
    assert (lv[:12, :20] == 0).all()
    assert (d[13:20, 21:28] > 0).all()
    # an affine inverse depth is reproduced by any triangle: the level does not show in the depth beyond float32 rounding
    assert np.allclose(d[13:20, 21:28], (1.0 / (0.3 + 0.001 * xs + 0.002 * ys))[13:20, 21:28], rtol=3e-7, atol=0)


def test_no_candidates_at_all():
    depth = np.zeros((48, 64), F32)
    depth[3, 3] = -0.0
    depth[5, 5] = np.nan
    depth[7, 7] = np.inf
    depth[9, 9] = -1.0
    d, n, lv = build_plane_prior_ref(depth, None, K0, EYE, 4)
    assert (d == 0).all() and (n == 0).all() and (lv == 255).all()


def test_max_levels_1_stops_at_level_0():
    h, w = 48, 64
    depth = np.full((h, w), 3.0, F32)
    depth[16:20, 24:28] = 0
    d, n, lv = build_plane_prior_ref(depth, None, K0, EYE, 4, max_levels=1)
    assert set(np.unique(lv)) == {0, 255} and (lv[14:19, 22:27] == 255).all()
    assert len(level_shapes(w, h, 4, 1)) == 1 and len(level_shapes(w, h, 4, 0)) == 4    # 16 x 12, 8 x 6, 4 x 3, 2 x 2 cells


def test_score_picks_the_support_ties_go_to_the_lower_raster_index_and_bad_scores_are_no_candidates():
    h, w = 8, 8
    depth = np.full((h, w), 2.0, F32)
    score = np.full((h, w), 0.5, F32)
    score[2, 1] = 0.25
    score[1, 2] = 0.25                                                 # a tie in cell (0, 0): raster index 1 * 8 + 2 < 2 * 8 + 1
    score[0, 4] = np.nan
    score[0, 5] = -1.0
    score[0, 6] = np.inf
    score[1, 4] = -0.0                                                 # a candidate, counts as +0.0: the best of cell (1, 0)
    score[4:, :4] = np.nan                                             # cell (0, 1): no candidate
    g = support_grids(depth, score, 4)[0]
    xy = lambda k: (int(k) & 0xFFFF, (int(k) >> 16) & 0xFFFF)
    assert xy(g[0, 0]) == (2, 1)
    assert xy(g[0, 1]) == (4, 1) and int(g[0, 1]) >> 32 == 0
    assert g[1, 0] == EMPTY
    assert xy(g[1, 1]) == (4, 4)                                       # all equal: the first pixel
    # without a score: the first pixel of every cell
    g = support_grids(depth, None, 4)[0]
    assert [xy(k) for k in g.ravel()] == [(0, 0), (4, 0), (0, 4), (4, 4)]


def test_coarser_support_is_the_minimum_of_the_children_on_partial_grids():
    rng = np.random.default_rng(5)
    h, w = 67, 101
    depth = np.where(rng.random((h, w)) < 0.3, 2.0, 0.0).astype(F32)
    score = rng.integers(0, 4, (h, w)).astype(F32)                    # many ties
    for cell in (8, 5):
        grids = support_grids(depth, score, cell)
        assert [g.shape[::-1] for g in grids] == level_shapes(w, h, cell)
        ys, xs = np.mgrid[0:h, 0:w]
        key = (score.view(np.uint32).astype(U64) << U64(32)) | (ys.astype(U64) << U64(16)) | xs.astype(U64)
        key[depth == 0] = EMPTY
        for l, g in enumerate(grids):                                  # every level directly from the pixels
            s = cell << l
            for j in range(g.shape[0]):
                for i in range(g.shape[1]):
                    assert g[j, i] == key[j * s:(j + 1) * s, i * s:(i + 1) * s].min()


# ---- the kernels' code objects: no scratch, no LDS -----------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_kernels_use_no_scratch_and_no_lds(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "tsar-mvs_amd", "csrc", "plane_prior_build_kernels.hip")
    out = str(tmp_path / "ppb.s")
    try:
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S",
                        src, "-o", out], check=True, capture_output=True, timeout=600)
    except FileNotFoundError:
        pytest.skip("hipcc not available")
    import re
    txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S*ppb_\w+kernel\S*)\n", txt)
    assert len([n for n in names if not n.endswith(".kd")]) >= 3
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", txt)] == [0] * len(re.findall(r"\.private_segment_fixed_size:", txt))
    assert all(int(v) == 0 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", txt))

"""The CPU oracle's geometric-consistency term (oracle/tsar_oracle.c geom_term, written from include/tsar.h) against the numpy float32
restatement of the same text (test_geom_cpu.geom_term), bit for bit, at the edges of every comparison in the statement; the oracle's
multi-view cost with the term against the numpy best-N combination; orc_pm_rescore against its statement (tsar_pm_rescore).  No GPU:
tests/test_gpu_call_parity.py holds the kernels to this oracle over whole calls."""
import numpy as np
import pytest

import oracle_lib as ol
from test_geom_cpu import expected_cost_planes, geom_term, matrices64
from tsar_mvs_amd import synth

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(96, 72, 3, seed=31, all_gt=True)


def _oracle(sc, **kw):
    return ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, **kw)


def _mats(sc):
    return [None] + [tuple(m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, v)) for v in range(1, len(sc.images))]


def _maps(sc):
    """every source view's ground-truth depth with holes: a block of 0, a block of negative depths (the way back then lands behind the
    reference camera: p2 <= 0) and single +inf / NaN entries (a map is input data: the statement's comparisons must reject them)"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
        maps[v][h // 2:h // 2 + 10, w // 2:w // 2 + 14] *= F32(-1)
        maps[v][5, 7::11] = np.inf
        maps[v][9, 3::13] = np.nan
    return maps


def _check(orc, mats, maps, v, x, y, D, weight, clip):
    got = orc.geom_term(v, x, y, D)
    want = geom_term(mats[v][0], mats[v][1], maps[v], x, y, D, weight, clip)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (int(bad.sum()), got[bad][:5], want[bad][:5])
    return got


def _projection(F, x, y, D):
    """s and floor(u + 0.5) of the statement, in numpy float32 (coverage checks only)"""
    X, Y = np.asarray(x).astype(F32), np.asarray(y).astype(F32)
    D = np.asarray(D, F32)
    with np.errstate(all="ignore"):
        xd, yd = X * D, Y * D
        a, s = (((F[r, 0] * xd + F[r, 1] * yd) + F[r, 2] * D) + F[r, 3] for r in (0, 2))
        return s, np.floor(a / s + F32(0.5))


@pytest.mark.parametrize("v", [1, 2, 3])
@pytest.mark.parametrize("kind", ["gt", "random", "outside", "behind", "nonfinite"])
def test_oracle_term_is_the_restatement(scene, v, kind):
    sc = scene
    h, w = sc.gt_depth.shape
    y, x = np.mgrid[0:h, 0:w]
    gt = sc.gt_depth.numpy().astype(F32)
    rng = np.random.default_rng(v)
    D = {"gt": gt,
         "random": rng.uniform(sc.depth_min * 0.5, sc.depth_max * 2.0, (h, w)).astype(F32),
         "outside": (gt * F32(0.05)).astype(F32),                  # very near: projects far off the source image
         "behind": -gt,                                            # s <= 0
         "nonfinite": np.where((x + y) % 3 == 0, F32(np.inf), np.where((x + y) % 3 == 1, F32(np.nan), F32(-np.inf))).astype(F32)}[kind]
    mats, maps = _mats(sc), _maps(sc)
    orc = _oracle(sc)
    orc.set_geom(maps, mats, weight=0.7, clip=3.0)
    e = _check(orc, mats, maps, v, x, y, D, 0.7, 3.0)
    s, _ = _projection(mats[v][0], x, y, D)
    if kind == "gt":
        assert (e < F32(0.7 * 3.0)).mean() > 0.5 and (e == F32(0.7 * 3.0)).any()       # (both branches taken)
    if kind in ("outside", "behind", "nonfinite"):
        assert np.all(e == F32(0.7) * F32(3.0))
    if kind == "behind":
        assert np.all(s <= 0)


def test_oracle_term_at_the_rounding_of_the_nearest_pixel(scene):
    """D solved in float64 so that u + 0.5 of view 1 lies on an integer, then D and its neighbours up to 3 ulp either side: the sum
    u + 0.5 lands within a few ulp of the integer, on both sides, and c = floor(u + 0.5) changes between neighbours"""
    sc = scene
    h, w = sc.gt_depth.shape
    mats, maps = _mats(sc), _maps(sc)
    F = mats[1][0].astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    gt = sc.gt_depth.numpy().astype(np.float64)
    al = F[0, 0] * xs + F[0, 1] * ys + F[0, 2]
    ga = F[2, 0] * xs + F[2, 1] * ys + F[2, 2]
    u = (al * gt + F[0, 3]) / (ga * gt + F[2, 3])
    target = np.floor(u) + 0.5
    D0 = ((F[2, 3] * target - F[0, 3]) / (al - ga * target)).astype(F32)
    orc = _oracle(sc)
    orc.set_geom(maps, mats, weight=1.0, clip=3.0)
    cs = []
    for k in range(-3, 4):
        D = D0.copy()
        for _ in range(abs(k)):
            D = np.nextafter(D, F32(np.inf) if k > 0 else F32(0))
        _check(orc, mats, maps, 1, xs.astype(int), ys.astype(int), D, 1.0, 3.0)
        cs.append(_projection(mats[1][0], xs.astype(int), ys.astype(int), D)[1])
    flips = (np.stack(cs) != cs[0]).any(0)
    assert flips.mean() > 0.5                                      # (the rounding boundary is crossed at most pixels)


def _synthetic(sc, back_x, dv=1.0, back_z=1.0):
    """F = [I | 0] (pixel (x, y) at depth D lands on source pixel (x, y)); B takes any source pixel to (back_x / dv, 0): at (0, 0) the
    error is exactly |back_x / dv|, so e2 can be placed on either side of a threshold.  back_z < 0: p2 = back_z dv, behind the
    reference camera"""
    F = np.zeros((3, 4), F32)
    F[0, 0] = F[1, 1] = F[2, 2] = 1
    B = np.zeros((3, 4), F32)
    B[0, 3] = back_x
    B[2, 2] = back_z
    h, w = sc.gt_depth.shape
    maps = [None] + [np.full((h, w), F32(dv), F32) for _ in range(1, len(sc.images))]
    return [None] + [(F, B)] * (len(sc.images) - 1), maps


@pytest.mark.parametrize("tau", [3.0, 0.75, 1.3])
def test_oracle_term_at_the_clip(scene, tau):
    """e2 just below and just above tau^2: B places the way back at distance a from (0, 0), for a = tau and its float32 neighbours;
    and on the real geometry, tau set to the error of one pixel and its neighbours"""
    sc = scene
    orc = _oracle(sc)
    tau = F32(tau)
    sides = set()
    for a in (tau * F32(1 - 2.0 ** -20), np.nextafter(tau, F32(0)), tau, np.nextafter(tau, F32(9)), tau * F32(1 + 2.0 ** -20)):
        a = F32(a)
        mats, maps = _synthetic(sc, a)
        orc.set_geom(maps, mats, weight=1.0, clip=float(tau))
        e = _check(orc, mats, maps, 1, 0, 0, F32(2.0), 1.0, float(tau))[()]
        below = bool(F32(a * a) < F32(tau * tau))
        sides.add(below)
        assert e == (min(a, tau) if below else tau)
    assert sides == {True, False}
    # real geometry: the unclipped error of a few pixels as tau
    mats, maps = _mats(sc), _maps(sc)
    h, w = sc.gt_depth.shape
    y, x = np.mgrid[0:h, 0:w]
    gt = sc.gt_depth.numpy().astype(F32)
    e = geom_term(mats[2][0], mats[2][1], maps[2], x, y, gt, 1.0, 1e5)
    for target in (0.1, 0.4, 0.9):
        t0 = F32(e.flat[np.argmin(np.abs(e - F32(target)))])
        for clip in (np.nextafter(t0, F32(0)), t0, np.nextafter(t0, F32(9))):
            orc.set_geom(maps, mats, weight=0.5, clip=float(clip))
            _check(orc, mats, maps, 2, x, y, gt, 0.5, float(clip))


def test_oracle_term_below_two_to_the_minus_100(scene):
    """e2 < 2^-100 gives 0, e2 >= 2^-100 the root: the way back at distance 2^-50 (e2 = 2^-100 exactly), one ulp either side, far
    below and above"""
    sc = scene
    orc = _oracle(sc)
    for a, zero in ((F32(2.0 ** -50), False), (np.nextafter(F32(2.0 ** -50), F32(0)), True), (np.nextafter(F32(2.0 ** -50), F32(1)), False),
                    (F32(2.0 ** -70), True), (F32(2.0 ** -30), False), (F32(0), True)):
        mats, maps = _synthetic(sc, a)
        orc.set_geom(maps, mats, weight=1.0, clip=3.0)
        e = _check(orc, mats, maps, 1, 0, 0, F32(2.0), 1.0, 3.0)[()]
        assert (e == 0) == zero, (a, e)
        if not zero:
            assert e == F32(np.sqrt(np.float64(F32(a * a))))


def test_oracle_term_rejects_a_way_back_behind_the_reference_camera(scene):
    """p2 <= 0 gives tau even where the quotients land exactly on (x, y): x' = 0 / p2 = -0 at (0, 0); so does D_v <= 0"""
    sc = scene
    orc = _oracle(sc)
    for back_z, dv, want in ((-1.0, 1.0, F32(3.0)), (1.0, 1.0, F32(0.0)), (1.0, 0.0, F32(3.0)), (1.0, -1.0, F32(3.0))):
        mats, maps = _synthetic(sc, F32(0), dv=dv, back_z=back_z)
        orc.set_geom(maps, mats, weight=1.0, clip=3.0)
        assert _check(orc, mats, maps, 1, 0, 0, F32(2.0), 1.0, 3.0)[()] == want, (back_z, dv)
    # D_v <= 0 is no estimate even where the way back does not depend on it (p2 = 1, x' = y' = 0)
    for dv, want in ((1.0, F32(0.0)), (0.0, F32(3.0)), (-1.0, F32(3.0)), (-0.0, F32(3.0))):
        mats, maps = _synthetic(sc, F32(0), dv=dv, back_z=0.0)
        mats[1][1][2, 3] = 1
        orc.set_geom(maps, mats, weight=1.0, clip=3.0)
        assert _check(orc, mats, maps, 1, 0, 0, F32(2.0), 1.0, 3.0)[()] == want, dv


def test_a_view_without_a_map_adds_nothing(scene):
    sc = scene
    h, w = sc.gt_depth.shape
    y, x = np.mgrid[0:h, 0:w]
    mats, maps = _mats(sc), _maps(sc)
    maps[2] = None
    orc = _oracle(sc)
    orc.set_geom(maps, mats, weight=0.7, clip=3.0)
    gt = sc.gt_depth.numpy().astype(F32)
    assert np.all(orc.geom_term(2, x, y, gt) == 0)
    assert (orc.geom_term(1, x, y, gt) > 0).any()


def _scene4():
    return synth.make_scene(64, 48, 4, seed=61, all_gt=True)


@pytest.mark.parametrize("n_best,box", [(1, 11), (2, 11), (3, 11), (2, 19), (2, 12)])
@pytest.mark.parametrize("kind", ["gt", "random"])
@pytest.mark.parametrize("weight,clip", [(0.2, 3.0), (1.0, 1.0)])
def test_oracle_cost_planes_with_the_term_is_the_best_n_combination(n_best, box, kind, weight, clip):
    """(weight 1, clip 1: c_v + lambda e_v reaches MAXCOST for many valid views, so validity decided on the sum would differ)"""
    sc = _scene4()
    orc = _oracle(sc, box=box, n_best=n_best, seed=5)
    if kind == "gt":
        planes = np.ascontiguousarray(synth.gt_planes(sc).numpy())
    else:
        orc.pm_init()
        planes = orc.norm4.copy()
    photometric = orc.pm_cost_planes(planes)
    mats, maps = _mats(sc), _maps(sc)
    maps[3] = None                                                 # (one view without a map)
    orc.set_geom(maps, mats, weight=weight, clip=clip)
    cost, bv, rt = orc.pm_cost_planes(planes)
    ec, ebv, ert = expected_cost_planes(orc, mats, maps, planes, n_best, weight, clip)
    assert np.array_equal(_bits(cost), _bits(ec)), int((_bits(cost) != _bits(ec)).sum())
    assert np.array_equal(bv, ebv)
    assert np.array_equal(_bits(rt), _bits(ert))
    assert not np.array_equal(_bits(cost), _bits(photometric[0]))          # (the term is not idle)
    # weight 0 and a cleared term: the photometric result bit for bit
    orc.set_geom(maps, mats, weight=0.0, clip=3.0)
    for _ in range(2):
        c0, b0, r0 = orc.pm_cost_planes(planes)
        assert np.array_equal(_bits(c0), _bits(photometric[0])) and np.array_equal(b0, photometric[1])
        assert np.array_equal(_bits(r0), _bits(photometric[2]))
        orc.clear_geom()


def _loaded(sc, orc):
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[10:22, 20:36] = 0                                        # depth 0: no valid plane there
    depth[30:34, 5:9] = F32(sc.depth_max) * F32(3)                 # finite, beyond depth_max
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    orc.load_planes(depth, normal_world)
    return depth, normal_world


@pytest.mark.parametrize("box", [11, 12])
@pytest.mark.parametrize("geom", [True, False])
def test_oracle_rescore_is_its_statement(box, geom):
    """valid planes stay bit for bit; the others are pm_init's draw at that pixel; cost, best view and ratio are pm_cost_planes of the
    result on the sweeps' window (box 12: init scores on box / 2 = 6, the sweeps on (box - 1) / 2 = 5); the launch counter restarts"""
    sc = _scene4()
    mats, maps = _mats(sc), _maps(sc)
    orc = _oracle(sc, box=box, n_best=2, seed=9)
    depth, normal_world = _loaded(sc, orc)
    before = orc.norm4.copy()
    if geom:
        orc.set_geom(maps, mats, weight=0.2, clip=3.0)
    orc.rescore()
    planes = orc.norm4.copy()
    h, w = depth.shape
    d = np.array([[orc.depth_from_plane(before[y, x], x, y) for x in range(w)] for y in range(h)], F32)
    keep = (d >= F32(sc.depth_min)) & (d <= F32(sc.depth_max))
    assert 0.5 < keep.mean() < 1.0 and not keep[10:22, 20:36].any() and not keep[30:34, 5:9].any()
    assert np.array_equal(_bits(planes[keep]), _bits(before[keep]))
    fresh = _oracle(sc, box=box, n_best=2, seed=9)
    fresh.pm_init()
    assert np.array_equal(_bits(planes[~keep]), _bits(fresh.norm4[~keep]))
    cost, bv, rt = orc.pm_cost_planes(planes)
    assert np.array_equal(_bits(orc.c), _bits(cost)) and np.array_equal(orc.beview, bv) and np.array_equal(_bits(orc.ratio), _bits(rt))
    if box == 12 and not geom:
        # (pm_init's own scores of the same planes are on its window: they differ where the draw was taken)
        assert not np.array_equal(_bits(fresh.c[~keep]), _bits(orc.c[~keep]))
    # the launch counter restarts: a context that swept before gives what a fresh one gives
    used = _oracle(sc, box=box, n_best=2, seed=9)
    used.pm_init()
    used.pm_iterate(1)
    _loaded(sc, used)
    if geom:
        used.set_geom(maps, mats, weight=0.2, clip=3.0)
    used.rescore()
    used.pm_iterate(1)
    orc.pm_iterate(1)
    assert np.array_equal(_bits(used.norm4), _bits(orc.norm4)) and np.array_equal(_bits(used.c), _bits(orc.c))

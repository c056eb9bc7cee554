"""The CPU oracle's plane-prior term (oracle/tsar_oracle.c prior_term / orc_set_plane_prior, written from include/tsar.h) against the
numpy float32 restatement of the same text (test_plane_prior_cpu.add_plane_prior), bit for bit: the oracle's pm_cost_planes with a
prior is its pm_cost_planes without one plus the restated term, with and without the geometric term, in the strict arithmetic and in
both fast ones, in the default build and the -DORC_NO_FMA one; best view and ratio are untouched; pixels without a prior and invalid
hypotheses keep their cost; weights 0 reproduce a whole run; the held array.  No GPU: tests/test_gpu_prior_call_parity.py and
tests/test_gpu_term_families.py hold the kernels to this oracle."""
import numpy as np
import pytest

import oracle_lib as ol
from test_geom_cpu import matrices64
from test_plane_prior_cpu import MAXCOST, add_plane_prior, default_params, hold_prior
from tsar_mvs_amd import synth

F32 = np.float32
HOLE = (slice(20, 32), slice(30, 46))          # 12 x 16 pixels of depth 0
NAN_AT = (5, 7)                                # one NaN normal
COMB_ALL, COMB_BEST_N = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes():
    return {3: synth.make_scene(64, 48, 3, seed=61, all_gt=True), 6: synth.make_scene(64, 48, 6, seed=62, all_gt=True)}


@pytest.fixture(scope="module")
def cpu_rcp_table():
    """the table FLAG_FAST_ARITH reads, here NOT the device's v_rcp_f32 (1 ulp) but 1 / z correctly rounded (numpy's float32 '/'):
    the CPU stand-in.  The term itself uses no reciprocal; the table only has to be the same with and without the prior."""
    z = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(F32)
    return (F32(1) / z).astype(F32)


def _oracle(sc, table=None, **kw):
    o = ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, **kw)
    if kw.get("flags", 0) & ol.FLAG_FAST_ARITH:
        o.set_rcp_table(table)
    return o


def _mats(sc):
    return [None] + [tuple(m.astype(F32) for m in matrices64(sc.K, sc.R, sc.t, v)) for v in range(1, len(sc.images))]


def _maps(sc):
    """every source view's ground-truth depth with a block of 0 (no estimate); the last view has no map"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
    maps[0] = None
    maps[-1] = None
    return maps


def _prior(sc, scale=1.01):
    """(depth, normal_world): ground truth scaled, a hole of depth 0 and one NaN normal"""
    depth = (sc.gt_depth.numpy().astype(np.float64) * scale).astype(F32)
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    depth[HOLE] = 0
    normal_world[NAN_AT] = np.nan
    return depth, normal_world


def held_prior(orc, depth, normal_world):
    """what the context holds for this prior: the depth as given and the normal taken to reference-camera coordinates as load_planes
    takes it (include/tsar.h), all zero where there is no prior.  Leaves the oracle's state as it found it."""
    saved = [a.copy() for a in (orc.norm4, orc.c, orc.depth)]
    with np.errstate(all="ignore"):
        orc.load_planes(np.where(np.asarray(depth) > 0, depth, F32(1)).astype(F32), normal_world)
    normal_cam = orc.norm4[..., :3].copy()
    for dst, src in zip((orc.norm4, orc.c, orc.depth), saved):
        dst[...] = src
    return hold_prior(depth, normal_cam)


def _planes(sc, orc, kind, depth_clip, prior_scale=1.01):
    """the planes of test_gpu_plane_prior.py::_test_planes, with the oracle's pm_init in place of the library's"""
    h, w = sc.gt_depth.shape
    gt = np.ascontiguousarray(synth.gt_planes(sc).numpy())
    if kind == "gt":
        return gt
    if kind == "random":
        orc.pm_init()
        return orc.norm4.copy()
    if kind == "outside":                                        # fronto-parallel, far outside both clips
        planes = np.zeros((h, w, 4), F32)
        planes[..., 2] = -1.0
        planes[..., 3] = F32(sc.depth_max) * F32(0.97)
        return planes
    # the prior's plane (ground truth scaled: a plane's depth at every pixel scales with its offset d) scaled again so that rel falls
    # within 1e-6 of depth_clip, on both sides
    ys, xs = np.mgrid[0:h, 0:w]
    delta = np.where((xs + ys) % 2 == 0, 5e-7, -5e-7)
    sign = np.where(xs % 2 == 0, 1.0, -1.0)
    planes = gt.copy()
    planes[..., 3] = (gt[..., 3].astype(np.float64) * prior_scale * (1.0 + sign * (float(depth_clip) + delta))).astype(F32)
    return planes


CONFIGS = [(11, 1, COMB_BEST_N, 3), (11, 3, COMB_BEST_N, 3), (15, 5, COMB_BEST_N, 6), (11, 1, COMB_ALL, 6)]   # box, n_best, comb, sources
FLAGS = {"strict": 0, "fast": ol.FLAG_FAST_ARITH, "fast8": ol.FLAGS_FAST_8BIT_IMAGERY}


@pytest.mark.parametrize("nofma", [False, True])
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("box,n_best,comb,n_src", CONFIGS)
def test_cost_planes_with_a_prior_is_the_restatement(scenes, cpu_rcp_table, box, n_best, comb, n_src, flags, nofma):
    """1-3 of the file's header, over ground truth, pm_init's planes, planes far outside both clips and planes at the clip's edge, with
    and without the geometric term"""
    sc = scenes[n_src]
    orc = _oracle(sc, cpu_rcp_table, box=box, n_best=n_best, cost_comb=comb, seed=5, flags=FLAGS[flags], nofma=nofma)
    params = default_params()
    held = held_prior(orc, *_prior(sc))
    assert not held[HOLE].any() and not held[NAN_AT].any() and (held[..., 3] > 0).mean() > 0.9
    mats, maps = _mats(sc), _maps(sc)
    for kind in ("gt", "random", "outside", "clip_edge"):
        planes = _planes(sc, orc, kind, params[2])
        D = orc.depth_from_planes(planes)
        for geom in (False, True):
            orc.clear_plane_prior()
            orc.clear_geom()
            if geom:
                orc.set_geom(maps, mats, weight=0.2, clip=3.0)
            c0, bv0, rt0 = orc.pm_cost_planes(planes)
            orc.set_plane_prior(held, params)
            c1, bv1, rt1 = orc.pm_cost_planes(planes)
            want = add_plane_prior(c0, bv0, held, planes, D, params)
            bad = _bits(c1) != _bits(want)
            assert not bad.any(), (kind, geom, int(bad.sum()), c1[bad][:4], want[bad][:4])
            assert np.array_equal(bv1, bv0) and np.array_equal(_bits(rt1), _bits(rt0))                  # 2. best view and ratio
            assert np.array_equal(_bits(c1[HOLE]), _bits(c0[HOLE])) and _bits(c1)[NAN_AT] == _bits(c0)[NAN_AT]   # 3. no prior
            invalid = bv0 < 0
            assert np.all(c0[invalid] == MAXCOST) and np.array_equal(_bits(c1[invalid]), _bits(c0[invalid]))   # 3. invalid
            paid = (_bits(c1) != _bits(c0))
            assert paid.mean() > 0.5, (kind, paid.mean())                                                 # the term is not idle
            if kind == "clip_edge":
                rel = np.abs(D - held[..., 3]) / np.where(held[..., 3] > 0, held[..., 3], 1)
                at = (held[..., 3] > 0) & (np.abs(rel - params[2]) < 1e-6)
                assert (rel[at] < params[2]).any() and (rel[at] >= params[2]).any() and at.mean() > 0.5
    assert not orc.rcp_out_of_range
    orc.clear_plane_prior()
    orc.clear_geom()


def test_an_invalid_hypothesis_keeps_maxcost_under_a_prior(scenes):
    """3, made certain: black images make every view's variance test fail, so every hypothesis is invalid (MAXCOST, best view -1) at
    pixels that do have a prior"""
    sc = scenes[3]
    flat = [np.zeros(sc.gt_depth.shape, F32) for _ in sc.images]            # (every weighted sum is exactly 0)
    orc = ol.Oracle(flat, sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=2, seed=5)
    real = _oracle(sc, box=11, n_best=2, seed=5)
    held = held_prior(real, *_prior(sc))
    orc.set_plane_prior(held, default_params())
    orc.set_geom(_maps(sc), _mats(sc), weight=0.2, clip=3.0)
    planes = np.ascontiguousarray(synth.gt_planes(sc).numpy())
    c, bv, rt = orc.pm_cost_planes(planes)
    assert np.all(bv == -1) and np.all(c == MAXCOST) and not rt.any()


@pytest.mark.parametrize("geom", [False, True])
@pytest.mark.parametrize("nofma", [False, True])
def test_both_weights_zero_reproduce_a_whole_run(scenes, geom, nofma):
    """4. pm_init + pm_iterate(3) with weight_depth = weight_normal = 0 is the run without a prior, bit for bit (t = +0 everywhere)"""
    sc = scenes[3]
    mats, maps = _mats(sc), _maps(sc)
    states = []
    for prior in (False, True):
        orc = _oracle(sc, box=11, n_best=2, seed=7, nofma=nofma)
        if geom:
            orc.set_geom(maps, mats, weight=0.2, clip=3.0)
        if prior:
            _, _, dc, nc = default_params()
            orc.set_plane_prior(held_prior(orc, *_prior(sc, 1.05)), (F32(0), F32(0), dc, nc))
        orc.pm_init()
        orc.pm_iterate(3)
        states.append((orc.norm4.copy(), orc.c.copy(), orc.beview.copy(), orc.ratio.copy()))
    for a, b in zip(*states):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_the_prior_moves_a_whole_run_and_clearing_it_restores_the_oracle(scenes):
    """the term reaches pm_init, the sweeps and rescore through pm_cost_multiview: a run under the prior differs from the photometric
    one at most pixels, every stored cost is pm_cost_planes of its plane under the prior, and after clear_plane_prior the oracle is
    bit for bit the one without a prior"""
    sc = scenes[3]
    plain = _oracle(sc, box=11, n_best=1, seed=7)
    plain.pm_init()
    first = plain.c.copy()
    plain.pm_iterate(3)
    orc = _oracle(sc, box=11, n_best=1, seed=7)
    held = held_prior(orc, *_prior(sc))
    orc.set_plane_prior(held, default_params())
    orc.pm_init()
    assert np.array_equal(_bits(orc.norm4), _bits(_planes(sc, _oracle(sc, box=11, n_best=1, seed=7), "random", 0)))   # the draw is the same
    assert (_bits(orc.c) != _bits(first)).mean() > 0.5 and np.array_equal(_bits(orc.c[HOLE]), _bits(first[HOLE]))
    orc.pm_iterate(3)
    moved = (_bits(orc.norm4) != _bits(plain.norm4)).any(-1).mean()
    assert moved > 0.9, moved
    c, bv, rt = orc.pm_cost_planes(orc.norm4.copy())
    assert np.array_equal(_bits(c), _bits(orc.c))
    # rescore's redraw scores the drawn plane with the term
    depth = sc.gt_depth.numpy().astype(F32).copy()
    depth[10:22, 20:36] = 0
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    orc.load_planes(depth, normal_world)
    orc.rescore()
    c, bv, rt = orc.pm_cost_planes(orc.norm4.copy())
    assert np.array_equal(_bits(c), _bits(orc.c)) and np.array_equal(bv, orc.beview) and np.array_equal(_bits(rt), _bits(orc.ratio))
    drawn = np.zeros(depth.shape, bool)
    drawn[10:22, 20:36] = True
    orc.clear_plane_prior()
    c0, _, _ = orc.pm_cost_planes(orc.norm4.copy())
    pays = drawn & (bv >= 0) & (held[..., 3] > 0)
    assert pays.sum() > 50 and np.all(c[pays] > c0[pays])
    orc.pm_init()
    orc.pm_iterate(3)
    assert np.array_equal(_bits(orc.norm4), _bits(plain.norm4)) and np.array_equal(_bits(orc.c), _bits(plain.c))


def test_the_held_array_is_hold_prior_of_load_planes_normals(scenes):
    """5. Dp is the caller's depth unchanged, q is load_planes's normal bit for bit (R n_world; close to the scene's camera-space
    normal), (0, 0, 0, 0) where the depth is not in (0, inf) or a normal component is not finite"""
    sc = scenes[3]
    orc = _oracle(sc)
    depth, normal_world = _prior(sc)
    depth[0, 0], depth[0, 1], depth[0, 2] = np.inf, -1.0, np.nan
    normal_world[1, 1, 2] = np.inf
    before = orc.norm4.copy()
    held = held_prior(orc, depth, normal_world)
    assert np.array_equal(_bits(orc.norm4), _bits(before))                   # (the oracle's state is left alone)
    none = np.zeros(depth.shape, bool)
    none[HOLE] = True
    none[NAN_AT] = True
    none[0, :3] = True
    none[1, 1] = True
    assert not held[none].any()
    orc.load_planes(sc.gt_depth.numpy().astype(F32), normal_world)
    assert np.array_equal(_bits(held[~none][:, :3]), _bits(orc.norm4[~none][:, :3]))
    assert np.array_equal(_bits(held[~none][:, 3]), _bits(depth[~none]))
    assert np.abs(held[~none][:, :3] - sc.gt_normal.numpy()[~none]).max() < 1e-5

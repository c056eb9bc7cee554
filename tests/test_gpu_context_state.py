"""The context's bookkeeping (tsar_dev.h: have_state, have_out, cost_consistent, sweeps_done), observed from outside through the C ABI,
so that the code that maintains it can move without changing what a caller sees.  96 x 64, 3 views, 8-bit imagery, box 5.

A. cost_consistent, through tsar_selftest_sweep_census, which takes the context's flag: on a state whose planes are all ONE plane with
   its depth inside the range, every arm present carries the pixel's own plane, so counter 4 (surviving arms) is 0 with the flag set
   and equals counter 7 (arms present, > 0) with it clear — exactly, for both colours.
B. sweeps_done, through results: it numbers the random streams of the next sweeps, so two contexts that differ only in the counter
   differ in their planes (asserted: the check can fail), and equal results show an equal counter.
C. have_out, through tsar_get_result's TSAR_ERR_STATE.

Two listed observations are not possible as worded and are replaced by the nearest ones that hold:
  - tsar_depth_to_plane rebuilds the plane offsets from the context's disparity plane, which tsar_compute_disp does not write (it
    writes the result buffer; the plane is zero after tsar_set_views and would give every pixel an invalid plane, none of whose arms
    survives whatever the flag).  tsar_getview writes it from the current planes, so the sequence is compute_disp, getview,
    depth_to_plane: the offsets come back as what they were, the field stays uniform and in range.
  - tsar_load_planes turns world normals by the reference camera's rotation, which is not the identity in the synthetic scenes:
    R (R^T n) has rounding in every component and the offsets then differ from pixel to pixel in the last bits.  The planes are one
    plane geometrically (every depth in range: the voided census holds exactly) but not bit for bit, so "rescore brings counter 4 to
    0" is shown from each of the other voided states and, after load_planes, from the same uniform planes set again.

An even box without TSAR_FLAG_FIX_INIT_RADIUS makes tsar_pm_init leave the flag clear (its window is not the sweeps').  The census
cannot see that on random planes; test_gpu_fast_exact.py::test_init_and_iterations_fast_bit_exact[12-1-0] holds an even box to the
oracle over init and three iterations, where a flag wrongly set skips a neighbour the reference scores and accepts, and
test_gpu_parity.py::test_init_strict_bit_exact holds the init windows of boxes 12, 10, (8, 11), 20 and 2."""
import numpy as np
import pytest

from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, N_SRC, BOX = 96, 64, 2, 5          # 3 views; the coarse level is 48 x 32
MODES = ["fast", "strict"]


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(W, H, N_SRC, seed=97, all_gt=True)


def _u8(sc):
    return [im.numpy().astype(np.uint8) for im in sc.images]


def _matcher(sc, mode, seed=5):
    m = api.Matcher()
    m.set_params(api.default_params(box_hsize=BOX, box_vsize=BOX, n_best=1, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV if mode == "strict" else 0, seed=seed))
    m.set_views(_u8(sc), sc.K, sc.R, sc.t, u8=True)
    return m


def _uniform(sc, w, h):
    """one fronto-parallel plane at mid-range depth: n = (0, 0, -1), n.X + d = 0"""
    p = np.zeros((h, w, 4), F32)
    p[..., 2] = -1.0
    p[..., 3] = F32(0.5) * (F32(sc.depth_min) + F32(sc.depth_max))
    return p


def _is_uniform(m):
    p = m.get_plane()[0].view(np.uint32).reshape(-1, 4)
    return bool((p == p[0]).all())


def _census(m):
    out = []
    for colour in (0, 1):
        c = m.selftest_sweep_census(colour)
        out.append((c["lane_survivors"], c["arms_present"]))
    return out


def _assert_voided(m, what):
    for colour, (alive, present) in enumerate(_census(m)):
        assert present > 0 and alive == present, f"{what}: colour {colour}: {alive} surviving arms of {present} present, expected all (costs not voided)"


def _assert_consistent(m, what):
    for colour, (alive, present) in enumerate(_census(m)):
        assert present > 0 and alive == 0, f"{what}: colour {colour}: {alive} surviving arms of {present} present, expected none"


def _maps(sc):
    return [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]


# ---- A. cost_consistent ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cost_consistent_single_context(scene, mode):
    sc = scene
    m = _matcher(sc, mode)
    P = _uniform(sc, W, H)
    zero = np.zeros((H, W), F32)
    m.set_plane(P, zero)
    _assert_voided(m, "set_plane")

    def rescored(after):
        m.rescore()                                    # the redraw form keeps a valid given plane
        assert _is_uniform(m), f"rescore after {after}: the field is no longer one plane"
        _assert_consistent(m, f"rescore after {after}")

    rescored("set_plane")

    def depth_to_plane():
        m.compute_disp()
        m.getview()                                    # writes the disparity plane that depth_to_plane reads (see the docstring)
        m.depth_to_plane()

    def set_same_planes():
        planes, cost, _, _ = m.get_plane()
        m.set_plane(planes, cost)

    voiders = [
        ("set_view_subset", lambda: m.set_view_subset([2])),
        ("set_geom_depths", lambda: m.set_geom_depths(_maps(sc))),
        ("clear_geom", m.clear_geom),                  # the term of the step before is installed
        ("depth_to_plane", depth_to_plane),
        ("set_plane", set_same_planes),
    ]
    for name, call in voiders:
        call()
        assert _is_uniform(m), name
        _assert_voided(m, name)
        rescored(name)
    # load_planes: the same plane as depth and world normal (one plane, but not bit for bit: see the docstring)
    depth = np.full((H, W), P[0, 0, 3], F32)
    normal_world = np.broadcast_to((np.array([0.0, 0.0, -1.0]) @ np.asarray(sc.R[0], np.float64)).astype(F32), (H, W, 3))
    m.load_planes(depth, np.ascontiguousarray(normal_world))
    _assert_voided(m, "load_planes")
    m.set_plane(P, zero)
    _assert_voided(m, "set_plane after load_planes")
    rescored("load_planes, set_plane")
    m.close()


@pytest.mark.parametrize("mode", MODES)
def test_cost_consistent_across_levels(scene, mode):
    sc = scene
    fine = _matcher(sc, mode)
    coarse = api.Matcher()
    coarse.pyramid_from(fine)
    assert (coarse.w, coarse.h) == (W // 2, H // 2)
    fine.set_plane(_uniform(sc, W, H), np.zeros((H, W), F32))
    # the coarse context: fine's planes at (2x, 2y), rescored
    coarse.pyramid_planes_from(fine)
    assert _is_uniform(coarse)
    _assert_consistent(coarse, "pyramid_planes_from")
    coarse.set_view_subset([2])
    _assert_voided(coarse, "coarse set_view_subset")
    coarse.pyramid_planes_from(fine)
    assert _is_uniform(coarse)
    _assert_consistent(coarse, "pyramid_planes_from on the voided coarse state")
    planes, cost, _, _ = coarse.get_plane()
    coarse.set_plane(planes, cost)
    _assert_voided(coarse, "coarse set_plane")
    coarse.rescore()
    assert _is_uniform(coarse)
    _assert_consistent(coarse, "coarse rescore")
    # the fine context: both levels hold the one plane, so whichever candidate wins, the field stays uniform
    _assert_voided(fine, "fine set_plane")
    fine.upsample_merge(coarse)
    assert _is_uniform(fine)
    _assert_consistent(fine, "upsample_merge")
    fine.set_view_subset([1])
    _assert_voided(fine, "fine set_view_subset")
    fine.upsample_merge(coarse)
    assert _is_uniform(fine)
    _assert_consistent(fine, "upsample_merge on the voided fine state")
    fine.close()
    coarse.close()


# ---- B. sweeps_done ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(a, b))


def _counter_run(sc, mode, call, counter):
    """pm_init, pm_iterate(1), the call under test, [set_sweep_counter(counter)], pm_iterate(1) on fresh contexts -> the state"""
    m = _matcher(sc, mode, seed=23)
    other = api.Matcher()
    if call == "pyramid_planes_from":                  # m is the coarse context
        fine = m
        fine.pm_init()
        fine.pm_iterate(1)
        m = other
        m.pyramid_from(fine)
        other = fine
    elif call in ("upsample_merge", "upsample_planes"):
        other.pyramid_from(m)
        other.pm_init()
        other.pm_iterate(1)
    m.pm_init()
    m.pm_iterate(1)
    if call in ("rescore",):
        m.rescore()
    elif call == "set_plane":
        planes, cost, _, _ = m.get_plane()
        m.set_plane(planes, cost)
    elif call == "load_planes":
        m.compute_disp()
        r = m.get_result(("depth", "normal"))
        m.load_planes(r["depth"], r["normal"])
    else:
        getattr(m, call)(other)
    if counter is not None:
        m.set_sweep_counter(counter)
    m.pm_iterate(1)
    out = m.get_plane()
    m.close()
    other.close()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("call", ["rescore", "pyramid_planes_from", "upsample_merge", "upsample_planes"])
def test_sweep_counter_is_reset(scene, mode, call):
    got = _counter_run(scene, mode, call, None)
    assert _same(got, _counter_run(scene, mode, call, 0)), f"{call} did not leave the sweep counter at 0"
    assert not _same(got, _counter_run(scene, mode, call, 2)), "the counter does not show in the result: the check above cannot fail"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("call", ["set_plane", "load_planes"])
def test_sweep_counter_is_kept(scene, mode, call):
    got = _counter_run(scene, mode, call, None)
    assert _same(got, _counter_run(scene, mode, call, 2)), f"{call} touched the sweep counter (2 after one iteration)"
    assert not _same(got, _counter_run(scene, mode, call, 0)), "the counter does not show in the result: the check above cannot fail"


# ---- C. have_out -------------------------------------------------------------------------------------------------------------------
def test_result_is_voided_by_every_state_change(scene):
    sc = scene
    m = _matcher(sc, "fast", seed=31)
    coarse = api.Matcher()
    coarse.pyramid_from(m)
    coarse.pm_init()

    def no_result(after):
        with pytest.raises(api.TsarError) as e:
            m.get_result(("depth",))
        assert e.value.code == api.TSAR_ERR_STATE and "tsar_compute_disp" in str(e.value), (after, str(e.value))

    def set_plane():
        planes, cost, _, _ = m.get_plane()
        m.set_plane(planes, cost)

    def load_planes():
        r = m.get_result(("depth", "normal"))
        m.load_planes(r["depth"], r["normal"])

    m.pm_init()
    no_result("pm_init")
    calls = [
        ("pm_init", m.pm_init),
        ("pm_iterate", lambda: m.pm_iterate(1)),
        ("pm_sweep", lambda: m.pm_sweep(0)),
        ("set_plane", set_plane),
        ("load_planes", load_planes),
        ("rescore", m.rescore),
        ("upsample_merge", lambda: m.upsample_merge(coarse)),
        ("wmf", lambda: m.wmf(1, False)),
    ]
    for name, call in calls:
        m.compute_disp()
        assert m.get_result(("depth",))["depth"].shape == (H, W)
        call()
        no_result(name)
    m.close()
    coarse.close()

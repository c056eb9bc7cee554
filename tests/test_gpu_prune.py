"""The sweep's partial-window pruning (kernels with variant bit 26, pm_tap_r5.h PRUNE / pm_sweep_impl.h pruned_cost) changes no
value: a wave leaves a refinement view only when the bound proves its cost >= cost_now for every lane, and repeats the hypothesis in
full when a lane accepts, so planes, costs, ratio, best view and the output maps are those of TSAR_PRUNE=0 bit for bit.  Checked with
the checks forced on from the first launch of the call (TSAR_PRUNE_FROM=0, steps 0-1), where cost_now is still high, on partial tiles
and every border, in the rolled and packed forms and both workgroup shapes; that the pruning kernels run only where a hypothesis's
cost is its best view's alone; and that views are in fact left on a converged state."""
import os

import numpy as np
import pytest

from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu

PRUNE_ON = {"TSAR_PRUNE": "1", "TSAR_PRUNE_FROM": "0", "TSAR_PRUNE_STEPS": "2"}
_SCENES = {}


def _scene(w, h):
    if (w, h) not in _SCENES:
        _SCENES[(w, h)] = synth.make_scene(w, h, 4, seed=33, all_gt=True)
    return _SCENES[(w, h)]


def _matcher(sc, env, n_best=1, strict=False):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:                                        # (the knobs are read once, when the context is created)
        m = api.Matcher()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=n_best, depth_min=sc.depth_min, depth_max=sc.depth_max,
                                    flags=api.FLAG_STRICT_DIV if strict else 0, seed=7))
    m.set_views([im.numpy().astype(np.uint8) for im in sc.images], sc.K, sc.R, sc.t, u8=True)
    return m


def _run(sc, env, iters, timing=False, **kw):
    m = _matcher(sc, env, **kw)
    if timing:
        m.enable_kernel_timing(True)
    m.pm_init()
    m.pm_iterate(iters)
    state = m.get_plane()                       # planes, cost, best view, ratio
    m.compute_disp()
    maps = m.get_result(("depth", "normal", "cost"))
    t = m.kernel_timing() if timing else None
    m.close()
    return list(state) + [maps[k] for k in ("depth", "normal", "cost")], t


def _assert_same(a, b):
    for k, (u, v) in enumerate(zip(a, b)):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), (k, int((u.view(np.uint32) != v.view(np.uint32)).sum()))


_BASE = {}


def _baseline(size, block, iters):
    key = (size, block, iters)
    if key not in _BASE:
        _BASE[key], t = _run(_scene(*size), {"TSAR_PRUNE": "0", "TSAR_BLOCK": block}, iters, timing=True)
        assert "pm_sweep_prune" not in t
    return _BASE[key]


@pytest.mark.parametrize("size", [(192, 128), (101, 67)])
@pytest.mark.parametrize("block", ["256", "128"])
@pytest.mark.parametrize("compact", ["2", None])
def test_pruned_run_is_the_unpruned_run_bit_for_bit(size, block, compact):
    env = dict(PRUNE_ON, TSAR_BLOCK=block)
    if compact:
        env["TSAR_COMPACT_FROM"] = compact
    got, t = _run(_scene(*size), env, 6, timing=True)
    assert t["pm_sweep_prune"][0] == 12, t
    assert ("pm_sweep_packed" in t) == True        # six iterations reach the packed form with either setting
    _assert_same(got, _baseline(size, block, 6))


@pytest.mark.parametrize("size", [(192, 128), (101, 67)])
def test_first_iteration_after_init_is_unchanged(size):
    """random planes, cost_now near 1 and above: the check must simply not fire wrongly"""
    got, t = _run(_scene(*size), dict(PRUNE_ON, TSAR_BLOCK="256"), 1, timing=True)
    assert t["pm_sweep_prune"][0] == 2
    _assert_same(got, _baseline(size, "256", 1))


def test_pruning_kernels_run_only_for_best_view_costs_in_fast_mode():
    sc = _scene(101, 67)
    for kw in ({"n_best": 2}, {"strict": True}):
        _, t = _run(sc, PRUNE_ON, 1, timing=True, **kw)
        assert "pm_sweep" in t and "pm_sweep_prune" not in t, (kw, t)
    m = _matcher(sc, PRUNE_ON)
    m.enable_kernel_timing(True)
    maps = [g[0].numpy().astype(np.float32).copy() for g in sc.meta["gt_all"]]
    m.set_geom_depths(maps, weight=0.2)
    m.pm_init()
    m.pm_iterate(1)
    t = m.kernel_timing()
    m.close()
    assert "pm_sweep_geom" in t and "pm_sweep_prune" not in t, t


def test_views_are_left_on_a_converged_state():
    sc = _scene(192, 128)
    m = _matcher(sc, dict(PRUNE_ON, TSAR_BLOCK="256"))
    m.pm_init()
    m.pm_iterate(6)
    m.selftest_prune_census(True)
    m.pm_iterate(1)
    k = m.selftest_prune_census(False)
    m.close()
    print("prune census, 192x128, iteration 7: [step][checked, views, views left, repeats] =", k[:2].tolist())
    waves = 2 * ((192 // 32) * (128 // 4))
    assert k[0, 0] > 0 and k[0, 0] <= waves and k[0, 1] == 4 * k[0, 0]
    assert k[0, 2] > 0, "no (wave, view) pair was left early at step 0"
    assert k[0, 3] <= k[0, 0] and k[2:].sum() == 0

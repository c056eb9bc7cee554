"""The paired gathers of the random-plane launches (pm_tap_r5.h PAIR, pm_pair.hip): fewer L1 look-ups, the same bits.

Taps 0, 2, 4 of a window row are gathered as 16 bytes; a lane whose next tap's entry is among those four takes it from there, the
others gather it as before.  The test is on element indices and every entry reaches the blend unchanged, so TSAR_PAIR=0 (the plain
kernels everywhere) and the default must agree bit for bit: after the initialisation, after the first iteration, and in the maps
compute_disp makes of that state.  Scenes: windows inside the sources; a camera step that sends border windows out of them (the
clamp loop, the last texture entries); partial tiles in x and y.  Both workgroup shapes of the sweep.  One leg keeps the
global-load kernels for three sweeps without pruning, so that the paired kernel also scores planes that have begun to cohere."""
import os

import numpy as np
import pytest

from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu

SCENES = {
    "inside": dict(w=150, h=101, n_src=3, seed=3),
    "windows leave the sources": dict(w=150, h=101, n_src=3, seed=3, step=0.2),
    "partial tiles": dict(w=70, h=45, n_src=2, seed=5),
}
_scene_cache = {}


def _scene(name):
    if name not in _scene_cache:
        kw = dict(SCENES[name])
        _scene_cache[name] = synth.make_scene(kw.pop("w"), kw.pop("h"), kw.pop("n_src"), **kw)
    return _scene_cache[name]


def _run(scene, env, iters):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = api.matcher_from_scene(scene, seed=77)          # the knobs are read once, by tsar_create
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m.enable_kernel_timing(True)
    m.pm_init()
    after_init = m.get_plane()[:2]
    m.pm_iterate(iters)
    state = m.get_plane()
    m.compute_disp()
    maps = m.get_result(want=("depth", "normal", "cost"))
    t = m.kernel_timing()
    m.close()
    return after_init, state, maps, t


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.shape == v.shape and u.dtype == v.dtype
        assert np.array_equal(u.view(np.uint32) if u.dtype.itemsize == 4 else u, v.view(np.uint32) if v.dtype.itemsize == 4 else v)


def _maps(r):
    return [r[k] for k in ("depth", "normal", "cost")] if isinstance(r, dict) else list(r)


@pytest.mark.parametrize("block", ["128", "256"])
@pytest.mark.parametrize("name", list(SCENES))
def test_paired_gathers_change_no_bit(name, block):
    sc = _scene(name)
    i0, s0, m0, t0 = _run(sc, {"TSAR_PAIR": "0", "TSAR_BLOCK": block}, 1)
    i1, s1, m1, t1 = _run(sc, {"TSAR_PAIR": "3", "TSAR_BLOCK": block}, 1)
    assert "pm_init_pair" not in t0 and "pm_sweep_pair" not in t0
    assert t1["pm_init_pair"][0] == 1 and t1["pm_sweep_pair"][0] == 1      # the first sweep of the run; the second reads the difference texture
    _same(i0, i1)
    _same(s0, s1)
    _same(_maps(m0), _maps(m1))
    assert (s0[1] < 1.0).mean() > 0.3                                       # the run scored textured pixels


@pytest.mark.parametrize("block", ["128", "256"])
def test_paired_sweeps_on_cohering_planes(block):
    """three sweeps on the global-load kernels (TSAR_BUFFER_FROM=3) without the pruning kernels: all three run paired"""
    sc = _scene("windows leave the sources")
    env = {"TSAR_BUFFER_FROM": "3", "TSAR_PRUNE": "0", "TSAR_BLOCK": block}
    i0, s0, m0, _ = _run(sc, dict(env, TSAR_PAIR="0"), 2)
    i1, s1, m1, t1 = _run(sc, dict(env, TSAR_PAIR="3"), 2)
    assert t1["pm_sweep_pair"][0] == 3
    _same(i0, i1)
    _same(s0, s1)
    _same(_maps(m0), _maps(m1))

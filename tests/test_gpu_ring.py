"""The ring form of the difference-texture sweep kernels (pm_tap_r5.h RING, pm_ring.hip; knob TSAR_RING): the unrolled clamp-free
walk with six gathers in flight across a view's six lines.  Every tap goes through the same arithmetic in the same order as in the
three-phase lines it replaces, so no bit of the state may differ.

TSAR_RING=0 against TSAR_RING=1, each in a fresh context (the knobs are read once, by tsar_create): planes, costs, ratio and best
view as 32-bit patterns after pm_init + one pm_iterate(4) with TSAR_COMPACT_FROM=2, so that the rolled kernel (launches 1), the
packed one (launches 2..7) and their pruning forms (from launch 1 on) all run; two source views (one drain and refill of the ring
per hypothesis) and ten (the benchmark's count), at both workgroup shapes (TSAR_BLOCK).  192 x 128: border waves take the clamp
loop, interior waves the ring.  One case is held to the CPU oracle's restatement of the fast arithmetic, and strict mode must not
launch a ring kernel at all.  kernel_timing() shows in every case whether the ring kernels ran."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu


def _run(scene, env, iters, flags=0, seed=77):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = api.matcher_from_scene(scene, box=11, n_best=1, seed=seed, flags=flags)      # the knobs are read once, by tsar_create
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m.enable_kernel_timing(True)
    m.pm_init()
    m.pm_iterate(iters)
    state = m.get_plane()
    t = m.kernel_timing()
    m.close()
    return state, t


def _same(a, b):
    assert len(a) == len(b) == 4
    for name, u, v in zip(("planes", "cost", "beview", "ratio"), a, b):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.shape == v.shape and u.dtype.itemsize == 4 and v.dtype.itemsize == 4, name
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), name


@pytest.fixture(scope="module", params=[2, 10], ids=["2 views", "10 views"])
def scene(request):
    return synth.make_scene(192, 128, request.param, seed=21)


@pytest.mark.parametrize("block", ["128", "256"])
def test_ring_changes_no_bit(scene, block):
    iters = 4
    env = {"TSAR_COMPACT_FROM": "2", "TSAR_BLOCK": block}
    off, t_off = _run(scene, dict(env, TSAR_RING="0"), iters)
    on, t_on = _run(scene, dict(env, TSAR_RING="1"), iters)
    assert "pm_sweep_ring" not in t_off
    # launch 0 of a run gathers from the byte texture with global loads; every later launch is a difference-texture kernel
    assert t_on["pm_sweep_ring"][0] == 2 * iters - 1
    for t in (t_off, t_on):
        assert t["pm_sweep"][0] == 2 * iters and t["pm_sweep_packed"][0] == 2 * iters - 2 and t["pm_sweep_prune"][0] == 2 * iters - 1
    _same(off, on)
    assert (on[1] < 2.0).mean() > 0.5                     # the run scored something


def test_default_rings_from_the_third_sweep_of_a_run():
    """TSAR_RING=n: from sweep n of a run on, counted from the initialisation like TSAR_BUFFER_FROM; the default is 3"""
    sc = synth.make_scene(192, 128, 2, seed=21)
    iters = 4
    off, _ = _run(sc, {"TSAR_RING": "0"}, iters)
    for env, first in (({}, 3), ({"TSAR_RING": "5"}, 5), ({"TSAR_RING": "1"}, 1)):
        old = os.environ.pop("TSAR_RING", None)
        try:
            on, t = _run(sc, env, iters)
        finally:
            if old is not None:
                os.environ["TSAR_RING"] = old
        assert t["pm_sweep_ring"][0] == 2 * iters - first, env
        _same(off, on)


def test_ring_against_the_oracle():
    sc = synth.make_scene(160, 120, 3, seed=21)
    f = api.Matcher()
    table = ol.rcp_table_from_device(f)
    f.close()
    got, t = _run(sc, {"TSAR_RING": "1"}, 2, seed=17)
    assert t["pm_sweep_ring"][0] == 3
    orc = ol.Oracle([im.numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, seed=17, flags=ol.FLAGS_FAST_8BIT_IMAGERY)
    orc.set_rcp_table(table)
    orc.pm_init()
    orc.pm_iterate(2)
    assert not orc.rcp_out_of_range
    _same(got, (orc.norm4, orc.c, orc.beview, orc.ratio))


def test_strict_mode_launches_no_ring_kernel():
    sc = synth.make_scene(192, 128, 2, seed=21)
    _, t = _run(sc, {"TSAR_RING": "1", "TSAR_COMPACT_FROM": "2"}, 2, flags=api.FLAG_STRICT_DIV)
    assert t["pm_sweep"][0] == 4 and "pm_sweep_ring" not in t

"""The partial-window bound of the sweep's pruning kernels (pm_tap_common.h prune_proven) on windows chosen to
sit at its rounding allowances, without a GPU.

tests/test_prune_bound_cpu.py holds the numpy restatement of the check (tools/prune_bound_census.py) to the oracle on one natural
scene, whose windows have mid-range texels and a variance in the hundreds: PM_PRUNE_E, PM_PRUNE_EA and PM_PRUNE_SLACK could be zero
there.  Here the windows are synthetic (adversarial_reference / adversarial_source): five reference classes (texels 246..255; a base
plus 0..5 with var_ref at the gate 2 PM_PRUNE_E; 0 or 255; 0..39 under a centre of 255 with every weight ~1e-6; 0..255) times four
source modes (the first 2-4 lines unrelated and the rest equal; the reference plus noise; the first three lines inverted; unrelated).
The truth is the fast arithmetic's cost of the whole window (full_window_cost: tap_accumulate<false>'s order and ncc_cost's tail),
and cost_now is put just above it: the next float, + 3e-5, + 1e-4, + 1e-3, + 1e-2.  Any proven verdict is then a false proof.

The fp32 cost differs from the float64 cost of the same window by up to 7e-3 (bright) and 1e-2 (lowvar) but 1e-4 on uniform texels:
on the first two classes the allowances carry the proof, and the last three tests show that the set fails when they are taken away."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("prune_bound_census", os.path.join(ROOT, "tools", "prune_bound_census.py"))
pbc = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pbc)

N = 20000
f32 = np.float32


def _census(cls, mode, **kw):
    return pbc.adversarial_census(cls, mode, N, np.random.default_rng(1), **kw)


@pytest.fixture(scope="module")
def census():
    return {(cls, mode): _census(cls, mode) for cls in pbc.REF_CLASSES for mode in pbc.SRC_MODES}


def test_the_set_is_the_one_described(census):
    """twenty combinations; the classes sit where they are meant to; cost_now is above the cost in every case"""
    assert len(census) == 20
    for (cls, mode), c in census.items():
        assert c["verdicts"].shape == (N, 5, pbc.LAST_LINE - pbc.FIRST_LINE + 1)
        for cn in pbc.cost_now_values(c["cost"]):
            assert cn.dtype == f32 and (cn > c["cost"]).all()
    p1 = {cls: float(np.percentile(census[(cls, "random")]["var_ref"], 1)) for cls in pbc.REF_CLASSES}
    print("first percentile of var_ref:", p1)
    gate = 3.0 * float(pbc.E_FULL)                                             # vr = var_ref - E >= 2 E
    shut = float((census[("lowvar", "random")]["var_ref"] < gate).mean())
    print("lowvar windows below the variance gate:", shut)
    assert 0.1 < shut < 0.9 and p1["lowvar"] < gate                            # on both sides: the lowest variances the check admits
    assert p1["bright"] < 10.0 and p1["uniform"] > 100.0
    r, cen = pbc.adversarial_reference(np.random.default_rng(1), 1000, "lonely")
    assert pbc.window_weights(r, cen).max() < 1e-5
    assert census[("bright", "noisy")]["max_err"] > 1e-3 and census[("lowvar", "noisy")]["max_err"] > 1e-3   # the allowances have work to do
    assert census[("uniform", "noisy")]["max_err"] < 1e-3


def test_no_window_is_proven_whose_cost_is_below_cost_now(census):
    verdicts = 0
    for (cls, mode), c in census.items():
        cost, var_ref = c["cost"], c["var_ref"]
        for k, cn in enumerate(pbc.cost_now_values(cost)):
            below = (cost < cn) & (var_ref >= f32(1e-5)) & (cost < f32(1.0))
            bad = c["verdicts"][:, k] & below[:, None]
            assert not bad.any(), (cls, mode, k, int(bad.sum()), float(cost[bad.any(axis=1)][0]), float(var_ref[bad.any(axis=1)][0]))
        verdicts += c["verdicts"].size
        print(cls, mode, "eligible", int(c["eligible"].sum()), "proven at 0.02", int(c["power"].any(axis=1).sum()), "max |fp32 - f64|", c["max_err"])
    print("verdicts:", verdicts)
    assert verdicts >= 1500000                                                 # a generator that silently shrinks cannot hide a failure


def test_the_bound_has_power_where_it_can(census):
    """At cost_now = 0.02 an unrelated source must be proven by the last check on uniform and on nearly weightless windows (else the
    check would be dead weight), and now and then on bright ones, where var_ref is a few units and the allowances eat most of the
    margin.  A binary window is never proven, by the variance gate: its centre is 0 or 255, the texels of the other value weigh
    exp(-255 / 18) ~ 7e-7, so the weighted variance is far below 2 PM_PRUNE_E = 1.8 (its first percentile is 0.02)."""
    share = {k: float(c["power"].any(axis=1).mean()) for k, c in census.items()}
    print({"/".join(k): round(v, 4) for k, v in share.items()})
    assert share[("uniform", "random")] > 0.9
    assert share[("lonely", "random")] > 0.9
    assert share[("bright", "random")] > 0.02
    for mode in pbc.SRC_MODES:
        c = census[("binary", mode)]
        assert not c["power"].any() and not c["verdicts"].any()
        assert (c["var_ref"] - pbc.E_FULL < f32(2.0) * pbc.E_FULL).all()       # the gate, not the bound


def _false_proofs(cls, mode, **kw):
    return int(_census(cls, mode, **kw)["false"].sum())


@pytest.mark.parametrize("cls", ["bright", "lowvar"])
def test_the_set_fails_without_the_rounding_allowances(cls, monkeypatch):
    """E_FULL = E_PART = SLACK = 0: the bound of exact arithmetic, applied to fp32 sums.  (If this stops failing after a change to
    the generators, the generators are wrong.)"""
    assert _false_proofs(cls, "noisy") == 0
    for name in ("E_FULL", "E_PART", "SLACK"):
        monkeypatch.setattr(pbc, name, f32(0.0))
    n = _false_proofs(cls, "noisy")
    print(cls, "noisy: false proofs without allowances:", n)
    assert n >= 1


def test_the_set_fails_on_a_misscaled_weight_sum():
    """the check's inv_wsum times 1.5 (a wrong normalisation of Q_A): where the first lines are unrelated and the rest matches, the
    bound is nearly an equality, and the factor breaks it"""
    n = _false_proofs("uniform", "tail", inv_wsum_scale=1.5)
    print("uniform tail: false proofs with inv_wsum * 1.5:", n)
    assert n >= 1

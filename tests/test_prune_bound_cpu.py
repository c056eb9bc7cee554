"""The partial-window bound of the sweep's pruning kernels (pm_tap_common.h prune_proven), without a GPU.

Soundness: the check, restated in numpy float32 as the kernel evaluates it (tools/prune_bound_census.py), is run on fresh refinement
hypotheses of the three widest steps around a converged oracle state, and every (pixel, hypothesis, view) it calls proven is held
against the CPU oracle's restatement of the fast arithmetic for that view (Oracle.pm_cost): none may score below the pixel's cost.
Power: at step 0 the share of proven (pixel, view) pairs must not be trivial.  Budget and identity: the pruning kernels fit 128
VGPRs without scratch, and every other sweep kernel is instruction for instruction what it was before the pruning change."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pbc = _tool("prune_bound_census")
isa = _tool("isa_identity")

W, H, N_SRC, DRAWS = 160, 120, 6, 3


@pytest.fixture(scope="module")
def census():
    """verdicts and oracle costs of DRAWS hypotheses per step (0, 1, 2) and pixel: every border pixel and every second pixel of
    every second row inside"""
    sc = synth.make_scene(W, H, N_SRC, seed=21)
    orc = pbc.fast_oracle(sc, 17, ol, pbc.exact_rcp_table())
    orc.pm_init()
    orc.pm_iterate(3)
    ys, xs = np.mgrid[0:H, 0:W]
    keep = (xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1) | ((xs % 2 == 1) & (ys % 2 == 1))
    xs, ys = xs[keep], ys[keep]
    rng = np.random.default_rng(11)
    out = {}
    for step in (0, 1, 2):
        out[step] = [pbc.census(orc, sc, xs, ys, step, rng) for _ in range(DRAWS)]
    assert not orc.rcp_out_of_range
    return out, (xs, ys)


def test_no_proven_view_scores_below_the_pixels_cost(census):
    out, (xs, ys) = census
    samples = proven = 0
    border = (xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1)
    for step, draws in out.items():
        for verdict, costs, cost_now, _ in draws:
            any_check = verdict.any(axis=2)                        # proven at any of the checks: the view would be left there
            bad = any_check & (costs < cost_now[:, None])
            assert not bad.any(), (step, int(bad.sum()), float((cost_now[:, None] - costs)[bad].max()))
            samples += any_check.size
            proven += int(any_check.sum())
            assert any_check[border].size > 0
    print("samples (pixel, hypothesis, view):", samples, "proven:", proven, "border pixels:", int(border.sum()))
    assert samples >= 200000


def test_the_bound_has_power_at_the_widest_step(census):
    """A step-0 hypothesis turns the normal by up to 1 per component and moves the disparity by up to half its range: the source
    window is unrelated to the reference window, 1 - ncc^2 is near 1 over any part of it, and the threshold 1 - (1 - cost_now)^2
    is a few per cent on a converged pixel.  So the bound must prove most such views by the fourth line (two thirds of the taps):
    below one half, the kernels' vote over 64 lanes would never carry and the check would be dead weight.  Observed here: see the
    printed shares (the 768 x 512 census of profiles/prune/README.md has .84 / .96 / .98 after 2 / 3 / 4 lines at step 0)."""
    out, _ = census
    for step in (0, 1, 2):
        v = np.concatenate([d[0] for d in out[step]])
        cum = np.logical_or.accumulate(v, axis=2).mean(axis=(0, 1))
        print("step", step, "share of (pixel, view) pairs proven after 2 / 3 / 4 lines:", [round(float(c), 3) for c in cum])
        if step == 0:
            assert cum[-1] >= 0.5
    near, wide = np.concatenate([d[0] for d in out[2]]), np.concatenate([d[0] for d in out[0]])
    assert near.any(axis=2).mean() < wide.any(axis=2).mean()           # near the pixel's plane the bound says little


def test_a_lane_that_must_not_be_proven_never_is():
    """cost_now >= 1 (and MAXCOST, which also stands for "this lane has seen a view below its cost"), a reference window whose
    variance is within the rounding bound, non-finite sums: all fail"""
    rng = np.random.default_rng(3)
    n = 4096
    wt = rng.uniform(0.05, 1.0, (n, 6, 6)).astype(np.float32)
    r = rng.integers(0, 256, (n, 6, 6)).astype(np.float32)
    s = rng.integers(0, 256, (n, 6, 6)).astype(np.float32)                  # unrelated to r: provable where allowed
    inv_wsum = (np.float32(1.0) / wt.sum(axis=(1, 2))).astype(np.float32)
    mean = (wt * r).sum(axis=(1, 2)) * inv_wsum
    var_ref = ((wt * r * r).sum(axis=(1, 2)) * inv_wsum - mean * mean).astype(np.float32)
    ok = pbc.proven_after_lines(wt, r, s, inv_wsum, var_ref, np.full(n, 0.02, np.float32))
    assert ok[:, -1].mean() > 0.9
    for cost_now in (1.0, 1.5, 2.0):
        assert not pbc.proven_after_lines(wt, r, s, inv_wsum, var_ref, np.full(n, cost_now, np.float32)).any()
    assert not pbc.proven_after_lines(wt, r, s, inv_wsum, np.full(n, 1.5, np.float32), np.full(n, 0.02, np.float32)).any()
    flat = np.full_like(s, 77.0)                                            # a source window without variance
    assert not pbc.proven_after_lines(wt, r, flat, inv_wsum, var_ref, np.full(n, 0.02, np.float32)).any()
    bad = s.copy(); bad[:, 0, 0] = np.nan
    assert not pbc.proven_after_lines(wt, r, bad, inv_wsum, var_ref, np.full(n, 0.02, np.float32)).any()
    same = pbc.proven_after_lines(wt, r, r, inv_wsum, var_ref, np.full(n, 0.02, np.float32))      # s = r: ncc = 1, cost 0 < cost_now
    assert not same.any()


HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def sweep_listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "pm_sweep.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "pm_sweep.hip"), str(out)], check=True, capture_output=True, timeout=900)
    return str(out)


PRUNE_BIT = 1 << 26


def _variant(name):
    m = re.search(r"pm_sweep_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELi(\d+)ELb([01])E", name)
    return int(m.group(5)), int(m.group(6)), m.group(7) == "1"


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_pruning_kernels_fit_four_waves_per_simd(sweep_listing):
    budgets = isa.kernel_budgets(sweep_listing)
    seen = set()
    for name, (vgpr, scratch) in budgets.items():
        if "pm_sweep_kernel" not in name or not (_variant(name)[0] & PRUNE_BIT):
            continue
        v, blk, packed = _variant(name)
        seen.add((v & ~PRUNE_BIT, blk, packed))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs (four waves per SIMD need <= 128)"
    # 250, + buffer loads, + the difference texture; both workgroup shapes; rolled and packed
    assert seen == {(v, b, p) for v in (250, 250 | 131072, 250 | 131072 | 2097152) for b in (128, 256) for p in (False, True)}, seen


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_every_other_sweep_kernel_is_instruction_identical_to_its_parent(sweep_listing):
    """profiles/prune/isa_non_prune_parent.txt: tools/isa_identity.py on the parent commit's listing (same compiler)"""
    now = isa.kernel_hashes(sweep_listing)
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "prune", "isa_non_prune_parent.txt")):
        name, sha, n = line.split()
        rec[name] = (sha, int(n))
    assert len(rec) == 112
    others = {k: v for k, v in now.items() if not (_variant(k)[0] & PRUNE_BIT)}
    assert set(others) == set(rec)
    changed = [k for k in rec if others[k] != rec[k]]
    assert not changed, changed[:4]

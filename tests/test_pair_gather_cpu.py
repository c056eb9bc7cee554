"""The paired-gather kernels of the random-plane launches (pm_pair.hip, pm_tap_r5.h PAIR), without a GPU.

Budget: every kernel of pm_pair.hip keeps four waves per SIMD (<= 128 VGPRs, no scratch) and carries the 16-byte gather.  Identity:
the every-pixel units (pm_init, pm_upsample and their general-window units) emit, kernel for kernel, the instructions they emitted
before the change (profiles/pair_gather/isa_parent.txt: tools/isa_identity.py on the parent commit's listings, same compiler);
tests/test_prune_bound_cpu.py holds pm_sweep.hip.  Premise: on the bench cameras, with planes drawn as the initialisation draws
them, the 16 bytes at a row tap's entry hold the next tap's entry for more than 0.8 of the pairs (tools/pair_gather_census.py)."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsar-mvs_amd", "csrc")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


isa = _tool("isa_identity")
census = _tool("pair_gather_census")

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")


def _listing(tmp, unit):
    out = tmp / (unit + ".s")
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(CSRC, unit + ".hip"), str(out)], check=True, capture_output=True, timeout=900)
    return str(out)


def _kernel_bodies(path):
    txt = open(path).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)}


@pytest.fixture(scope="module")
def pair_listing(tmp_path_factory):
    return _listing(tmp_path_factory.mktemp("isa_pair"), "pm_pair")


PAIR_BIT = 1 << 27


@needs_hipcc
def test_paired_kernels_fit_four_waves_per_simd(pair_listing):
    budgets = isa.kernel_budgets(pair_listing)
    assert len(budgets) == 3, sorted(budgets)                    # the initialisation; the sweep at both workgroup shapes
    for name, (vgpr, scratch) in budgets.items():
        v = int(re.search(r"ELb[01]ELb[01](?:ELb[01])?ELi(\d+)", name).group(1))
        assert v == (250 | PAIR_BIT), name
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs (four waves per SIMD need <= 128)"
    assert sum("pm_full_kernel" in n for n in budgets) == 1
    assert {re.search(r"ELi(\d+)ELb0EEv", n).group(1) for n in budgets if "pm_sweep_kernel" in n} == {"128", "256"}


@needs_hipcc
def test_paired_kernels_carry_the_wide_gather(pair_listing):
    bodies = _kernel_bodies(pair_listing)
    kernels = isa.kernel_budgets(pair_listing)
    for name in kernels:
        # both tap loops (clamp and clamp-free) gather three times 16 bytes per line from the pinned base
        wide = re.findall(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", bodies[name])
        assert len(wide) >= 6, (name, len(wide))


@needs_hipcc
@pytest.mark.parametrize("unit", ["pm_init", "pm_init_lut", "pm_upsample", "pm_upsample_lut"])
def test_every_pixel_units_are_instruction_identical_to_the_parent(unit, tmp_path):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "pair_gather", "isa_parent.txt")):
        u, name, sha, n = line.split()
        if u == unit + ".hip":
            rec[name] = (sha, int(n))
    assert rec
    path = _listing(tmp_path, unit)
    now = isa.kernel_hashes(path, prefix="_Z")
    kernels = set(isa.kernel_budgets(path))
    assert kernels == set(rec)
    changed = [k for k in rec if now[k] != rec[k]]
    assert not changed, changed[:4]


def test_most_pairs_are_covered_on_the_bench_cameras():
    r = census.census(6048, 4032, 10, pixels=20000, seed=1)
    print(r)
    assert r["pairs"] > 100000
    assert r["covered"] > 0.8

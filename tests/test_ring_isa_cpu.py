"""Register budget of the ring sweep kernels (tsar-mvs_amd/csrc/pm_ring.hip, variant bit TSAR_V_RING), from the assembler's kernel
metadata alone: four waves per SIMD need at most 128 VGPRs, and a kernel that spilled to scratch would stay bit-exact and lose the
time the ring is there to gain.  Runs without a GPU: hipcc cross-compiles the unit for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING_BIT, PRUNE_BIT = 1 << 28, 1 << 26
BASE = 250 | 131072 | 2097152                    # the fast row-wise loop, buffer loads, the difference texture


def test_ring_kernels_fit_four_waves_per_simd_without_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "tsar-mvs_amd", "csrc", "pm_ring.hip")
    out = str(tmp_path / "pm_ring.s")
    try:
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S",
                        src, "-o", out], check=True, capture_output=True, timeout=900)
    except FileNotFoundError:
        pytest.skip("hipcc not available")
    txt = open(out).read()
    seen = set()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        k = re.search(r"pm_sweep_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELi(\d+)ELb([01])E", name)
        assert k, name                           # the unit holds sweep kernels only
        nb, hr, strict, quad, v, blk, packed = int(k.group(1)), int(k.group(2)), k.group(3) == "1", k.group(4) == "1", int(k.group(5)), int(k.group(6)), k.group(7) == "1"
        assert v & RING_BIT and (v & ~(RING_BIT | PRUNE_BIT)) == BASE and (nb, hr, strict, quad) == (2, 5, False, True), name
        seen.add((bool(v & PRUNE_BIT), blk, packed))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs (four waves per SIMD need <= 128)"
    # plain and pruning; both workgroup shapes; rolled and packed
    assert seen == {(p, b, c) for p in (False, True) for b in (128, 256) for c in (False, True)}, seen

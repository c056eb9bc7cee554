"""Register budget of the kernels of tsar-mvs_amd/csrc/cloud_neighbor_kernels.hip, from the assembler's kernel metadata alone: the sorted list
of the k smallest distances must live in registers (a list indexed at run time, or one that no longer fits, would go to scratch, stay
bit-exact and lose the time), and the 32-entry list must leave room for four waves per SIMD.  Runs without a GPU: tools/isa.sh
cross-compiles the unit for gfx950."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_neighbor_kernels_use_no_scratch_and_the_longest_list_fits_128_vgprs(tmp_path):
    out = tmp_path / "cloud_neighbor_kernels.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "cloud_neighbor_kernels.hip"), str(out)], check=True,
                   capture_output=True, timeout=900)
    caps, others = {}, set()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        name, body = m.group(1), m.group(2)
        assert "rocprim" not in name, name             # the sort is cloud_grid.hip's: none of its kernels is compiled into this unit
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        k = re.search(r"cn_search_kernelILi(\d+)E", name)
        if k:
            caps[int(k.group(1))] = vgpr
        else:
            others.add(re.search(r"(c[dn]_[a-z_]+_kernel)", name).group(1))
    assert sorted(caps) == [0, 4, 8, 16, 32], caps           # the count-only kernel and one list length per template instance
    assert caps[32] <= 128, f"the 32-entry list takes {caps[32]} VGPRs (four waves per SIMD need <= 128)"
    assert others == {"cn_fill_kernel"}, others      # (the bounds, keys, gather and pair-count kernels are cloud_grid.hip's)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_shared_pair_count_kernel_uses_no_scratch(tmp_path):
    """cd_self_pairs_kernel, which counts the pairs for this unit and for cloud_normal_kernels.hip, is compiled in cloud_grid.hip"""
    out = tmp_path / "cloud_grid.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "cloud_grid.hip"), str(out)], check=True, capture_output=True,
                   timeout=900)
    found = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        name, body = m.group(1), m.group(2)
        if "rocprim" in name:
            continue
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        found += "cd_self_pairs_kernel" in name
    assert found == 1

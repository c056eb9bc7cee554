"""Register budget of the kernels of tsar-mvs_amd/csrc/cloud_normal_kernels.hip, from the assembler's kernel metadata alone: the sorted list of
the k smallest 64-bit codes, the moments and the Jacobi state must live in registers (a list or a matrix indexed at run time would go to
scratch, stay bit-exact and lose the time), and the 32-entry instance must leave room for four waves per SIMD.  Runs without a GPU:
tools/isa.sh cross-compiles the unit for gfx950."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_normal_kernels_use_no_scratch_and_the_longest_list_fits_128_vgprs(tmp_path):
    out = tmp_path / "cloud_normal_kernels.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "cloud_normal_kernels.hip"), str(out)], check=True,
                   capture_output=True, timeout=900)
    caps, others = {}, set()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        name, body = m.group(1), m.group(2)
        assert "rocprim" not in name, name             # the sort is cloud_grid.hip's: none of its kernels is compiled into this unit
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        k = re.search(r"nr_normals_kernelILi(\d+)E", name)
        if k:
            caps[int(k.group(1))] = vgpr
        else:
            others.add(re.search(r"(nr_[a-z_]+_kernel)", name).group(1))
    assert sorted(caps) == [8, 16, 32], caps                 # one list length per template instance
    assert caps[32] <= 128, f"the 32-entry instance takes {caps[32]} VGPRs (four waves per SIMD need <= 128)"
    assert others == {"nr_fill_kernel", "nr_compare_kernel"}, others      # (the pair count is cloud_grid.hip's: tests/test_neighbors_isa_cpu.py)

"""Register budget of the render kernels of tsar-mvs_amd/csrc/cloud_render_kernels.hip (the square and the oriented render share the unit), from
the assembler's kernel metadata alone: in the oriented scatter the per-point terms (a, num, g), the per-row terms and M live in registers across
the footprint loop; nothing may go to scratch, no render kernel uses LDS, and every one must leave room for eight waves per SIMD (64 VGPRs;
the compiler takes 33 in the oriented scatter).  depth_compare_kernel of the same unit keeps its waves' partial counts in LDS by design: it
is held to no scratch only.  Runs without a GPU: tools/isa.sh cross-compiles the unit for gfx950."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_splat_kernels_use_no_scratch_no_lds_and_at_most_64_vgprs(tmp_path):
    out = tmp_path / "cloud_render_kernels.s"
    subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", "cloud_render_kernels.hip"), str(out)], check=True,
                   capture_output=True, timeout=900)
    found, others = {}, set()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        name, body = m.group(1), m.group(2)
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        render = re.search(r"(cloud_(?:render|splat)_[a-z]+_kernel)", name)
        if not render:
            others.add(name)
            continue
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        found.setdefault(render.group(1), []).append(vgpr)
    print("VGPRs:", found)
    assert sorted(found) == ["cloud_render_count_kernel", "cloud_render_resolve_kernel", "cloud_render_scatter_kernel", "cloud_render_support_kernel",
                             "cloud_splat_scatter_kernel"], found
    assert len(others) == 1 and "depth_compare_kernel" in others.pop()
    assert len(found["cloud_splat_scatter_kernel"]) == 2                       # with and without the load that lets a lane skip an atomic
    assert max(max(v) for v in found.values()) <= 64, found

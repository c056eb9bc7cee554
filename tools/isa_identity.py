#!/usr/bin/env python3
"""tools/isa_identity.py <listing.s> — one line per pm_sweep kernel of a tools/isa.sh listing: its name, the SHA-256 of its
instruction stream (comments, directives and the function's number in local labels removed) and the instruction count.  Two builds
whose lines agree for a kernel emit the same machine code for it; tests/test_prune_bound_cpu.py holds the kernels without variant bit
26 to the record taken at the parent of the pruning change (profiles/prune/isa_non_prune_parent.txt)."""
import hashlib
import re
import sys


def kernel_hashes(path, prefix="_Z15pm_sweep_kernel"):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(" + re.escape(prefix) + r"\S+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        lines = [re.sub(r"LBB[0-9]+_", "LBB_", ln.split(";")[0].rstrip()) for ln in m.group(2).splitlines()]
        lines = [ln for ln in lines if ln.strip() and (not ln.strip().startswith(".") or ln.strip().startswith(".LBB"))]
        out[m.group(1)] = (hashlib.sha256("\n".join(lines).encode()).hexdigest(), sum(1 for ln in lines if not ln.startswith(".")))
    return out


def kernel_budgets(path):
    """name -> (VGPRs, scratch bytes per lane) from the assembler's metadata"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        body = m.group(2)
        out[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    return out


if __name__ == "__main__":
    for name, (sha, n) in sorted(kernel_hashes(sys.argv[1]).items()):
        print(name, sha, n)

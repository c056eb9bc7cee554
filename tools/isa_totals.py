#!/usr/bin/env python3
"""tools/isa_totals.py <file.s> plain|geom — per sweep kernel of an assembly file written by tools/isa.sh: registers, LDS, scratch and
instruction totals (all, and by the first word of the mnemonic), for the kernels without (plain) or with (geom) variant bit 24.  Two
listings of the same selection, before and after a change, compare with cmp.  No GPU."""
import re
import sys


def main():
    txt = open(sys.argv[1]).read()
    want_geom = sys.argv[2] == "geom"
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        g = lambda k: (re.search(r"\." + k + r" (\S+)", body) or [None, "?"])[1]
        meta[name] = (g("amdhsa_next_free_vgpr"), g("amdhsa_next_free_sgpr"), g("amdhsa_group_segment_fixed_size"), g("amdhsa_private_segment_fixed_size"))
    for name in sorted(meta):
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)
        ins = [ln.split()[0] for ln in m.group(1).splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
        v = re.search(r"pm_sweep_kernelILi\d+ELi\d+ELb[01]ELb[01]ELi(\d+)E", name)
        if bool(v and int(v.group(1)) & (1 << 24)) != want_geom:
            continue
        kinds = {}
        for i in ins:
            kinds[i.split("_")[0]] = kinds.get(i.split("_")[0], 0) + 1
        print(name)
        print("   vgpr %s sgpr %s lds %s scratch %s instructions %d (%s)" % (*meta[name], len(ins), " ".join(f"{k} {n}" for k, n in sorted(kinds.items()))))


if __name__ == "__main__":
    main()

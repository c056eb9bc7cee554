"""Build-time guard for the rule the coarse-to-fine and geometric-consistency passes rest on: the every-pixel operators choose the
same tap loop for the same context, so a candidate's score in tsar_upsample_planes / tsar_upsample_merge / tsar_pm_rescore is
tsar_pm_cost_planes's.  All of them pick their template arguments through csrc/pm_dispatch.h; a selector instantiates one kernel per
configuration it can choose, so the configurations an operator can run are the kernels its translation units contain.  Runs without
a GPU: hipcc cross-compiles the four every-pixel units and the test compares the sets of instantiated configurations."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ["pm_init.hip", "pm_init_lut.hip", "pm_upsample.hip", "pm_upsample_lut.hip"]
V_GEOM, V_REDRAW = 1 << 24, 1 << 25      # csrc/tsar_dev.h TSAR_V_GEOM, TSAR_V_REDRAW

# pm_full_kernel<NB, HR, STRICT, QUAD, INIT, V> and pm_upsample_kernel<NB, HR, STRICT, QUAD, V, MERGE>
FULL = re.compile(r"pm_full_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELi(\d+)EE")
UP = re.compile(r"pm_upsample_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])EE")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_every_pixel_operators_instantiate_the_same_configurations(tmp_path):
    init, cost, rescore, plain, merge = set(), set(), set(), set(), set()
    n_kernels = 0
    for unit in UNITS:
        out = tmp_path / (unit + ".s")
        subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), os.path.join(ROOT, "tsar-mvs_amd", "csrc", unit), str(out)], check=True, capture_output=True, timeout=900)
        for name in re.findall(r"\.amdhsa_kernel (\S+)", out.read_text()):
            n_kernels += 1
            m = FULL.search(name)
            if m:
                nb, hr, strict, quad, is_init, v = (int(g) for g in m.groups())
                (rescore if v & V_REDRAW else init if is_init else cost).add((nb, hr, strict, quad, v & ~V_REDRAW))
                assert not (v & V_REDRAW) or (is_init and v & V_GEOM), name      # the redrawing form is an initialising one and carries the term
                continue
            m = UP.search(name)
            assert m, f"{unit}: a kernel that is neither pm_full_kernel nor pm_upsample_kernel: {name}"
            nb, hr, strict, quad, v, is_merge = (int(g) for g in m.groups())
            (merge if is_merge else plain).add((nb, hr, strict, quad, v))
    base = {c for c in cost if not c[4] & V_GEOM}
    with_geom = {c[:4] + (c[4] | V_GEOM,) for c in base}
    assert cost == base | with_geom, "tsar_pm_cost_planes: a configuration exists with the geometric term and not without it, or the reverse"
    assert merge == cost, sorted(merge ^ cost)
    assert init == cost, sorted(init ^ cost)
    assert plain == base, sorted(plain ^ base)                   # (tsar_upsample_planes never runs with a term installed)
    assert rescore == with_geom, sorted(rescore ^ with_geom)     # (tsar_pm_rescore always carries the term's code)
    # 21 box-11 / float-imagery configurations (16 of the one-tap loop, 5 of the box-11 loop) + 18 general-window ones
    assert len(base) == 39, sorted(base)
    assert n_kernels == 8 * len(base)     # init and merge 2 each, cost 2, rescore 1, plain 1 per configuration: no other kernel in these units

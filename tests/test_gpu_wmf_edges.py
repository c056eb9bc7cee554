"""The weighted median filter kernels (wmf_kernels.hip, through tsar_wmf) against the CPU oracle on the inputs of wmf_cases.py — fill
passes 4-6 (radius 40 / 80 / 160, gap 8 / 16 / 32, the scalar tap offsets of the interior path at gap 32), full windows (num == 121:
122 valid entries through the sorting network, rank 121 of LDS, the last walk batch), nearly empty windows (num = 1, 2, 3: the zero
slot of SURVEY quirk 12 decides), lists of ties with +-0 and fp32 denormals (the stable order of the reference's `>` bubble sort),
+-inf in the depth list, fill waves with one or four active lanes, images narrower than a tap gap — every pixel, bit for bit.
test_wmf_edges_cpu.py holds the same oracle to the reference's text on the same inputs.

NaN tap VALUES stay outside the parity claim: the reference's `>` sort defines no order for them (the kernel places them last).  NaN
RESULTS (0 / 0 in a normalisation, inf - inf) are compared as NaN against NaN, only where the oracle's element is NaN."""
import numpy as np
import pytest

import wmf_cases as wc
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu

_records = {}


def _record(name):
    """the oracle's run over the case: computed once, shared, left unchanged"""
    if name not in _records:
        _records[name] = wc.run_oracle(wc.case(name))       # (asserts the case's conditions)
    return _records[name]


def _matcher(c, flags=api.FLAG_STRICT_DIV):
    return api.matcher_from_scene(c["scene"], seed=wc.SEED, flags=flags)


def _load(m, c, mask=None):
    """the case's state: planes, lines->depth through getview, reliability mask, regions"""
    h, w = c["mask"].shape
    m.set_plane(c["planes"], np.zeros((h, w), np.float32))
    m.getview()
    m.set_reliable_mask(c["mask"] if mask is None else mask)
    m.set_regions(c["labels"], c["region_text"])


def _where(ok):
    bad = np.argwhere(~ok)
    return int(len(bad)), bad[:5].tolist()


class _Findings(list):
    """every comparison of a test prints its figure and is recorded; the test asserts at its end that none failed"""

    def check(self, ok, what, plane):
        print(what, plane + ": mismatching elements", int((~ok).sum()))
        if not ok.all():
            self.append((what, plane) + _where(ok))

    def mask(self, m, want, what):
        self.check(m.get_reliable_mask().view(np.uint32) == want.view(np.uint32), what, "reliability mask")

    def fill_state(self, m, want, what):
        """planes, reliability mask and the depth compute_disp derives, against the oracle's state after the same passes"""
        self.check(wc.same_bits(m.get_plane()[0], want["norm4"]), what, "planes (NaN in the oracle's: %d)" % int(np.isnan(want["norm4"]).sum()))
        self.mask(m, want["scale"], what)
        m.compute_disp()
        self.check(wc.same_bits(m.get_result(("depth",))["depth"], want["disp"]), what, "depth")


def _run_case(name, flags):
    c, rec = wc.case(name), _record(name)
    found = _Findings()
    m = _matcher(c, flags)
    _load(m, c, c.get("detect_mask"))
    m.wmf(4, False)
    found.mask(m, rec["detect_scale"], name + " after wmf(4, False):")
    for start in c["fill_from"]:
        if start == "mask":
            _load(m, c)
        m.wmf(c["fill_passes"], True)
        found.fill_state(m, rec["fill"][start][-1], "%s after wmf(%d, True) from %s:" % (name, c["fill_passes"], start))
    m.close()
    assert not found, found


@pytest.mark.parametrize("name", wc.NAMES)
def test_detection_and_fill_bit_exact(name):
    _run_case(name, api.FLAG_STRICT_DIV)


@pytest.mark.parametrize("name", wc.BELOW_THE_ABI)
def test_images_below_8_by_8_are_refused(name):
    """7 x 5 and 33 x 3 never reach the kernels: tsar_set_views refuses them (the oracle's side of them: test_wmf_edges_cpu.py)"""
    with pytest.raises(api.TsarError) as e:
        _matcher(wc.case(name))
    assert e.value.code == api.TSAR_ERR_INVALID


def test_full_windows_without_strict_div():
    """the filter has no mode-dependent arithmetic: the same bits from a context of the default mode"""
    _run_case("full", 0)


@pytest.mark.parametrize("k", [4, 5, 6])
def test_fill_passes_4_to_6_each_from_a_fresh_state(k):
    """tsar_wmf restarts at it = 0 on every call: the state after pass k - 1 is wmf(k, True) from the case's state, against the
    oracle's first k passes (islands that pass k - 1 alone rewrites, one with its window inside the image, one clamped)"""
    c, rec = wc.case("six_passes"), _record("six_passes")
    assert int(rec["fill"]["mask"][k - 1]["rewritten"].sum()) >= 32
    found = _Findings()
    m = _matcher(c)
    _load(m, c)
    m.wmf(k, True)
    found.fill_state(m, rec["fill"]["mask"][k - 1], "six_passes after wmf(%d, True):" % k)
    m.close()
    assert not found, found


def test_sparse_windows_pass_by_pass():
    """num = 1, 2, 3 at passes 4 and 5: the targets that pass 4 rewrites and those that only pass 5 reaches (the zero-slot branch)"""
    c, rec = wc.case("sparse"), _record("sparse")
    found = _Findings()
    m = _matcher(c)
    for k in (5, 6):
        _load(m, c)
        m.wmf(k, True)
        found.fill_state(m, rec["fill"]["mask"][k - 1], "sparse after wmf(%d, True):" % k)
    m.close()
    assert not found, found


def test_pass_counts_beyond_the_reference_are_refused():
    """more passes than the reference runs (4 detection, 6 fill) are TSAR_ERR_INVALID, and the context serves the full counts after"""
    c, rec = wc.case("sparse"), _record("sparse")
    found = _Findings()
    m = _matcher(c)
    _load(m, c, c["detect_mask"])
    for iters, final in ((5, False), (7, True), (0, False), (0, True)):
        with pytest.raises(api.TsarError) as e:
            m.wmf(iters, final)
        assert e.value.code == api.TSAR_ERR_INVALID, (iters, final)
    m.wmf(4, False)
    found.mask(m, rec["detect_scale"], "sparse after the refusals, wmf(4, False):")
    _load(m, c)
    with pytest.raises(api.TsarError):
        m.wmf(7, True)
    m.wmf(6, True)
    found.fill_state(m, rec["fill"]["mask"][5], "sparse after the refusals, wmf(6, True):")
    m.close()
    assert not found, found

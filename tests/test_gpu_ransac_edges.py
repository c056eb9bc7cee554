"""tsar_ransac_regions against orc_ransac_regions where tests/test_gpu_parity.py::test_ransac_regions_bit_exact does not reach: regions
above the 50 000-point subsampling threshold (the branch every large weak region of a full-size view takes), regions with 0 to 3
reliable pixels, more region slots than the device has compute units to share out, textureless ids that are not contiguous and
include 0, reliability values other than exactly 1, and TSAR_FLAG_FIX_PLANE_FIT.  Label maps and masks are written by hand.

Every case: planes of all textureless regions and every inlier ratio bit for bit, twice in the same context (the second call takes
recycled, unzeroed arena memory), then fake_depth + fill_textureless against the oracle's fake_depth + update_scale + compute_disp.
NaN equals NaN whatever its sign (a region of one point has only degenerate hypotheses: 0 / 0; x86 produces the negative default
NaN, the GPU the positive one)."""
import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu

SEED = 12
_states, _fits = {}, {}


def _oracle(sc, **kw):
    return ol.Oracle([im.cpu().numpy() for im in sc.images], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, **kw)


def _state(w, h):
    """the scene and the oracle's PatchMatch state after init + 2 iterations, as _prepared_pair of test_gpu_parity.py builds it;
    computed once per size and shared"""
    if (w, h) not in _states:
        sc = synth.make_scene(w, h, 1, seed=7)
        orc = _oracle(sc, seed=SEED)
        orc.pm_init()
        orc.pm_iterate(2)
        _states[(w, h)] = (sc, orc.norm4.copy(), orc.c.copy())
    return _states[(w, h)]


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _reference(key, w, h, labels, text, size, mask, flags=0):
    """the oracle's fit and filled depth map for one case (cached under `key`: the launch-form parameters share it)"""
    if key not in _fits:
        sc, norm4, c = _state(w, h)
        orc = _oracle(sc, seed=SEED, flags=flags)
        orc.norm4[:] = norm4
        orc.c[:] = c
        orc.getview()
        orc.scale[:] = mask
        orc.set_regions(labels, text, size)
        planes, ratio = orc.ransac_regions()
        orc.fake_depth()
        orc.update_scale()
        _fits[key] = (planes, ratio, orc.compute_disp()[..., 3].copy())
    return _fits[key]


def _check(key, w, h, labels, text, size, mask, flags=0):
    sc, norm4, c = _state(w, h)
    planes_ref, ratio_ref, depth_ref = _reference(key, w, h, labels, text, size, mask, flags)
    m = api.matcher_from_scene(sc, seed=SEED, flags=flags | api.FLAG_STRICT_DIV)
    m.set_plane(norm4, c)
    m.getview()
    m.set_reliable_mask(mask)
    m.set_regions(labels, text, size)
    weak = text == -1.0
    for call in range(2):
        planes, ratio = m.ransac_regions()
        assert _same(planes[weak], planes_ref[weak]), (call, np.nonzero(~np.all((planes.view(np.uint32) == planes_ref.view(np.uint32)) | ~weak[:, None], axis=1))[0][:8])
        assert _same(ratio, ratio_ref), call
    m.fake_depth()
    m.fill_textureless()
    assert _same(m.get_result(("depth",))["depth"], depth_ref)
    m.close()
    return planes_ref, ratio_ref


# ---- the subsampling branch ---------------------------------------------------------------------------------------------------
SUB_W, SUB_H = 419, 311                  # 130 309 pixels, both sides odd


def _subsampling_case():
    """three textureless regions as column bands (so that the raster-order pixel list interleaves them and the stable sort by region
    has work to do) with exactly 50 000, 50 001 and 20 000 reliable pixels: at the threshold (kept whole), one above it (every point
    but one: 49 999 of 50 001, the `hi <= lo` skip fires twice) and below"""
    rng = np.random.default_rng(5)
    x = np.broadcast_to(np.arange(SUB_W), (SUB_H, SUB_W))
    labels = np.where(x < 165, 1, np.where(x < 330, 2, np.where(x < 400, 3, 0))).astype(np.int32)
    mask = np.zeros(SUB_W * SUB_H, np.float32)
    for rg, want in ((1, 50000), (2, 50001), (3, 20000)):
        mask[rng.choice(np.nonzero(labels.ravel() == rg)[0], want, replace=False)] = 1.0
    textured = np.nonzero(labels.ravel() == 0)[0]
    mask[textured[rng.uniform(size=textured.size) < 0.5]] = 1.0
    mask = mask.reshape(SUB_H, SUB_W)
    text = np.array([1.0, -1.0, -1.0, -1.0], np.float32)
    size = np.array([0.0, 310.0, 310.0, 310.0], np.float32)
    return labels, text, size, mask


@pytest.mark.parametrize("knob", [None, "TSAR_RANSAC_WGS", "TSAR_RANSAC_FORCE_FALLBACK"], ids=["default", "one_workgroup", "forced_fallback"])
def test_ransac_subsampling_threshold(monkeypatch, knob):
    if knob:
        monkeypatch.setenv(knob, "1")
    labels, text, size, mask = _subsampling_case()
    counts = [int(((labels == rg) & (mask == 1.0)).sum()) for rg in (1, 2, 3)]
    assert counts == [50000, 50001, 20000]
    planes, ratio = _check("sub", SUB_W, SUB_H, labels, text, size, mask)
    assert np.isfinite(planes[1:]).all() and (ratio[1:] > 0).all() and ratio[0] == 0


# ---- degenerate regions ---------------------------------------------------------------------------------------------------------
SMALL_W, SMALL_H = 101, 75


def _degenerate_case(any_reliable):
    """regions 1..5 with 0, 1, 2, 3 and 70 reliable pixels, region 6 an ordinary one, region 7 textureless without a single pixel;
    region 0 textured.  With the default 8 workgroups per region, a region of fewer than 8 points leaves workgroups an empty share."""
    rng = np.random.default_rng(9)
    labels = np.zeros((SMALL_H, SMALL_W), np.int32)
    for rg in range(1, 6):
        labels[10 * rg: 10 * rg + 9, 5:40] = rg
    labels[:, 50:] = 6
    mask = np.zeros(SMALL_W * SMALL_H, np.float32)
    if any_reliable:
        for rg, want in ((2, 1), (3, 2), (4, 3), (5, 70)):
            mask[rng.choice(np.nonzero(labels.ravel() == rg)[0], want, replace=False)] = 1.0
        big = np.nonzero(labels.ravel() == 6)[0]
        mask[big[rng.uniform(size=big.size) < 0.6]] = 1.0
    textured = np.nonzero(labels.ravel() == 0)[0]
    mask[textured[rng.uniform(size=textured.size) < 0.5]] = 1.0
    text = np.array([1.0] + [-1.0] * 7, np.float32)
    size = np.array([0, 34, 34, 34, 34, 34, 74, 10], np.float32)
    return labels, text, size, mask.reshape(SMALL_H, SMALL_W)


@pytest.mark.parametrize("knob", [None, "TSAR_RANSAC_WGS"], ids=["default", "one_workgroup"])
def test_ransac_degenerate_regions(monkeypatch, knob):
    if knob:
        monkeypatch.setenv(knob, "1")
    labels, text, size, mask = _degenerate_case(True)
    counts = [int(((labels == rg) & (mask == 1.0)).sum()) for rg in range(1, 8)]
    assert counts[:5] == [0, 1, 2, 3, 70] and counts[5] > 1000 and counts[6] == 0
    planes, ratio = _check("degenerate", SMALL_W, SMALL_H, labels, text, size, mask)
    for rg in (1, 7):                                            # no point: the initial plane, ratio 0
        assert np.array_equal(planes[rg], np.array([0, 0, 1, -1], np.float32)) and ratio[rg] == 0
    assert np.isnan(planes[2]).all() and ratio[2] == 0           # one point: every hypothesis is 0 / 0
    assert np.isfinite(planes[6]).all() and ratio[6] > 0


def test_ransac_no_reliable_pixel_in_any_textureless_region():
    """the selection comes back empty (the host's nsel == 0 path): every textureless region keeps the initial plane"""
    labels, text, size, mask = _degenerate_case(False)
    assert not ((labels > 0) & (mask == 1.0)).any() and (mask == 1.0).any()
    planes, ratio = _check("no reliable", SMALL_W, SMALL_H, labels, text, size, mask)
    assert (planes[1:] == np.array([0, 0, 1, -1], np.float32)).all() and (ratio == 0).all()


# ---- more slots than compute units to share out -----------------------------------------------------------------------------
def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _many_slots_case(nslot):
    """the 419 x 311 image tiled with 7 x 5 cells dealt out to 3 nslot - 2 regions in turn; every third id is textureless, 0 and
    the last among them; half the pixels reliable: 50-300 points per region for the slot counts used on a 256-CU device"""
    rng = np.random.default_rng(nslot)
    nreg = 3 * nslot - 2
    y, x = np.mgrid[0:SUB_H, 0:SUB_W]
    labels = (((y // 5) * ((SUB_W + 6) // 7) + x // 7) % nreg).astype(np.int32)
    text = np.where(np.arange(nreg) % 3 == 0, -1.0, 1.0).astype(np.float32)
    size = (20 + 10 * (np.arange(nreg) % 7)).astype(np.float32)
    mask = (rng.uniform(size=(SUB_H, SUB_W)) < 0.5).astype(np.float32)
    return labels, text, size, mask


@pytest.mark.parametrize("which", ["n_cu/3", "n_cu/2", "n_cu/2+1", "n_cu+1"], ids=["wgs3", "wgs2", "wgs1", "wgs0"])
def test_ransac_many_slots(which):
    """the host clamps the workgroups per region to n_cu / slots: 3, 2, then 1 and 0 (both the single-workgroup kernel)"""
    n_cu = _n_cu()
    nslot = {"n_cu/3": n_cu // 3, "n_cu/2": n_cu // 2, "n_cu/2+1": n_cu // 2 + 1, "n_cu+1": n_cu + 1}[which]
    assert n_cu // nslot == {"n_cu/3": 3, "n_cu/2": 2, "n_cu/2+1": 1, "n_cu+1": 0}[which]
    labels, text, size, mask = _many_slots_case(nslot)
    assert int((text == -1).sum()) == nslot and text[0] == -1 and text[-1] == -1
    pts = np.bincount(labels[mask == 1.0], minlength=len(text))[text == -1]
    if n_cu == 256:
        assert 50 <= pts.min() and pts.max() <= 300, (pts.min(), pts.max())
    planes, ratio = _check(("slots", nslot), SUB_W, SUB_H, labels, text, size, mask)
    assert (ratio[text == -1] > 0).all() and (ratio[text != -1] == 0).all()


# ---- reliability values ---------------------------------------------------------------------------------------------------------
def test_ransac_counts_only_mask_values_equal_to_one():
    rng = np.random.default_rng(3)
    labels = np.zeros((SMALL_H, SMALL_W), np.int32)
    labels[:, 30:65] = 1
    labels[:, 65:] = 2
    values = np.array([1.0, 0.5, 2.0, np.nan, -1.0, 0.0], np.float32)
    mask = values[rng.integers(0, len(values), size=(SMALL_H, SMALL_W))]
    text = np.array([1.0, -1.0, -1.0], np.float32)
    size = np.array([0, 74, 74], np.float32)
    for v in values[1:5]:
        assert ((mask == v) | (np.isnan(mask) & np.isnan(v)))[labels > 0].sum() > 100
    planes, ratio = _check("mask values", SMALL_W, SMALL_H, labels, text, size, mask)
    # the same fit as with every other value cleared: only == 1 counts
    planes1, ratio1 = _reference("mask values, ones only", SMALL_W, SMALL_H, labels, text, size, (mask == 1.0).astype(np.float32))[:2]
    assert _same(planes[1:], planes1[1:]) and _same(ratio, ratio1)


# ---- TSAR_FLAG_FIX_PLANE_FIT ------------------------------------------------------------------------------------------------------
def test_ransac_fix_plane_fit_flag():
    """the flag replaces calcLinePara's first component (main.cpp:159 writes y3 - y1 in both products) by the cross product's: other
    hypotheses, another plane — in the oracle by construction, on the GPU equal to the oracle's in both settings"""
    rng = np.random.default_rng(4)
    labels = np.zeros((SMALL_H, SMALL_W), np.int32)
    labels[:, 30:65] = 1
    labels[:, 65:] = 2
    mask = (rng.uniform(size=(SMALL_H, SMALL_W)) < 0.7).astype(np.float32)
    text = np.array([1.0, -1.0, -1.0], np.float32)
    size = np.array([0, 74, 74], np.float32)
    plain, _ = _check("plane fit, reference", SMALL_W, SMALL_H, labels, text, size, mask)
    fixed, _ = _check("plane fit, fixed", SMALL_W, SMALL_H, labels, text, size, mask, flags=api.FLAG_FIX_PLANE_FIT)
    assert not np.array_equal(plain[1], fixed[1]) and not np.array_equal(plain[2], fixed[2])

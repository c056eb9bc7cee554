"""The sweep's partial-window pruning (pm_tap_common.h prune_proven, pm_tap_r5.h PRUNE, pm_sweep_impl.h pruned_cost) on imagery chosen
to sit at the bound's rounding allowances and to walk the repeat path, where tests/test_gpu_prune.py has one natural scene.

Scenes (built like tests/test_gpu_edges.py::_scene): the reference camera at the origin, three source cameras that differ by pure
translations, uint8 images.  The truth is the fronto-parallel plane Z0 whose shift in the TRUE source is 2.5 pixels; that view is a
crop of the reference's base image two pixels along, so at the truth every sample is the mean of two texels, and the one exact match
(shift 2) lies just outside the depth range, whose shifts are 2.016 .. 10: every sample of every hypothesis is a bilinear blend, the
pixels creep towards the far end of the range and their costs towards 1.3e-4, the size of PM_PRUNE_SLACK, without reaching 0, so
lanes go on accepting in every iteration.  (With shifts of 2.12 .. 2.87 every wide hypothesis is a near match and some lane of a
wave nearly always accepts: no view is left once the true view comes first.  With shift 2 inside the range the costs reach 0 and
only the finest step ever repeats.  Measured: profiles/prune/README.md section 6.)  The two DECOY sources are independent images of
the same class: nothing in them matches anything.

    layout "decoys_first": [reference, decoy, decoy, true]   a wave leaves views 1 and 2, then meets a view below its cost: the
                                                             hypothesis is scored again in full (the repeat path), on which the
                                                             accepted cost's ratio = best[0] / best[1] and best view depend
    layout "true_first":   [reference, true, decoy, decoy]   a lane that has seen a cost below its own must never be proven

Image classes: texture (0..255), bright (246..255: the largest sums beside the smallest variances), gate (a slow ramp plus noise
0..5: windows on both sides of the variance gate), binary (3 x 3 blocks of 0 or 255: the largest variance, weights of ~1e-6 beside
weights of ~1), lonely (0..39 with 3 % of the pixels at 255: windows whose every weight is ~1e-6), banded (texture, but rows
y % 22 < 7 of the true source are independent noise, the phase moved per layout: for many pixels the first lines of the window are
unrelated and the rest matches, the case in which the bound is nearly an equality).  101 x 67: both extents odd, partial tiles on
every border; 192 x 128: interior waves take the clamp-free and ring walks.

Every run is a fresh context (the knobs are read once, by tsar_create): pm_init, then pm_iterate(4)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu

F, Z0, SHIFT = 100.0, 10.0, 2.5
DEPTH_MIN, DEPTH_MAX = 2.5, 12.4            # shifts of 10 .. 2.016 pixels in the true source: the exact match at 2 lies just outside
CLASSES = ("texture", "bright", "gate", "binary", "lonely", "banded")
LAYOUTS = ("decoys_first", "true_first")
SIZES = ((101, 67), (192, 128))
SEED = 7
ITERS = 4
PAD = 8

# every refinement step and every launch are checked: more than production checks
PRUNE_ALL = {"TSAR_PRUNE": "1", "TSAR_PRUNE_FROM": "0", "TSAR_COMPACT_FROM": "2", "TSAR_PRUNE_STEPS": "8"}
PRUNE_DEFAULT = {"TSAR_PRUNE": "1", "TSAR_PRUNE_FROM": "1", "TSAR_PRUNE_STEPS": "2"}


def _image(rng, cls, h, w):
    if cls in ("texture", "banded"):
        return rng.integers(0, 256, (h, w))
    if cls == "bright":
        return rng.integers(246, 256, (h, w))
    if cls == "gate":
        y, x = np.mgrid[0:h, 0:w]
        return np.floor(100.0 + 0.05 * x + 0.03 * y).astype(np.int64) + rng.integers(0, 6, (h, w))
    if cls == "binary":
        blocks = 255 * rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3))
        return np.kron(blocks, np.ones((3, 3), np.int64))[:h, :w]
    if cls == "lonely":
        return np.where(rng.random((h, w)) < 0.03, 255, rng.integers(0, 40, (h, w)))
    raise ValueError(cls)


_SCENES = {}


def _scene(cls, layout, size):
    """images (uint8), K, R, t of the four views"""
    key = (cls, layout, size)
    if key not in _SCENES:
        w, h = size
        rng = np.random.default_rng([41, CLASSES.index(cls), w])
        bh, bw = h + 2 * PAD, w + 2 * PAD
        base = _image(rng, cls, bh, bw)
        ref = base[PAD:PAD + h, PAD:PAD + w]
        true = base[PAD:PAD + h, PAD - 2:PAD - 2 + w].copy()            # true[y, u] = ref[y, u - 2]: u = x + 2.5 samples between ref x and x + 1
        if cls == "banded":
            rows = (np.arange(h) + 11 * LAYOUTS.index(layout)) % 22 < 7
            true[rows] = _image(rng, cls, h, w)[rows]
        decoys = [_image(rng, cls, bh, bw)[PAD:PAD + h, PAD:PAD + w] for _ in range(2)]
        tx = SHIFT * Z0 / F
        t_true, t_decoys = [tx, 0.0, 0.0], [[0.0, tx, 0.0], [-0.8 * tx, 0.4 * tx, 0.0]]
        if layout == "decoys_first":
            imgs, t = [ref] + decoys + [true], [[0.0, 0.0, 0.0]] + t_decoys + [t_true]
        else:
            imgs, t = [ref, true] + decoys, [[0.0, 0.0, 0.0], t_true] + t_decoys
        imgs = [np.ascontiguousarray(im).astype(np.uint8) for im in imgs]
        K = np.tile(np.array([[F, 0, w / 2], [0, F, h / 2], [0, 0, 1]], np.float32), (4, 1, 1))
        R = np.tile(np.eye(3, dtype=np.float32), (4, 1, 1))
        _SCENES[key] = (imgs, K, R, np.array(t, np.float32))
    return _SCENES[key]


def test_the_scenes_are_what_the_header_says():
    for layout in LAYOUTS:
        true_at = 3 if layout == "decoys_first" else 1
        for cls in CLASSES:
            imgs, K, R, t = _scene(cls, layout, SIZES[0])
            assert all(im.dtype == np.uint8 and im.shape == (67, 101) for im in imgs)
            same = imgs[true_at][:, 2:] == imgs[0][:, :-2]
            assert same.all() if cls != "banded" else 0.6 < same.all(axis=1).mean() < 0.75
            assert F * t[true_at, 0] / Z0 == SHIFT
            for v in range(1, 4):
                if v != true_at:
                    assert (imgs[v][:, 2:] == imgs[0][:, :-2]).mean() < (0.6 if cls == "binary" else 0.25)
    lo = _scene("bright", LAYOUTS[0], SIZES[0])[0]
    assert min(im.min() for im in lo) >= 246
    assert set(np.unique(_scene("binary", LAYOUTS[0], SIZES[0])[0][0])) == {0, 255}
    lonely = _scene("lonely", LAYOUTS[0], SIZES[1])[0][0]
    assert 0.02 < (lonely == 255).mean() < 0.04 and lonely[lonely < 255].max() == 39
    a, b = _scene("banded", LAYOUTS[0], SIZES[0])[0][3], _scene("banded", LAYOUTS[1], SIZES[0])[0][1]
    assert (a != b).any(axis=1).sum() >= 2 * 7 * (67 // 22)                   # the band's phase differs between the layouts


def _matcher(scene, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:                                        # (the knobs are read once, when the context is created)
        m = api.Matcher()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    imgs, K, R, t = scene
    m.set_params(api.default_params(box_hsize=11, box_vsize=11, n_best=1, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, flags=0, seed=SEED))
    m.set_views(imgs, K, R, t, u8=True)
    return m


NAMES = ("planes", "cost", "best view", "ratio", "depth", "normal", "cost map")


def _run(scene, env, iters=ITERS, maps=True):
    m = _matcher(scene, env)
    m.enable_kernel_timing(True)
    m.pm_init()
    m.pm_iterate(iters)
    out = list(m.get_plane())                   # planes, cost, best view, ratio
    if maps:
        m.compute_disp()
        res = m.get_result(("depth", "normal", "cost"))
        out += [res[k] for k in ("depth", "normal", "cost")]
    t = m.kernel_timing()
    m.close()
    return out, t


def _differing(a, b):
    """per array: how many 32-bit patterns differ (and where the first one is)"""
    out = {}
    for name, u, v in zip(NAMES, a, b):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape and u.dtype.itemsize == 4, name
        d = u.view(np.uint32) != v.view(np.uint32)
        if d.any():
            out[name] = (int(d.sum()), tuple(int(i) for i in np.argwhere(d)[0]))
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls", CLASSES)
def test_pruned_run_is_the_unpruned_run_bit_for_bit(cls, layout, size):
    scene = _scene(cls, layout, size)
    base = {}
    for block in ("128", "256", None):
        env = {"TSAR_PRUNE": "0", "TSAR_COMPACT_FROM": "2"} if block else {"TSAR_PRUNE": "0"}
        if block:
            env["TSAR_BLOCK"] = block
        base[block], t = _run(scene, env)
        assert "pm_sweep_prune" not in t and "pm_sweep_packed" in t, (block, t)
    assert (base[None][1] < 2.0).mean() > 0.5                                 # the run scored something
    failures = {}
    for block in ("128", "256"):
        for ring in ("0", "1"):
            got, t = _run(scene, dict(PRUNE_ALL, TSAR_BLOCK=block, TSAR_RING=ring))
            assert t["pm_sweep_prune"][0] == 2 * ITERS and "pm_sweep_packed" in t, t
            assert ("pm_sweep_ring" in t) == (ring == "1"), t
            d = _differing(got, base[block])
            if d:
                failures["block %s ring %s" % (block, ring)] = d
    got, t = _run(scene, PRUNE_DEFAULT)
    assert t["pm_sweep_prune"][0] == 2 * ITERS - 1 and "pm_sweep_packed" in t, t
    d = _differing(got, base[None])
    if d:
        failures["defaults"] = d
    assert not failures, failures


# ---- the unpruned kernels on these images against the CPU oracle ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def rcp_table():
    m = api.Matcher()
    table = ol.rcp_table_from_device(m)
    m.close()
    return table


@pytest.mark.parametrize("cls", CLASSES)
def test_unpruned_kernels_equal_the_oracle_on_these_images(cls, rcp_table):
    """bright and binary stress ncc_cost's claim that var_ref * var_src stays inside sqrt_rsq_exact's range (var >= 1e-5 each, so the
    product may be 1e-10, and up to 127.5^4) on imagery no parity test has"""
    imgs, K, R, t = scene = _scene(cls, "decoys_first", SIZES[0])
    got, _ = _run(scene, {"TSAR_PRUNE": "0"}, iters=2, maps=False)
    orc = ol.Oracle([im.astype(np.float32) for im in imgs], K, R, t, DEPTH_MIN, DEPTH_MAX, box=11, n_best=1, seed=SEED, flags=ol.FLAGS_FAST_8BIT_IMAGERY)
    orc.set_rcp_table(rcp_table)
    orc.pm_init()
    orc.pm_iterate(2)
    assert not orc.rcp_out_of_range
    d = _differing(got, (orc.norm4, orc.c, orc.beview, orc.ratio))
    assert not d, d
    assert (orc.c < 2.0).mean() > 0.5


# ---- the checks did something ----------------------------------------------------------------------------------------------------------

def _census(cls, layout, size):
    """[step][hypotheses checked, views checked, views left, repeats] of the fifth iteration of a run that checks every step"""
    m = _matcher(_scene(cls, layout, size), dict(PRUNE_ALL, TSAR_BLOCK="256", TSAR_RING="1"))
    m.pm_init()
    m.pm_iterate(ITERS)
    m.selftest_prune_census(True)
    m.pm_iterate(1)
    k = m.selftest_prune_census(False)
    m.close()
    return k


# Classes whose fifth iteration leaves views in both layouts at both sizes (measured on an MI355X: profiles/prune/README.md section 6)
LEAVES_VIEWS = ("texture", "lonely", "banded")
# ... and those that leave none in any case, and why.  (With the three allowances at 0 the bright and gate scenes do leave views, and
# their pruned runs differ from the unpruned ones: these are the classes in which the allowances carry the proof.)
LEAVES_NONE = {
    "bright": "var_ref is 5 to 12 and e = 0.9 takes most of the margin: one lane in ten is proven against an unrelated view "
              "(tests/test_prune_bound_adversarial_cpu.py), a whole wave of 64 never",
    "gate": "the noise 0..5 has variance 2.9; a bilinear blend of it and the W_A / W of a partial window bring vs below 2 e = 1.8 in "
            "nearly every lane, and var_ref - e is below it in four lanes of ten: the variance gate stops the wave",
    "binary": "the texels of the other value weigh exp(-255 / 18): var_ref is ~0.05 in every window, far below the variance gate",
}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls", CLASSES)
def test_the_checks_leave_views_and_repeat(cls, layout, size):
    k = _census(cls, layout, size)
    print("prune census %s %s %dx%d, iteration 5: [step][checked, views, views left, repeats] =" % ((cls, layout) + size), k.tolist())
    steps = int((k[:, 0] > 0).sum())
    assert steps >= 2 and (k[:steps, 0] > 0).all() and k[steps:].sum() == 0   # every refinement step was checked
    assert (k[:, 1] == 3 * k[:, 0]).all()                                      # three views per hypothesis
    assert (k[:, 2] <= k[:, 1]).all() and (k[:, 3] <= k[:, 0]).all()           # at most every view left, at most one repeat per hypothesis
    if cls == "texture":
        assert k[0, 2] > 0, "no (wave, view) pair was left early at step 0"
    if cls in ("texture", "banded") and layout == "decoys_first":
        assert k[:, 3].sum() > 0, "no hypothesis was scored again: the repeat path never ran"
    if cls in LEAVES_VIEWS:
        assert k[:, 2].sum() > 0
    else:
        print("   no view left is expected:", LEAVES_NONE[cls])
    if cls == "binary":                                                        # the gate shuts every lane out: the CPU set predicts exactly 0
        assert k[:, 2].sum() == 0 and k[:, 3].sum() == 0, LEAVES_NONE[cls]


def test_unrelated_views_are_left_by_nearly_every_wave():
    """The power of the kernel's check, which no equality of states can see: a check that errs on the safe side (say, reference sums
    of one line fewer than the view's sums) changes no value and leaves no view.  The texture scene's converged planes, every pixel's
    cost set to 0.02, the two decoys as the only views, one iteration: every checked hypothesis meets unrelated samples in both views
    and nothing can be accepted.  The CPU restatement proves 99.95 % of such lanes by the last check (uniform / random in
    tests/test_prune_bound_adversarial_cpu.py), so 0.9995^64 = 97 % of the (wave, view) pairs of whole interior waves are left; border
    waves (a 32 x 4 strip whose windows reach past the image: clamped windows, replicated texels) are 42 % of the 6 x 32 strips at
    192 x 128, so even with none of them the share is 0.97 * 0.58 = 0.56, above one half."""
    scene = _scene("texture", "decoys_first", SIZES[1])
    env = dict(PRUNE_ALL, TSAR_BLOCK="256", TSAR_RING="1")
    m = _matcher(scene, env)
    m.pm_init()
    m.pm_iterate(ITERS)
    planes = m.get_plane()[0]
    m.close()
    m = _matcher(scene, env)
    m.set_view_subset([1, 2])
    m.pm_init()
    m.set_plane(planes, np.full(planes.shape[:2], 0.02, np.float32))
    m.selftest_prune_census(True)
    m.pm_iterate(1)
    k = m.selftest_prune_census(False)
    cost = m.get_plane()[1]
    m.close()
    print("prune census, unrelated views only, cost_now 0.02: [step][checked, views, views left, repeats] =", k[:4].tolist())
    steps = int((k[:, 0] > 0).sum())
    assert steps >= 2 and (k[:steps, 1] == 2 * k[:steps, 0]).all()
    assert (cost == np.float32(0.02)).all() and k[:, 3].sum() == 0            # nothing was accepted, nothing repeated
    assert (k[:steps, 2] > 0.5 * k[:steps, 1]).all(), (k[:steps, 2] / k[:steps, 1]).tolist()

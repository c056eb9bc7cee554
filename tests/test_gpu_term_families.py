"""Every tap-loop family with the geometric-consistency term and the plane prior installed (variant bit 24, TSAR_V_GEOM), against the CPU
oracle with set_geom + set_plane_prior, bit for bit.

The bit doubles every PatchMatch kernel (tests/test_kernel_configs.py counts 39 tap-loop configurations, each with and without it), and
phase 2 of `tsar_gipuma --all --geom_consistency` runs only the instantiations that carry it; the other GPU tests that install maps or a
prior reach the box-11 loop and the general-window loop at chunk 5 / 6 with two or four best views, on 8-bit imagery under best-N.  One
test body; a row installs the ground-truth maps (one source view without a map, a hole in the others) and the prior (ground truth x
1.01, a hole, one NaN normal) and checks
  - pm_cost_planes on the ground-truth planes and on pm_init's planes,
  - the state after pm_init,
  - the state after pm_iterate(3) in one call with TSAR_COMPACT_FROM=2 (six launches: global-load, buffer-load and packed forms), or
    for the final-mode rows pm_iterate(1), pm_iterate_final(2, text), pm_iterate(1),
that kernel_timing() shows pm_sweep_geom and no pm_sweep, and that the row is not vacuous (with the terms cleared the same planes score
differently at more than half of the pixels, and the final state is not the photometric run's).
Strict mode runs against the strict oracle.  Fast mode runs against the oracle flags the row's photometric twin uses in
tests/test_gpu_fast_exact.py: FLAGS_FAST_8BIT_IMAGERY for the 8-bit production loops, FLAG_FAST_ARITH (column order) for float imagery
and TSAR_VARIANT=122.  A row without a fast photometric twin in the suite (fast = "composition") is held in fast mode to a composition
for pm_cost_planes only: the per-view photometric costs from the device itself (set_view_subset([v]), terms cleared), combined by
test_geom_cpu.expected_cost_planes plus test_plane_prior_cpu.add_plane_prior; its whole-call leg is strict only.
Beside each row: the TapConfig<NB, HR, STRICT, QUAD, V> pm_dispatch.h chooses for it (S = the mode; LUT_V(ch) = the general-window
loop in chunks of ch taps, ch = lut_chunk_taps(taps per line), a line being a window row in fast mode and a column in strict mode)."""
import numpy as np
import pytest

import oracle_lib as ol
from test_geom_cpu import expected_cost_planes
from test_gpu_call_parity import _assert_same, _state
from test_plane_prior_cpu import add_plane_prior
from test_plane_prior_oracle_cpu import held_prior
from tsar_mvs_amd import api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
FAST8, FASTF = ol.FLAGS_FAST_8BIT_IMAGERY, ol.FLAG_FAST_ARITH
QUIRKS = api.FLAG_FIX_DOWN_FAR_SEED | api.FLAG_FIX_RIGHT_FAR_CMP
WEIGHT, CLIP = 0.2, 3.0


def row(box=11, n_best=1, comb=api.COMB_BEST_N, six=False, flags=0, u8=True, env=None, subset=None, fast=FAST8, final=False, modes=("strict", "fast"),
        per_view_env=None):
    box = box if isinstance(box, tuple) else (box, box)
    return dict(box=box, n_best=n_best, comb=comb, six=six, flags=flags, u8=u8, env=env or {}, subset=subset, fast=fast, final=final, modes=modes,
                per_view_env=per_view_env or {})


ROWS = {
    # control: the geometric leg of this one already passes elsewhere
    "control": row(),                                                          # TapConfig<2, 5, false, true, 250> / <2, 5, true, true, 122>
    # selection width
    "box11_nbest4": row(n_best=4),                                             # <4, 0, S, true, LUT_V(6)>; the sweeps: the box-11 four-best loop <4, 5, S, true, 250 / 122>
    "box11_nbest5_six": row(n_best=5, six=True),                               # <32, 0, S, true, LUT_V(6)>
    "box11_all_three": row(comb=api.COMB_ALL, subset=[1, 2, 3]),               # <4, 0, S, true, LUT_V(6)>
    "box11_all_six": row(comb=api.COMB_ALL, six=True),                         # <32, 0, S, true, LUT_V(6)>
    "box11_angle_six": row(comb=api.COMB_ANGLE, six=True),                     # <32, 0, S, true, LUT_V(6)>
    "box9_nbest4_all": row(box=9, n_best=4, comb=api.COMB_ALL),                # <4, 0, S, true, LUT_V(5)>: 5 taps per line
    # general-window chunk lengths: every (selection width) x (chunk) pair
    "box7": row(box=7),                                                        # <2, 0, S, true, LUT_V(4)>: 4 taps per line
    "box7_nbest3": row(box=7, n_best=3),                                       # <4, 0, S, true, LUT_V(4)>
    "box15_nbest2": row(box=15, n_best=2),                                     # <2, 0, S, true, LUT_V(4)>: 8 taps per line
    "box15_nbest5_six": row(box=15, n_best=5, six=True),                       # <32, 0, S, true, LUT_V(4)>
    "box19_nbest2": row(box=19, n_best=2),                                     # <2, 0, S, true, LUT_V(5)>: 10 taps per line
    "box19_all_six": row(box=19, comb=api.COMB_ALL, six=True),                 # <32, 0, S, true, LUT_V(5)>
    "box17_nbest3": row(box=17, n_best=3),                                     # <4, 0, S, true, LUT_V(5)>: 9 taps per line
    # an even box: the sweeps' window is (box - 1) / 2 = 5, box 11's; pm_init alone takes box / 2 = 6 (7 taps per line) unless FIX_INIT_RADIUS
    "box12": row(box=12),                                                      # init <2, 0, S, true, LUT_V(4)>; everything else the control's kernels
    "box12_fix_init_radius": row(box=12, flags=api.FLAG_FIX_INIT_RADIUS),      # the control's kernels throughout
    "box12_nbest3": row(box=12, n_best=3),                                     # init <4, 0, S, true, LUT_V(4)>, cost_planes <4, 0, S, true, LUT_V(6)>, sweeps <4, 5, S, true, 250 / 122>
    "rect_7x13": row(box=(7, 13)),                                             # <2, 0, false, true, LUT_V(4)> (rows of 4) / strict LUT_V(4) (columns of 7)
    "rect_19x5": row(box=(19, 5), n_best=2),                                   # <2, 0, false, true, LUT_V(5)> (rows of 10) / strict LUT_V(4) (columns of 3)
    "box11_tex_filter_8bit": row(flags=api.FLAG_TEX_FILTER_8BIT),              # <2, 0, S, true, LUT_V(6)>
    "box11_tex_filter_8bit_nbest3": row(n_best=3, flags=api.FLAG_TEX_FILTER_8BIT),   # <4, 0, S, true, LUT_V(6)>, the sweeps too
    "box11_lut2": row(env={"TSAR_LUT": "2"}, fast="composition"),              # <2, 0, S, true, LUT_V(6)>
    # float imagery: the one-tap loop without quad textures
    "float_box11": row(u8=False, fast=FASTF),                                  # <2, 5, S, false, 0>
    "float_box7": row(box=7, u8=False, fast=FASTF),                            # <2, 0, S, false, 0>
    "float_box11_nbest3": row(n_best=3, u8=False, fast=FASTF),                 # <32, 5, S, false, 0>
    "float_box9_nbest5_six": row(box=9, n_best=5, six=True, u8=False, fast=FASTF),   # <32, 0, S, false, 0>
    # 8-bit imagery through the one-tap loop
    "lut0_box7": row(box=7, env={"TSAR_LUT": "0"}, fast="composition"),        # <2, 0, S, true, 0>
    # (the composition's per-view scores must come from the row's own tap loop: a single selected view at box 11 would take the box-11
    # loop <2, 5, false, true, 250>, whose fast arithmetic walks rows; TSAR_VARIANT=0 keeps the per-view context on <2, 5, false, true, 0>)
    "lut0_box11_nbest5_six": row(n_best=5, six=True, env={"TSAR_LUT": "0"}, fast="composition", per_view_env={"TSAR_VARIANT": "0"}),   # <32, 5, S, true, 0>
    "lut0_box7_nbest5_six": row(box=7, n_best=5, six=True, env={"TSAR_LUT": "0"}, fast="composition"),   # <32, 0, S, true, 0>
    "variant0_box11": row(env={"TSAR_VARIANT": "0"}, fast="composition"),      # <2, 5, S, true, 0>
    # the fallback forms of the box-11 loop
    "variant122_fast": row(env={"TSAR_VARIANT": "122"}, fast=FASTF, modes=("fast",)),   # <2, 5, false, true, 122>
    "variant114": row(env={"TSAR_VARIANT": "114"}, fast="composition"),        # <2, 5, S, true, 114>
    # flags
    "fix_propagation_quirks": row(flags=QUIRKS),                               # the control's kernels
    # view selection
    "subset_3_1": row(n_best=2, subset=[3, 1]),                                # the control's kernels; view 2 unselected with a map, view 3 none
    # (in [3, 1] the only selected view with a map, view 1, also stands at position 1 of the selection, so indexing geom_back by the
    # position passes that row; here views 4 and 1 stand at positions 1 and 2 and view 2, at position 0, has no map)
    "subset_2_4_1": row(n_best=2, subset=[2, 4, 1]),                           # the control's kernels (two of three views enter the cost)
    "single_view": row(subset=[2]),                                            # the control's kernels; ratio = 0
    # final mode
    "final_box11": row(final=True),                                            # the control's kernels
    "final_box15": row(box=15, final=True),                                    # <2, 0, S, true, LUT_V(4)>
}
CASES = [(name, mode) for name, r in ROWS.items() for mode in r["modes"]]


@pytest.fixture(scope="module")
def rcp_table():
    m = api.Matcher()
    t = ol.rcp_table_from_device(m)
    m.close()
    return t


_scenes = {}


def _scene(six):
    """101 x 67 with four sources, 96 x 64 with six: whole and partial 32 x 8 and 32 x 16 tiles, room for a 19-wide window"""
    if six not in _scenes:
        _scenes[six] = synth.make_scene(96, 64, 6, seed=91, all_gt=True) if six else synth.make_scene(101, 67, 4, seed=92, all_gt=True)
    return _scenes[six]


def _maps(sc, none_view):
    """every source view's ground-truth depth with a hole of 0; none_view has no map"""
    maps = [g[0].numpy().astype(F32).copy() for g in sc.meta["gt_all"]]
    h, w = maps[0].shape
    for v in range(1, len(maps)):
        maps[v][h // 3:h // 3 + 12, w // 4:w // 4 + 16] = 0
    maps[0] = None
    maps[none_view] = None
    return maps


def _prior(sc):
    depth = (sc.gt_depth.numpy().astype(np.float64) * 1.01).astype(F32)
    normal_world = (sc.gt_normal.numpy().astype(np.float64) @ np.asarray(sc.R[0], np.float64)).astype(F32)
    h, w = depth.shape
    depth[h // 2:h // 2 + 12, w // 2:w // 2 + 16] = 0
    normal_world[5, 7] = np.nan
    return depth, normal_world


def _text(sc):
    rng = np.random.default_rng(8)
    text = rng.choice(np.array([-1.0, 0.0, 1.0], F32), size=(sc.h, sc.w))
    text[:, : sc.w // 4] = -1.0
    return text


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_cost(got, want, what):
    """(cost, best view, ratio) of pm_cost_planes as uint32"""
    for label, a, b in zip(("cost", "best view", "ratio"), got, want):
        bad = _bits(a) != _bits(b)
        assert not bad.any(), f"{what}: {label} differs at {int(bad.sum())} pixels, first {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("name,mode", CASES)
def test_family_with_both_terms(monkeypatch, rcp_table, name, mode):
    r = ROWS[name]
    strict = mode == "strict"
    composed = not strict and r["fast"] == "composition"
    monkeypatch.setenv("TSAR_COMPACT_FROM", "2")
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    sc = _scene(r["six"])
    n_views = len(sc.images)
    imgs = [im.numpy().astype(np.uint8) for im in sc.images] if r["u8"] else [(im + 0.25).numpy() for im in sc.images]
    sel = r["subset"] if r["subset"] is not None else list(range(1, n_views))
    # the view without a map: the last one; under a subset the first selected one (3 of [3, 1]), or an unselected one if only one is
    none_view = n_views - 1 if r["subset"] is None else sel[0] if len(sel) > 1 else 1
    maps = _maps(sc, none_view)
    prior = _prior(sc)
    (bh, bv_), seed = r["box"], 37

    def matcher(extra_env=None):
        with monkeypatch.context() as mp:                               # (the knobs are read once, when the context is created)
            for k, v in (extra_env or {}).items():
                mp.setenv(k, v)
            mm = api.Matcher()
        mm.set_params(api.default_params(box_hsize=bh, box_vsize=bv_, n_best=r["n_best"], cost_comb=r["comb"], depth_min=sc.depth_min,
                                         depth_max=sc.depth_max, flags=r["flags"] | (api.FLAG_STRICT_DIV if strict else 0), seed=seed))
        mm.set_views(imgs, sc.K, sc.R, sc.t, u8=r["u8"])
        if r["subset"] is not None:
            mm.set_view_subset(sel)
        return mm

    m = matcher()
    m.enable_kernel_timing(True)

    def install():
        m.set_geom_depths(maps, weight=WEIGHT, clip=CLIP)
        m.set_plane_prior(*prior)

    install()
    mats = [None] + [m.get_geom_matrices(v) for v in range(1, n_views)]
    held = m.get_plane_prior()
    q = m.plane_prior_params
    params = (F32(q.weight_depth), F32(q.weight_normal), F32(q.depth_clip), F32(q.normal_clip))

    def oracle(terms):
        o = ol.Oracle([np.asarray(i, F32) for i in imgs], sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=bh, box_v=bv_, n_best=r["n_best"],
                      cost_comb=r["comb"], seed=seed, subset=sel, flags=r["flags"] | (0 if strict or composed else r["fast"]))
        if not strict and not composed:
            o.set_rcp_table(rcp_table)
        if terms:
            o.set_geom(maps, mats, weight=WEIGHT, clip=CLIP)
            o.set_plane_prior(held, params)
        return o

    orc = oracle(True)
    assert np.array_equal(_bits(held), _bits(held_prior(orc, *prior)))
    gt = np.ascontiguousarray(synth.gt_planes(sc).numpy())
    with_terms = m.pm_cost_planes(gt)

    if composed:
        # pm_init's planes do not depend on the arithmetic: the strict oracle draws them
        orc.pm_init()
        drawn = orc.norm4.copy()
        m.pm_init()
        assert np.array_equal(_bits(m.get_plane()[0]), _bits(drawn))
        scored = {"gt": (gt, with_terms), "init": (drawn, m.pm_cost_planes(drawn))}
        m.clear_geom()
        m.clear_plane_prior()
        plain = m.pm_cost_planes(gt)
        pv = matcher(r["per_view_env"]) if r["per_view_env"] else m
        for what, (planes, got) in scored.items():
            per_view = {}
            for v in sel:
                pv.set_view_subset([v])
                per_view[v] = pv.pm_cost_planes(planes)[0]
            pv.set_view_subset(sel)
            c, bv, rt = expected_cost_planes(orc, mats, maps, planes, r["n_best"], WEIGHT, CLIP, cost_comb=r["comb"], views=sel, photometric=per_view)
            c = add_plane_prior(c, bv, held, planes, orc.depth_from_planes(planes), params)
            _same_cost(got, (c, bv, rt), f"{name} {mode} composition on {what} planes")
        if pv is not m:
            pv.close()
        m.close()
        assert (_bits(plain[0]) != _bits(with_terms[0])).mean() > 0.5
        return

    _same_cost(with_terms, orc.pm_cost_planes(gt), f"{name} {mode} pm_cost_planes on ground-truth planes")
    orc.pm_init()
    m.pm_init()
    _assert_same(m.get_plane(), _state(orc), f"{name} {mode} after pm_init")
    drawn = orc.norm4.copy()
    _same_cost(m.pm_cost_planes(drawn), orc.pm_cost_planes(drawn), f"{name} {mode} pm_cost_planes on pm_init's planes")
    photometric = oracle(False)
    photometric.pm_init()
    if r["final"]:
        text = _text(sc)
        m.pm_iterate(1)
        m.pm_iterate_final(2, text)
        for o in (orc, photometric):
            o.pm_iterate(1)
            o.pm_iterate_final(2, text)
        _assert_same(m.get_plane(), _state(orc), f"{name} {mode} after pm_iterate_final(2)")
        m.pm_iterate(1)
        orc.pm_iterate(1)
        photometric.pm_iterate(1)
        got, want = m.get_plane(), _state(orc)
        _assert_same(got[:2], want[:2], f"{name} {mode} an ordinary iteration after final mode")
    else:
        m.pm_iterate(3)                                                # one call, six launches, the last four packed where there is such a form
        orc.pm_iterate(3)
        photometric.pm_iterate(3)
        _assert_same(m.get_plane(), _state(orc), f"{name} {mode} after pm_iterate(3)")
    assert not orc.rcp_out_of_range
    t = m.kernel_timing()
    assert "pm_sweep_geom" in t and "pm_sweep" not in t, sorted(t)
    # not vacuous
    m.clear_geom()
    m.clear_plane_prior()
    plain = m.pm_cost_planes(gt)
    m.close()
    assert (_bits(plain[0]) != _bits(with_terms[0])).mean() > 0.5
    assert (_bits(orc.norm4) != _bits(photometric.norm4)).any(-1).mean() > 0.25     # (final mode freezes a quarter of the image)
    if len(sel) == 1:
        assert not orc.ratio.any()                                     # ratio = num >= 2 ? ... : 0

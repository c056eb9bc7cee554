"""Every phase of tsar_gipuma --all on the CPU: the tool is compiled against tests/cli_stub/tsar_stub.cpp, a stand-in for the C ABI that
opens no device, records every call with its scalar arguments and returns fixed maps.  What is pinned here is the host tool's own
behaviour: per view, the sequence of library calls; every line it prints; the records it writes; which views a rerun skips; what an
error releases.  The expected call sequences below are also the shortest description of what each phase does.

The tool is built from TSAR_GIPUMA_SRC (default host/tsar_gipuma.cpp; a file beside it, so that its includes resolve) with
TSAR_GIPUMA_CXXFLAGS (default -O0), so the same assertions can be held against another revision of the source, or against a build with
a host sanitizer."""
import os
import re
import shlex
import shutil
import subprocess
import time

import numpy as np
import pytest

from tsar_mvs_amd import io as tio
from tsar_mvs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.environ.get("TSAR_GIPUMA_SRC", os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_gipuma.cpp"))
CXXFLAGS = shlex.split(os.environ.get("TSAR_GIPUMA_CXXFLAGS", "-O0"))
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub.cpp")
W, H, NP = 64, 48, 64 * 48
VIEWS = range(3)
KEPT = np.arange(NP) % 3 != 0                         # the pixels the stub's tsar_geom_check keeps
STUB_DEPTH = (1.0 + (np.arange(NP) % 97) * 0.03125).astype(np.float32).reshape(H, W)      # the stub's tsar_get_result


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """the stub library and a tsar_gipuma linked against it"""
    d = str(tmp_path_factory.mktemp("cli_stub"))
    for cmd in (["g++", *CXXFLAGS, "-std=c++17", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", STUB],
                ["g++", *CXXFLAGS, "-std=c++17", "-pthread", "-o", d + "/tsar_gipuma", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_gipuma"


@pytest.fixture(scope="module")
def scene_template(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scene")) + "/"
    tio.export_scene(synth.make_scene(W, H, 2, seed=2), root)
    return root


@pytest.fixture
def scene(scene_template, tmp_path):
    root = str(tmp_path) + "/s/"
    shutil.copytree(scene_template, root)
    return root


class Run:
    def __init__(self, tool, root, *args, env=None, all_views=True):
        trace = root + "trace.txt"
        if os.path.exists(trace):
            os.remove(trace)
        cmd = [tool, *(["--all", "--gpus=1"] if all_views else []), "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=1",
               "--blocksize=11", "--n_best=1", *args]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, TSAR_STUB_TRACE=trace, **(env or {})))
        self.rc, self.stderr = out.returncode, out.stderr
        self.stdout = re.sub(r"\(\d+\.\d\d s\)", "(T s)", out.stdout)                    # the only figures that vary
        lines = open(trace).read().splitlines() if os.path.exists(trace) else []
        # page-locked buffers are sized on helper threads (their place in the trace varies) and the defaults take no argument
        self.calls = [ln for ln in lines if not ln.startswith(("tsar_host_", "tsar_default_"))]
        self.pinned = [ln for ln in lines if ln.startswith("tsar_host_")]


def rec(root, v, name):
    return open(root + f"APD/{v:08d}/{name}", "rb").read()


# ---- the expected calls, written out ------------------------------------------------------------------------------------------------
PARAMS = "box=11x11 n_best=1 cost_comb=1 depth_min=3.18134356 depth_max=9.15442753 cam_scale=1 flags=0"
UPLOAD = ["tsar_device_alloc device=0 bytes=3072", "tsar_device_write device=0 dst=set host_src=set bytes=3072"]   # one image, once per GPU
RELEASE_IMAGES = ["tsar_device_free device=0 p=set"] * 3
GET_RESULT = "tsar_get_result ctx={c} depth=set normal_world=set cost=null confid=null mem=0"


def fmt(lines, **kw):
    return [ln.format(**kw) for ln in lines]


def start(c, v, n=3, mem=1):
    """every view of every phase starts like this: its parameters (the seed is the run's plus the view id), then its images"""
    return [f"tsar_set_params ctx={c} {PARAMS} seed={v}", f"tsar_set_views_u8 ctx={c} n_views={n} w=64 h=48 gray=set mem={mem} cams=set"]


PHASE1 = ["tsar_pm_init ctx={c}", "tsar_pm_iterate ctx={c} iters=1", "tsar_compute_disp ctx={c}", GET_RESULT]
PHASE1_MULTI_SCALE = ["tsar_pyramid_views coarse={k} fine={c}",
                      "tsar_pm_init ctx={k}", "tsar_pm_iterate ctx={k} iters=3",
                      "tsar_upsample_planes fine={c} coarse={k}", "tsar_pm_iterate ctx={c} iters=1",
                      "tsar_compute_disp ctx={c}", GET_RESULT]
GEOM = ["tsar_load_planes ctx={c} depth=set normal_world=set mem=0",
        "tsar_set_geom_depths ctx={c} n_views=3 depth=null,set,set mem=0 weight=0.200000003 clip=3",
        "tsar_pm_rescore ctx={c}", "tsar_pm_iterate ctx={c} iters=2",
        "tsar_compute_disp ctx={c}", GET_RESULT,
        "tsar_clear_geom ctx={c}", "tsar_clear_plane_prior ctx={c}"]
SET_PRIOR = "tsar_set_plane_prior ctx={c} depth=set normal_world=set mem=0 weight_depth=0.100000001 weight_normal=0.0500000007 depth_clip=0.0199999996 normal_clip=0.133974597"
# every switch of phase 2: the coarse level's views before any term; the term, then the prior, then the sources' maps rendered and merged
# (which rescores: no tsar_pm_rescore); only then the term and the planes go down the chain
GEOM_EVERY_SWITCH_HEAD = ["tsar_clear_geom ctx={k}", "tsar_pyramid_views coarse={k} fine={c}",
                          "tsar_load_planes ctx={c} depth=set normal_world=set mem=0",
                          "tsar_set_geom_depths ctx={c} n_views=3 depth=null,set,set mem=0 weight=0.200000003 clip=3"]
GEOM_EVERY_SWITCH_TAIL = ["tsar_device_alloc device=0 bytes=12288",
                          "tsar_geom_reproject ctx={c} depth_diff=0.00999999978 min_views=1 depth_out=set count_out=null mem=1",
                          "tsar_pm_merge_depths ctx={c} depth=set mem=1 n_taken_out=null",
                          "tsar_device_free device=0 p=set",
                          "tsar_geom_pyramid coarse={k} fine={c}", "tsar_pyramid_planes coarse={k} fine={c}",
                          "tsar_pm_iterate ctx={k} iters=3",
                          "tsar_upsample_merge fine={c} coarse={k}", "tsar_pm_iterate ctx={c} iters=2",
                          "tsar_compute_disp ctx={c}", GET_RESULT,
                          "tsar_clear_geom ctx={c}", "tsar_clear_plane_prior ctx={c}"]
FILTER = ["tsar_set_geom_depths ctx={c} n_views={n} depth={maps} mem=0 weight=0 clip=3",
          "tsar_geom_check ctx={c} depth=set reproj_error=2 depth_diff=0.00999999978 min_consistent=2 count_out=null depth_out=set mem=0",
          "tsar_get_reliable_mask ctx={c} scale=set mem=0",
          "tsar_clear_geom ctx={c}"]
# --mode=tsar: the reference image alone, the external planes, then the live path's operators
LIVE = ["tsar_load_planes ctx={c} depth=set normal_world=set mem=0",
        "tsar_set_reliable_mask ctx={c} scale=set mem=0",
        "tsar_detect_weak_texture ctx={c} labels_out=null mem=0 n_regions_out=set text_out=null size_out=null cap=0",
        "tsar_getview ctx={c}",
        "tsar_ransac_regions ctx={c} region_planes_out=set inlier_ratio_out=set",
        "tsar_fake_depth ctx={c} fakedepth_out=null mem=0", "tsar_fill_textureless ctx={c}",
        GET_RESULT]


def phase1_calls(per_view, coarse=False):
    calls = ["tsar_create device=0 ctx=0"] + UPLOAD * 3
    for v in VIEWS:
        calls += start(0, v) + (["tsar_create device=0 ctx=1"] if coarse and v == 0 else []) + fmt(per_view, c=0, k=1)
    return calls + (["tsar_destroy ctx=1"] if coarse else []) + ["tsar_destroy ctx=0"]


def geom_calls(c):
    calls = [f"tsar_create device=0 ctx={c}"]
    for v in VIEWS:
        calls += start(c, v) + fmt(GEOM, c=c)
    return calls + [f"tsar_destroy ctx={c}"]


def filter_calls(c, views, sources=None):
    calls = [f"tsar_create device=0 ctx={c}"]
    for v in views:
        n = 1 + (len(sources[v]) if sources else 2)
        calls += start(c, v, n=n) + fmt(FILTER, c=c, n=n, maps=",".join(["null"] + ["set"] * (n - 1)))
    return calls + [f"tsar_destroy ctx={c}"]


def ok_lines(label):
    return "".join(f"view {v:08d} on gpu 0{label}: ok (T s)\n" for v in VIEWS)


# ---- case 1: phase 1 ------------------------------------------------------------------------------------------------------------------
def test_phase1_single_scale_and_multi_scale(tool, scene):
    r = Run(tool, scene)
    assert (r.rc, r.stderr, r.stdout) == (0, "", ok_lines(""))
    assert r.calls == phase1_calls(PHASE1) + RELEASE_IMAGES
    # --all page-locks two result sets per worker, each a depth and a normal map, and releases them
    assert sorted(r.pinned) == sorted(["tsar_host_alloc bytes=12288", "tsar_host_alloc bytes=36864"] * 2 + ["tsar_host_free p=set"] * 4)
    for v in VIEWS:
        assert not os.path.exists(scene + f"APD/{v:08d}/TSAR_multiscale.txt")
        assert np.array_equal(tio.read_dmb(scene + f"APD/{v:08d}/TSAR_disp.dmb"), STUB_DEPTH)
    # the single-scale maps are not a multi-scale run's: every view is matched again, coarse to fine, under its record
    r = Run(tool, scene, "--multi_scale=1", "--coarse_iterations=3")
    assert (r.rc, r.stderr, r.stdout) == (0, "", ok_lines(""))
    assert r.calls == phase1_calls(PHASE1_MULTI_SCALE, coarse=True) + RELEASE_IMAGES
    for v in VIEWS:
        assert rec(scene, v, "TSAR_multiscale.txt") == b"multi_scale=1 coarse_iterations=3 textureless_merge=0\n"
    r = Run(tool, scene, "--multi_scale=1", "--coarse_iterations=3")
    assert r.stdout == ("resuming: 3 of 3 views already have complete TSAR_disp.dmb / TSAR_normals.dmb and are skipped (--force recomputes them)\n" +
                        "".join(f"view {v:08d}: outputs present, skipped\n" for v in VIEWS))
    assert r.calls == []


# ---- case 2: phase 2, plain --------------------------------------------------------------------------------------------------------------
GEOM_RECORD = ("geom_iterations=2 geom_weight=0.200000003 geom_clip=3 blocksize=11 n_best=1 cost_comb=1 seed=0 strict=0 fix_quirks=0 "
               "texture_filter_8bit=0 cam_scale=1 depth_min=-1 depth_max=-1\n")


def test_phase2_plain(tool, scene):
    r = Run(tool, scene, "--geom_consistency")
    assert (r.rc, r.stderr, r.stdout) == (0, "", ok_lines("") + ok_lines(" (geom)"))
    assert r.calls == phase1_calls(PHASE1) + geom_calls(1) + RELEASE_IMAGES
    for v in VIEWS:
        assert rec(scene, v, "TSAR_geom.txt") == GEOM_RECORD.encode()
        assert np.array_equal(tio.read_dmb(scene + f"APD/{v:08d}/TSAR_geom_disp.dmb"), STUB_DEPTH)
        assert tio.read_dmb(scene + f"APD/{v:08d}/TSAR_geom_normals.dmb").shape == (H, W, 3)


# ---- case 3: phase 2 with every switch ---------------------------------------------------------------------------------------------------
def _copy_as_prior(root, views, stem="P"):
    for v in views:
        d = root + f"APD/{v:08d}/"
        shutil.copy(d + "TSAR_disp.dmb", d + stem + "_disp.dmb")
        shutil.copy(d + "TSAR_normals.dmb", d + stem + "_normals.dmb")


EVERY_SWITCH = ["--geom_consistency", "--geom_multi_scale=1", "--geom_coarse_iterations=3", "--geom_cross_view=1", "--geom_plane_prior=P"]


def test_phase2_with_every_switch(tool, scene):
    assert Run(tool, scene).rc == 0
    _copy_as_prior(scene, (0, 2))
    r = Run(tool, scene, *EVERY_SWITCH)
    d1 = scene + "APD/00000001/"
    assert (r.rc, r.stderr) == (0, "")
    assert r.stdout == ("resuming: 3 of 3 views already have complete TSAR_disp.dmb / TSAR_normals.dmb and are skipped (--force recomputes them)\n" +
                        "".join(f"view {v:08d}: outputs present, skipped\n" for v in VIEWS) +
                        "view 00000000 on gpu 0 (geom): ok (T s)\n" +
                        f"view 00000001 (geom): no plane prior ({d1}P_disp.dmb / {d1}P_normals.dmb not readable at 64 x 48): runs without one\n" +
                        "view 00000001 on gpu 0 (geom): ok (T s)\nview 00000002 on gpu 0 (geom): ok (T s)\n")
    want = ["tsar_create device=0 ctx=0"] + UPLOAD * 3
    for v in VIEWS:
        want += (start(0, v) + (["tsar_create device=0 ctx=1"] if v == 0 else []) + fmt(GEOM_EVERY_SWITCH_HEAD, c=0, k=1) +
                 (fmt([SET_PRIOR], c=0) if v != 1 else []) + fmt(GEOM_EVERY_SWITCH_TAIL, c=0, k=1))
    assert r.calls == want + ["tsar_destroy ctx=1", "tsar_destroy ctx=0"] + RELEASE_IMAGES
    assert "tsar_pm_rescore" not in "".join(r.calls)
    for v in VIEWS:
        assert rec(scene, v, "TSAR_geom.txt") == (GEOM_RECORD + "geom_cross_view=1 geom_cross_view_depth_diff=0.00999999978\n"
                                                  "geom_plane_prior=P geom_prior_weight_depth=0.100000001 geom_prior_weight_normal=0.0500000007 "
                                                  "geom_prior_depth_clip=0.0199999996 geom_prior_angle_clip=30\n"
                                                  "geom_multi_scale=1 geom_coarse_iterations=3\n").encode()


# ---- case 4: the filter after phase 2, and what a rerun skips -----------------------------------------------------------------------------
def _skips(r):
    return (r.stdout.count(": outputs present, skipped"), r.stdout.count(": geom outputs present, skipped"), r.stdout.count(": filter outputs present, skipped"))


def test_filter_after_phase2_and_resume(tool, scene):
    sources = {0: [1, 2], 1: [0, 2], 2: [1]}            # view 2 does not read view 0
    tio.write_pairs(scene + "pair.txt", {r: [(s, 1.0) for s in srcs] for r, srcs in sources.items()})
    args = ["--geom_consistency", "--geom_plane_prior=P", "--consistency_filter"]
    r = Run(tool, scene, *args)
    assert (r.rc, r.stderr) == (0, "")
    assert r.stdout.count("(geom): no plane prior") == 3
    assert r.stdout.endswith("".join(f"view {v:08d} (filter): 2048 of 3072 pixels of TSAR_geom_disp.dmb kept\nview {v:08d} on gpu 0 (filter): ok (T s)\n" for v in VIEWS))
    assert r.calls[-len(filter_calls(2, VIEWS, sources)) - 3:] == filter_calls(2, VIEWS, sources) + RELEASE_IMAGES
    for v in VIEWS:
        assert rec(scene, v, "TSAR_filter.txt") == ("min_consistent=2 reproj_error=2 depth_diff=0.00999999978 cam_scale=1 checked=TSAR_geom_disp.dmb sources=" +
                                                    ",".join(f"{s:08d}" for s in sources[v]) + "\n").encode()
        assert np.array_equal(tio.read_dmb(scene + f"APD/{v:08d}/TSAR_filtered_disp.dmb"), np.where(KEPT.reshape(H, W), STUB_DEPTH, 0))
    out = subprocess.run([tool, "--check-mask=" + scene + "APD/00000001/TSAR_consistent.png"], capture_output=True, text=True)
    assert out.stdout == f"mask 64 x 48 reliable 2048 checksum {int((np.arange(NP)[KEPT] % 9973).sum())}\n"
    # a rerun skips every view of every phase and calls nothing
    r = Run(tool, scene, *args)
    assert (r.rc, _skips(r), r.calls) == (0, (3, 3, 3), [])
    assert "geom: resuming: 3 of 3" in r.stdout and "filter: resuming: 3 of 3 views have current TSAR_filtered_disp.dmb / TSAR_consistent.png" in r.stdout
    # view 0's geom map replaced (and newer): the filter runs again for the views that read it, 0 and 1, on that map
    tio.write_dmb(scene + "APD/00000000/TSAR_geom_disp.dmb", np.full((H, W), 7.0, np.float32))
    later = time.time() + 5
    os.utime(scene + "APD/00000000/TSAR_geom_disp.dmb", (later, later))
    r = Run(tool, scene, *args)
    assert (r.rc, _skips(r)) == (0, (3, 3, 1)) and "view 00000002: filter outputs present, skipped" in r.stdout
    want = filter_calls(0, (0, 1), sources)
    assert r.calls == want[:1] + UPLOAD * 3 + want[1:] + RELEASE_IMAGES
    assert np.array_equal(tio.read_dmb(scene + "APD/00000000/TSAR_filtered_disp.dmb"), np.where(KEPT.reshape(H, W), np.float32(7.0), 0))
    # a prior file newer than a view's geom maps: that view's phase 2 runs again, with the prior, and so does the filter over its new map
    _copy_as_prior(scene, (2,))
    later += 5
    for name in ("P_disp.dmb", "P_normals.dmb"):
        os.utime(scene + "APD/00000002/" + name, (later, later))
    r = Run(tool, scene, *args)
    assert (r.rc, _skips(r)[:2]) == (0, (3, 2)) and "view 00000002 on gpu 0 (geom): ok" in r.stdout and "no plane prior" not in r.stdout
    geom2 = start(0, 2, n=2) + fmt(GEOM[:2] + [SET_PRIOR] + GEOM[2:], c=0)
    geom2[3] = geom2[3].replace("n_views=3 depth=null,set,set", "n_views=2 depth=null,set")
    assert r.calls[:len(geom2) + 5] == ["tsar_create device=0 ctx=0"] + UPLOAD * 2 + geom2
    # --force: everything again
    r = Run(tool, scene, *args, "--force")
    assert (r.rc, _skips(r)) == (0, (0, 0, 0)) and "resuming" not in r.stdout
    assert [c.split()[0] for c in r.calls].count("tsar_get_result") == 6 and [c.split()[0] for c in r.calls].count("tsar_geom_check") == 3


# ---- case 5: --fuse with --geom_consistency ------------------------------------------------------------------------------------------------
def test_fuse_with_geom_consistency(tool, scene):
    r = Run(tool, scene, "--geom_consistency", "--fuse")
    assert (r.rc, r.stderr) == (0, "")
    ply = scene + "APD/APD_TSAR.ply"
    assert re.fullmatch(re.escape(ok_lines("") + ok_lines(" (geom)")) +
                        rf"fused 3 views on gpu 0: 2 points -> {re.escape(ply)} \(gather of 0\.0 MB from other gpus \+ uploads \d+\.\d\d\d s, total \d+\.\d\d\d s\)\n", r.stdout)
    # phase 1 keeps each view's maps on its device; they are released and the geom maps read back from their files in their place
    keep = ["tsar_device_alloc device=0 bytes=12288", "tsar_device_alloc device=0 bytes=36864",
            "tsar_get_result ctx=0 depth=set normal_world=set cost=null confid=null mem=1"]
    assert r.calls == (phase1_calls(PHASE1 + keep) + geom_calls(1) + RELEASE_IMAGES +
                       (["tsar_device_free device=0 p=set"] * 2 + keep[:2] + ["tsar_device_write device=0 dst=set host_src=set bytes=12288",
                                                                              "tsar_device_write device=0 dst=set host_src=set bytes=36864"]) * 3 +
                       ["tsar_device_alloc device=0 bytes=12288", "tsar_device_write device=0 dst=set host_src=set bytes=12288"] * 3 +       # the images, as float
                       ["tsar_fuse device=0 n_views=3 w=64 h=48 cams=set depth=set normal_world=set gray=set mem=1 sources=1,2|0,2|0,1 num_consistent=1 "
                        f"reproj_error=2 depth_diff=0.00999999978 angle_deg=15 used_list=1 points_out=set cap={3 * NP} n_points_out=set"] +
                       ["tsar_device_free device=0 p=set"] * 9)
    assert os.path.getsize(ply) > 0 and b"element vertex 2" in open(ply, "rb").read(400)


# ---- case 6: an error in a later phase --------------------------------------------------------------------------------------------------------
def test_error_in_phase2_drops_the_contexts_and_retries_on_fresh_ones(tool, scene):
    assert Run(tool, scene).rc == 0
    # (the stub counts calls per process: phase 1 is skipped, so the first tsar_pm_iterate is view 0's at the coarse level)
    r = Run(tool, scene, "--geom_consistency", "--geom_multi_scale=1", env={"TSAR_STUB_FAIL": "tsar_pm_iterate:1"})
    assert r.rc == 0
    assert r.stderr == "view 00000000 (geom): tsar_pm_iterate (coarsest level): stub: injected failure\n"
    assert r.stdout.endswith("view 00000000 on gpu 0 (geom): FAILED (T s)\nview 00000001 on gpu 0 (geom): ok (T s)\nview 00000002 on gpu 0 (geom): ok (T s)\n"
                             "view 00000000 on gpu 0 (geom, retry): ok (T s)\n")
    assert "retrying once" not in r.stdout
    names = [c.split(" ", 1) for c in r.calls]
    fail_at = r.calls.index("tsar_pm_iterate ctx=1 iters=2 -> TSAR_ERR_HIP")
    # the worker's contexts go, the coarse one first; view 1 starts on fresh ones; the retry gets a worker of its own
    assert r.calls[fail_at + 1:fail_at + 5] == ["tsar_last_error ctx=1", "tsar_destroy ctx=1", "tsar_destroy ctx=0", "tsar_create device=0 ctx=2"]
    assert r.calls[fail_at + 5:fail_at + 7] == start(2, 1) and r.calls[fail_at + 7] == "tsar_create device=0 ctx=3"
    retry = r.calls.index("tsar_create device=0 ctx=4")
    assert r.calls[retry - 2:retry] == ["tsar_destroy ctx=3", "tsar_destroy ctx=2"]
    assert r.calls[retry + 1:retry + 3] == start(4, 0) and r.calls[retry + 3] == "tsar_create device=0 ctx=5"
    assert r.calls[-5:] == ["tsar_destroy ctx=5", "tsar_destroy ctx=4"] + RELEASE_IMAGES
    assert [n for n, _ in names].count("tsar_create") == [n for n, _ in names].count("tsar_destroy") == 6
    for v in VIEWS:
        assert rec(scene, v, "TSAR_geom.txt") == (GEOM_RECORD + "geom_multi_scale=1 geom_coarse_iterations=2\n").encode()


# ---- case 7: --all --mode=tsar, the live path ---------------------------------------------------------------------------------------------------
def test_all_views_live_path(tool, scene):
    rng = np.random.default_rng(4)
    for v in VIEWS:                                       # the inputs of test_io_cli's --mode=tsar test: external maps and weak.png per view
        apd = scene + f"APD/{v:08d}/"
        os.makedirs(apd, exist_ok=True)
        tio.write_dmb(apd + "depths_geom.dmb", rng.uniform(3.5, 9.0, (H, W)).astype(np.float32))
        tio.write_dmb(apd + "normals.dmb", np.tile(np.float32([0, 0, -1]), (H, W, 1)))
        tio.write_reliable_mask(apd + "weak.png", rng.uniform(size=(H, W)) < 0.7)
    r = Run(tool, scene, "--mode=tsar")
    assert (r.rc, r.stderr) == (0, "")
    assert r.stdout == "".join(f"view {v:08d}: 1 regions labelled, textureless ones refitted and filled\nview {v:08d} on gpu 0: ok (T s)\n" for v in VIEWS)
    want = ["tsar_create device=0 ctx=0"]
    for v in VIEWS:                                       # the reference image alone: one upload per view, as it is first used
        want += UPLOAD + start(0, v, n=1) + fmt(LIVE, c=0)
    assert r.calls == want + ["tsar_destroy ctx=0"] + RELEASE_IMAGES
    # the read-ahead ring: eight sets of external maps per worker, page-locked as they are first filled (three views: three sets), beside
    # the two result sets
    allocs = sorted(ln for ln in r.pinned if "alloc" in ln)
    assert allocs == sorted(["tsar_host_alloc bytes=12288", "tsar_host_alloc bytes=36864"] * 5)
    assert len(r.pinned) == 20


# ---- case 8: the checked integers, and two options that share a suffix ------------------------------------------------------------------------
@pytest.mark.parametrize("option,values,message", [
    ("--multi_scale=", ("x", "", "9", "-1"), "Command-line parameter error: {a} must be an integer in 0..8\n"),
    ("--geom_multi_scale=", ("1x", "", "9", "-1"), "Command-line parameter error: {a} must be an integer in 0..8\n"),
    ("--coarse_iterations=", ("x", "", "1000001", "-1"), "Command-line parameter error: {a} must be a non-negative integer\n"),
    ("--geom_coarse_iterations=", ("2.5", "", "1000001", "-1"), "Command-line parameter error: {a} must be a non-negative integer\n"),
    ("--geom_cross_view=", ("x", "", "0", "64"), "Command-line parameter error: --geom_cross_view=K must be an integer in 1..63\n"),
    ("--consistency_filter=", ("2k", "", "0", "32"), "Command-line parameter error: --consistency_filter=K must be an integer in 1..31\n"),
])
def test_checked_integers(tool, scene, option, values, message):
    for value in values:
        r = Run(tool, scene, "--geom_consistency", option + value)
        assert (r.rc, r.stdout, r.stderr, r.calls) == (1, message.format(a=option + value), "", [])


def test_checked_integers_at_their_limits_and_shared_suffixes(tool, scene):
    r = Run(tool, scene, "--geom_consistency", "--geom_cross_view=63", "--geom_cross_view_depth_diff=0.02", "--depth_diff=0.03", "--consistency_filter=31",
            "--multi_scale=8", "--geom_multi_scale=0", "--coarse_iterations=1000000", "--fuse", "--mystery=1")
    assert r.stdout.startswith("Command-line parameter warning: unknown option --mystery=1\n")        # unknown options only warn
    assert [c for c in r.calls if c.startswith("tsar_geom_reproject")] == ["tsar_geom_reproject ctx=9 depth_diff=0.0199999996 min_views=63 depth_out=set count_out=null mem=1"] * 3
    assert [c for c in r.calls if c.startswith("tsar_geom_check")] == [
        "tsar_geom_check ctx=10 depth=set reproj_error=2 depth_diff=0.00999999978 min_consistent=31 count_out=null depth_out=set mem=0"] * 3
    assert [c for c in r.calls if c.startswith("tsar_fuse")][0].split("num_consistent")[1].startswith("=1 reproj_error=2 depth_diff=0.0299999993 ")
    assert [c for c in r.calls if c.startswith("tsar_pm_iterate ctx=8")] == ["tsar_pm_iterate ctx=8 iters=1000000"] * 3
    assert r.rc == 0

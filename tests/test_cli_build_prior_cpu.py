"""tsar_gipuma --all --geom_consistency --geom_build_prior on the CPU: the tool linked against tests/cli_stub/tsar_stub_build_prior.cpp (the
recording stand-in of test_cli_phases_cpu.py plus the entries only this switch calls) makes the call sequence of api.run_geom_pass's
build_prior, view by view, and writes the record line; linked against the stand-in without those entries it refuses the switch with one
line and runs everything else as before; the refusals decided from the command line."""
import os
import subprocess

import pytest

from test_cli_phases_cpu import (CXXFLAGS, GEOM, GEOM_RECORD, PHASE1, RELEASE_IMAGES, ROOT, SRC, STUB, UPLOAD, VIEWS, Run, fmt, geom_calls, ok_lines,
                                 phase1_calls, rec, scene, scene_template, start, tool)     # noqa: F401 (fixtures)

STUB_BUILD = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_build_prior.cpp")


@pytest.fixture(scope="module")
def tool_build(tmp_path_factory):
    """the tool linked against the stand-in that has the builder's entries"""
    d = str(tmp_path_factory.mktemp("cli_stub_build"))
    for cmd in (["g++", *CXXFLAGS, "-std=c++17", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", STUB_BUILD],
                ["g++", *CXXFLAGS, "-std=c++17", "-pthread", "-o", d + "/tsar_gipuma", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_gipuma"


SET_PRIOR_DEVICE = "tsar_set_plane_prior ctx={c} depth=set normal_world=set mem=1 weight_depth=0.200000003 weight_normal=0.0500000007 depth_clip=0.0199999996 normal_clip=0.133974597"
# after the term is installed: three device buffers (the score, the own depth, the prior's depth and normals), rescore, the stored cost,
# the own depth to the device and checked in place, the builder, the prior, rescore (the pass's own), the buffers released
BUILD = ["tsar_device_alloc device=0 bytes=12288", "tsar_device_alloc device=0 bytes=12288", "tsar_device_alloc device=0 bytes=49152",
         "tsar_pm_rescore ctx={c}",
         "tsar_get_plane ctx={c} planes=null cost=set beview=null ratio=null mem=1",
         "tsar_device_write device=0 dst=set host_src=set bytes=12288",
         "tsar_geom_check ctx={c} depth=set reproj_error=2 depth_diff=0.00999999978 min_consistent=2 count_out=null depth_out=set mem=1",
         "tsar_build_plane_prior ctx={c} depth=set score=set mem=1 cell={cell} max_levels={levels} depth_out=set normal_world_out=set level_out=null",
         SET_PRIOR_DEVICE,
         "tsar_pm_rescore ctx={c}",
         "tsar_device_free device=0 p=set", "tsar_device_free device=0 p=set", "tsar_device_free device=0 p=set"]
BUILD_RECORD = ("geom_build_prior={cell} geom_build_prior_levels={levels} geom_build_min_consistent=2 geom_build_reproj_error=2 "
                "geom_build_depth_diff=0.00999999978 geom_prior_weight_depth=0.200000003 geom_prior_weight_normal=0.0500000007 "
                "geom_prior_depth_clip=0.0199999996 geom_prior_angle_clip=30\n")


def build_calls(c, cell, levels):
    calls = [f"tsar_create device=0 ctx={c}"]
    for v in VIEWS:
        # GEOM without its own rescore: load_planes, set_geom_depths | BUILD | iterate, compute_disp, get_result, the two clears
        calls += start(c, v) + fmt(GEOM[:2] + BUILD + GEOM[3:], c=c, cell=cell, levels=levels)
    return calls + [f"tsar_destroy ctx={c}"]


def test_the_switch_makes_the_passes_calls(tool_build, scene):
    assert GEOM[2] == "tsar_pm_rescore ctx={c}"
    r = Run(tool_build, scene, "--geom_consistency", "--geom_build_prior=6", "--geom_build_prior_levels=2", "--geom_prior_weight_depth=0.2")
    assert (r.rc, r.stderr, r.stdout) == (0, "", ok_lines("") + ok_lines(" (geom)"))
    assert r.calls == phase1_calls(PHASE1) + build_calls(1, 6, 2) + RELEASE_IMAGES
    for v in VIEWS:
        assert rec(scene, v, "TSAR_geom.txt") == (GEOM_RECORD + BUILD_RECORD.format(cell=6, levels=2)).encode()
    # a rerun skips; the defaults are another record, so every view runs again
    r = Run(tool_build, scene, "--geom_consistency", "--geom_build_prior=6", "--geom_build_prior_levels=2", "--geom_prior_weight_depth=0.2")
    assert r.calls == [] and r.stdout.count(": geom outputs present, skipped") == 3
    r = Run(tool_build, scene, "--geom_consistency", "--geom_build_prior", "--geom_prior_weight_depth=0.2")
    assert r.rc == 0 and r.calls == build_calls(0, 4, 0)[:1] + UPLOAD * 3 + build_calls(0, 4, 0)[1:] + RELEASE_IMAGES
    assert rec(scene, 0, "TSAR_geom.txt") == (GEOM_RECORD + BUILD_RECORD.format(cell=4, levels=0)).encode()
    # without the switch: the pass and the record as they always were
    r = Run(tool_build, scene, "--geom_consistency")
    assert r.rc == 0 and r.calls == geom_calls(0)[:1] + UPLOAD * 3 + geom_calls(0)[1:] + RELEASE_IMAGES
    assert rec(scene, 0, "TSAR_geom.txt") == GEOM_RECORD.encode()


def test_a_failing_builder_releases_its_buffers(tool_build, scene):
    r = Run(tool_build, scene, "--geom_consistency", "--geom_build_prior", env={"TSAR_STUB_FAIL": "tsar_build_plane_prior:1"})
    names = [c.split()[0] for c in r.calls]
    assert r.rc == 0 and names.count("tsar_build_plane_prior") == 4          # (the failed view is retried once, on a fresh context)
    first = names.index("tsar_build_plane_prior")
    assert names[first + 1:first + 4] == ["tsar_device_free"] * 3 and "tsar_set_plane_prior" not in names[first:first + 4]


def test_a_library_without_the_entry_refuses_the_switch(tool, scene):
    """the tool linked against the stand-in of test_cli_phases_cpu.py, which has neither tsar_build_plane_prior nor tsar_get_plane"""
    r = Run(tool, scene, "--geom_consistency", "--geom_build_prior")
    assert r.rc != 0 and r.calls == [] and r.stdout == ""
    assert r.stderr == "--geom_build_prior: this libtsar_hip.so has no tsar_build_plane_prior\n"
    r = Run(tool, scene, "--geom_consistency")                       # everything else runs there as before
    assert r.rc == 0 and r.calls == phase1_calls(PHASE1) + geom_calls(1) + RELEASE_IMAGES


@pytest.mark.parametrize("args,message", [
    (["--geom_build_prior"], "work with --geom_consistency only"),
    (["--geom_build_prior_levels=2"], "work with --geom_consistency only"),
    (["--geom_consistency", "--geom_build_prior_levels=2"], "--geom_build_prior_levels needs --geom_build_prior"),
    (["--geom_consistency", "--geom_build_prior", "--geom_plane_prior=P"], "mutually exclusive"),
    (["--geom_consistency", "--geom_build_prior=1"], "--geom_build_prior=CELL must be an integer in 2..256"),
    (["--geom_consistency", "--geom_build_prior=257"], "--geom_build_prior=CELL must be an integer in 2..256"),
    (["--geom_consistency", "--geom_build_prior=x"], "--geom_build_prior=CELL must be an integer in 2..256"),
    (["--geom_consistency", "--geom_build_prior", "--geom_build_prior_levels=17"], "--geom_build_prior_levels=N must be an integer in 0..16"),
    (["--geom_consistency", "--geom_build_prior", "--geom_build_prior_levels=-1"], "--geom_build_prior_levels=N must be an integer in 0..16"),
    (["--geom_consistency", "--geom_build_prior", "--geom_prior_depth_clip=0"], "--geom_prior_depth_clip finite and > 0"),
])
def test_refusals(tool_build, scene, args, message):
    r = Run(tool_build, scene, *args)
    assert r.rc != 0 and r.calls == []
    assert message in r.stdout + r.stderr


def test_usage_names_the_switch(tool_build):
    out = subprocess.run([tool_build], capture_output=True, text=True, timeout=60)
    assert "--geom_build_prior[=CELL]" in out.stdout and "--geom_build_prior_levels=N" in out.stdout

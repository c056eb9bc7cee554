"""tsar_gipuma --all's settings records on the CPU: TSAR_geom.txt (phase 2, --geom_consistency) and TSAR_multiscale.txt (phase 1,
--multi_scale) decide whether an existing output folder resumes.  Both records are pinned byte for byte here, and phase 2's retry
path runs: a view that has to be matched again cannot get a device on this machine, fails, is retried once and is reported missing."""
import os
import subprocess
import time

import numpy as np
import pytest

from tsar_mvs_amd import io as tio
from tsar_mvs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")

# what the tool writes for --iterations=1 --blocksize=11 --n_best=1, every other option at its default
GEOM_RECORD = ("geom_iterations=2 geom_weight=0.200000003 geom_clip=3 blocksize=11 n_best=1 cost_comb=1 seed=0 strict=0 fix_quirks=0 "
               "texture_filter_8bit=0 cam_scale=1 depth_min=-1 depth_max=-1\n")
MS_RECORD = "multi_scale=1 coarse_iterations=1 textureless_merge=0\n"
VIEWS = range(3)


@pytest.fixture
def scene(tmp_path):
    """a 64 x 48 scene of three views, each with complete phase-1 maps; returns (root, command line)"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the failing half of this test would match the view instead")
    if not os.path.exists(CLI):
        pytest.fail("tsar_gipuma is not built (__graft_entry__.build())")
    sc = synth.make_scene(64, 48, 2, seed=2)
    root = str(tmp_path) + "/"
    tio.export_scene(sc, root)
    for v in VIEWS:
        os.makedirs(root + f"APD/{v:08d}", exist_ok=True)
        tio.write_dmb(root + f"APD/{v:08d}/TSAR_disp.dmb", np.ones((48, 64), np.float32))
        tio.write_dmb(root + f"APD/{v:08d}/TSAR_normals.dmb", np.zeros((48, 64, 3), np.float32))
    cmd = [CLI, "--all", "--gpus=1", "-mslp_folder", root, "-images_folder", root + "images/", "--iterations=1", "--blocksize=11", "--n_best=1"]
    return root, cmd


def _write_geom_outputs(root):
    """every view's geom maps and record, all newer than every input (the views' phase-1 maps)"""
    now = time.time()
    for v in VIEWS:
        d = root + f"APD/{v:08d}/"
        tio.write_dmb(d + "TSAR_geom_disp.dmb", np.ones((48, 64), np.float32))
        tio.write_dmb(d + "TSAR_geom_normals.dmb", np.zeros((48, 64, 3), np.float32))
        with open(d + "TSAR_geom.txt", "w") as f:
            f.write(GEOM_RECORD)
        for name in ("TSAR_disp.dmb", "TSAR_normals.dmb"):
            os.utime(d + name, (now - 100, now - 100))
        for name in ("TSAR_geom_disp.dmb", "TSAR_geom_normals.dmb", "TSAR_geom.txt"):
            os.utime(d + name, (now, now))


def _run(cmd, *extra):
    return subprocess.run([*cmd, *extra], capture_output=True, text=True, timeout=120)


def test_geom_record_resumes_every_view(scene):
    root, cmd = scene
    _write_geom_outputs(root)
    out = _run(cmd, "--geom_consistency")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("view 0000000") == 6, out.stdout        # three skip lines per phase, nothing else per view
    assert out.stdout.count(": outputs present, skipped") == 3 and "resuming: 3 of 3" in out.stdout
    assert out.stdout.count("geom outputs present, skipped") == 3 and "geom: resuming: 3 of 3" in out.stdout


@pytest.mark.parametrize("damage", ["record", "map"])
def test_stale_or_broken_geom_outputs_are_attempted_and_retried(scene, damage):
    root, cmd = scene
    _write_geom_outputs(root)
    d = root + "APD/00000001/"
    if damage == "record":
        with open(d + "TSAR_geom.txt", "w") as f:
            f.write(GEOM_RECORD.replace("geom_iterations=2", "geom_iterations=3"))
    else:
        raw = open(d + "TSAR_geom_normals.dmb", "rb").read()
        open(d + "TSAR_geom_normals.dmb", "wb").write(raw[:-4])
    out = _run(cmd, "--geom_consistency")
    assert out.returncode != 0, out.stdout + out.stderr
    assert out.stdout.count(": outputs present, skipped") == 3          # phase 1 resumes every view
    assert out.stdout.count("geom outputs present, skipped") == 2 and "geom: resuming: 2 of 3" in out.stdout
    assert "view 00000001 on gpu 0 (geom): FAILED" in out.stdout
    assert "view 00000001 on gpu 0 (geom, retry): FAILED" in out.stdout
    assert "retrying once" not in out.stdout                             # phase 2 announces no retry
    assert "view 00000001: geom outputs missing" in out.stderr
    assert out.stderr.count("geom outputs missing") == 1


def test_multiscale_record_decides_the_resume(scene):
    root, cmd = scene
    for v in (0, 2):
        with open(root + f"APD/{v:08d}/TSAR_multiscale.txt", "w") as f:
            f.write(MS_RECORD)
    out = _run(cmd, "--multi_scale=1")
    assert out.returncode != 0, out.stdout + out.stderr
    assert out.stdout.count("outputs present, skipped") == 2 and "resuming: 2 of 3" in out.stdout
    assert "view 00000000: outputs present, skipped" in out.stdout and "view 00000002: outputs present, skipped" in out.stdout
    assert "view 00000001 on gpu 0: FAILED" in out.stdout
    assert "view 00000001 FAILED on gpu 0: retrying once on gpu 0 with a fresh context" in out.stdout
    assert "view 00000001 on gpu 0 (retry): FAILED" in out.stdout
    assert "view 00000001: outputs missing or incomplete" in out.stderr
    # a single-scale run does not take the multi-scale maps for its own
    out = _run(cmd)
    assert out.returncode != 0, out.stdout + out.stderr
    assert out.stdout.count("outputs present, skipped") == 1 and "view 00000001: outputs present, skipped" in out.stdout
    for v in (0, 2):
        assert f"view {v:08d} on gpu 0 (retry): FAILED" in out.stdout
        assert f"view {v:08d}: outputs missing or incomplete" in out.stderr

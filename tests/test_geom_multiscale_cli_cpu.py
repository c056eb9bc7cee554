"""tsar_gipuma's --geom_multi_scale / --geom_coarse_iterations refusals, decided from the command line before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")


def _run(tmp_path, *args):
    if not os.path.exists(CLI):
        pytest.fail("tsar_gipuma is not built (__graft_entry__.build())")
    common = ["-mslp_folder", str(tmp_path) + "/", "-images_folder", str(tmp_path) + "/images/"]
    return subprocess.run([CLI, "--all", *common, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,message", [
    (["--geom_multi_scale=1"], "--geom_multi_scale / --geom_coarse_iterations work with --geom_consistency only"),
    (["--geom_multi_scale=2", "--geom_coarse_iterations=4"], "work with --geom_consistency only"),
    (["--geom_consistency", "--geom_coarse_iterations=4"], "--geom_coarse_iterations needs --geom_multi_scale=L with L >= 1"),
    (["--geom_consistency", "--geom_multi_scale=9"], "must be an integer in 0..8"),
    (["--geom_consistency", "--geom_multi_scale=x"], "must be an integer in 0..8"),
    (["--geom_consistency", "--geom_multi_scale=1", "--geom_coarse_iterations=-1"], "must be a non-negative integer"),
])
def test_refusals(tmp_path, args, message):
    out = _run(tmp_path, *args)
    assert out.returncode != 0
    assert message in out.stdout + out.stderr


def test_usage_names_the_options(tmp_path):
    out = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--geom_multi_scale=L" in out.stdout and "--geom_coarse_iterations=N" in out.stdout

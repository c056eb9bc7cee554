"""tsar_gipuma's --geom_plane_prior refusals and usage text, decided from the command line before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tsar-mvs_amd", "tsar_gipuma")

NEEDS_GEOM = "--geom_plane_prior and its settings work with --geom_consistency only"
NEEDS_SWITCH = "need --geom_plane_prior=STEM"
BAD_STEM = "STEM must be a non-empty file-name stem without a path separator"
OWN_OUTPUTS = "TSAR and TSAR_geom name a phase's own outputs"
RANGES = "--geom_prior_depth_clip finite and > 0, --geom_prior_angle_clip in (0, 180] degrees"


def _run(tmp_path, *args):
    if not os.path.exists(CLI):
        pytest.fail("tsar_gipuma is not built (__graft_entry__.build())")
    common = ["-mslp_folder", str(tmp_path) + "/", "-images_folder", str(tmp_path) + "/images/"]
    return subprocess.run([CLI, "--all", *common, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,message", [
    (["--geom_plane_prior=PRIOR"], NEEDS_GEOM),                                     # --geom_consistency is absent
    (["--geom_prior_weight_depth=0.2"], NEEDS_GEOM),
    (["--geom_consistency", "--geom_plane_prior="], BAD_STEM),
    (["--geom_consistency", "--geom_plane_prior=a/b"], BAD_STEM),
    (["--geom_consistency", "--geom_plane_prior=../PRIOR"], BAD_STEM),
    (["--geom_consistency", "--geom_plane_prior=a\\b"], BAD_STEM),
    (["--geom_consistency", "--geom_plane_prior=TSAR"], OWN_OUTPUTS),
    (["--geom_consistency", "--geom_plane_prior=TSAR_geom"], OWN_OUTPUTS),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_weight_depth=-0.1"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_weight_depth=inf"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_weight_normal=-1"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_weight_normal=nan"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_depth_clip=0"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_depth_clip=inf"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_angle_clip=0"], RANGES),
    (["--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_angle_clip=181"], RANGES),
    (["--geom_consistency", "--geom_prior_weight_depth=0.2"], NEEDS_SWITCH),        # a setting without the switch, four times
    (["--geom_consistency", "--geom_prior_weight_normal=0.1"], NEEDS_SWITCH),
    (["--geom_consistency", "--geom_prior_depth_clip=0.05"], NEEDS_SWITCH),
    (["--geom_consistency", "--geom_prior_angle_clip=20"], NEEDS_SWITCH),
])
def test_refusals(tmp_path, args, message):
    out = _run(tmp_path, *args)
    assert out.returncode != 0
    assert message in out.stdout + out.stderr


def test_a_valid_command_line_passes_the_refusals(tmp_path):
    """the same settings inside their ranges get past the command-line checks: the run then stops for want of pair.txt"""
    out = _run(tmp_path, "--geom_consistency", "--geom_plane_prior=PRIOR", "--geom_prior_weight_depth=0", "--geom_prior_weight_normal=0.2",
               "--geom_prior_depth_clip=0.05", "--geom_prior_angle_clip=180")
    assert out.returncode != 0
    assert "pair.txt" in out.stdout + out.stderr


def test_usage_names_the_options(tmp_path):
    out = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    for opt in ("--geom_plane_prior=STEM", "--geom_prior_weight_depth=W", "--geom_prior_weight_normal=W", "--geom_prior_depth_clip=REL",
                "--geom_prior_angle_clip=DEG"):
        assert opt in out.stdout, opt

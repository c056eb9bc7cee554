"""tsar_evaluate --voxel= / --crop= on the CPU: host/tsar_evaluate.cpp linked against tests/cli_stub/tsar_stub_voxels.cpp (the cloud-distance
entries plus tsar_cloud_voxels by brute force on the host).  Every integer field of the JSON record and every float64 ratio equals the numpy
restatement's (tests/cloud_voxels_ref.py); the new refusals give one line and a non-zero exit; against the stand-in without the voxel entry
the tool refuses --voxel= in one line and still runs without it."""
import json
import os
import subprocess

import numpy as np
import pytest

from cloud_voxels_ref import density_case, evaluate_voxel_ref
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_voxels.cpp")
OLD_STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_cloud.cpp")
F = np.float32


def build(d, stub):
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", stub],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_evaluate"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_voxels")), STUB)


@pytest.fixture(scope="module")
def old_tool(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_no_voxels")), OLD_STUB)


def run(tool, *args):
    return subprocess.run([tool, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def clouds():
    """a noisy copy of part of a random cloud, denser in one corner, with a few non-finite records"""
    rng = np.random.default_rng(21)
    gt = rng.random((700, 3), dtype=F)
    recon = (gt[:450] + rng.normal(scale=0.02, size=(450, 3))).astype(F)
    recon = np.concatenate([recon, (rng.random((250, 3), dtype=F) * F(0.2)).astype(F)])
    recon[7] = [np.nan, 0, 0]
    gt[9, 2] = np.inf
    return recon, gt


def check_record(rec, ref, voxel=None, crop=None):
    for k in ("n_recon_valid", "n_gt_valid"):
        assert rec[k] == ref[k]
    for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1"):
        assert rec[k] == ref[k].tolist(), k
    if voxel is not None:
        assert F(rec["voxel"]) == F(voxel)
        assert rec["n_recon_voxels"] == ref["n_recon_voxels"] and rec["n_gt_voxels"] == ref["n_gt_voxels"]
        for k in ("accuracy_voxel", "completeness_voxel", "f1_voxel"):
            assert rec[k] == ref[k].tolist(), k                                    # float64 for float64: %.17g names the double
    else:
        assert not any(k in rec for k in ("voxel", "n_recon_voxels", "n_gt_voxels", "accuracy_voxel", "completeness_voxel", "f1_voxel"))
    if crop is not None:
        assert [F(v) for v in rec["crop"]] == [F(v) for v in crop]
        assert rec["n_recon_cropped"] == ref["n_recon_cropped"] and rec["n_gt_cropped"] == ref["n_gt_cropped"]
    else:
        assert not any(k in rec for k in ("crop", "n_recon_cropped", "n_gt_cropped"))


@pytest.mark.parametrize("voxel,crop", [(0.11, None), (None, (0.1, 0.0, 0.05, 0.9, 1.0, 0.8)), (0.07, (0.1, 0.0, 0.05, 0.9, 1.0, 0.8)), (5.0, None)])
def test_json_equals_the_restatement(tool, clouds, tmp_path, voxel, crop):
    recon, gt = clouds
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt, binary=False)
    tol = [0.01, 0.03, 0.1]
    args = ["--tolerances=0.01,0.03,0.1", "--json=" + str(tmp_path / "r.json")]
    if voxel is not None:
        args.append("--voxel=%.9g" % voxel)
    if crop is not None:
        args.append("--crop=" + ",".join("%.9g" % v for v in crop))
    out = run(tool, a, b, *args)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    head = ["tolerance", "accuracy", "completeness", "f1", "n_accurate", "n_complete"] + (["accuracy_voxel", "completeness_voxel", "f1_voxel"] if voxel is not None else [])
    assert lines[0].split() == head and len(lines) == 1 + len(tol) + 1 and all(len(row.split()) == len(head) for row in lines[1:-1])
    rec = json.loads(lines[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    ref = evaluate_voxel_ref(recon, gt, tol, voxel=voxel, crop=crop)
    check_record(rec, ref, voxel, crop)
    assert rec["n_recon"] == len(recon) and rec["n_gt"] == len(gt)
    if voxel == 0.11:                                                               # the case says something: the dense corner weighs less per voxel
        assert 1 < ref["n_recon_voxels"] < ref["n_recon_valid"] and 0 < ref["accuracy_voxel"][1] < 1 and ref["accuracy_voxel"][1] != ref["accuracy"][1]
    if voxel == 5.0:                                                                # one voxel: the voxel average is the point-wise share
        assert ref["n_recon_voxels"] == 1 and ref["accuracy_voxel"].tolist() == ref["accuracy"].tolist()
    if crop is not None:
        assert 0 < ref["n_recon_cropped"] < len(recon) and 0 < ref["n_gt_cropped"] < len(gt)
        assert ref["n_recon_valid"] == 699 - ref["n_recon_cropped"] and ref["n_gt_valid"] == 699 - ref["n_gt_cropped"]


def test_the_density_case(tool, tmp_path):
    recon, gt, tau, voxel = density_case()
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt)
    out = run(tool, a, b, "--tolerances=%.9g" % tau, "--voxel=%.9g" % voxel)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec["n_accurate"] == [32] and rec["n_recon_valid"] == 352 and rec["accuracy"] == [32 / 352]
    assert rec["accuracy_voxel"] == [0.5] and rec["n_recon_voxels"] == 64 and rec["completeness_voxel"] == [0.5] and rec["f1_voxel"] == [0.5]
    out = run(tool, a, b, "--tolerances=%.9g" % tau, "--voxel=%.9g" % voxel, "--crop=4,0,-1,8,8,1")
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec["accuracy_voxel"] == [1.0] and rec["accuracy"] == [1.0] and (rec["n_recon_cropped"], rec["n_gt_cropped"]) == (320, 32)


def test_without_the_switches_the_output_is_as_before(tool, old_tool, clouds, tmp_path):
    """the same bytes on stdout as the tool built against the stand-in without the voxel entry, the two times apart"""
    recon, gt = clouds
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt)
    outs = [run(t, a, b, "--tolerances=0.02,0.05") for t in (tool, old_tool)]
    assert all(o.returncode == 0 and o.stderr == "" for o in outs)
    recs = [json.loads(o.stdout.splitlines()[-1]) for o in outs]
    assert list(recs[0]) == ["recon", "gt", "n_recon", "n_gt", "n_recon_valid", "n_gt_valid", "tolerances", "n_accurate", "n_complete", "accuracy", "completeness",
                             "f1", "pairs_accuracy", "pairs_completeness", "ms_accuracy", "ms_completeness"]
    for r in recs:
        r.pop("ms_accuracy"), r.pop("ms_completeness")
    assert recs[0] == recs[1] and outs[0].stdout.splitlines()[:-1] == outs[1].stdout.splitlines()[:-1]


VOXEL_MSG = "--voxel=V must be a finite number > 0"
CROP_MSG = "--crop=x0,y0,z0,x1,y1,z1 must be six finite numbers with x0 <= x1, y0 <= y1 and z0 <= z1"


@pytest.mark.parametrize("args,message", [
    (["--voxel="], VOXEL_MSG), (["--voxel=0"], VOXEL_MSG), (["--voxel=-1"], VOXEL_MSG), (["--voxel=inf"], VOXEL_MSG), (["--voxel=nan"], VOXEL_MSG),
    (["--voxel=1e-60"], VOXEL_MSG), (["--voxel=0.1x"], VOXEL_MSG), (["--voxel=1e60"], VOXEL_MSG),
    (["--crop="], CROP_MSG), (["--crop=0,0,0,1,1"], CROP_MSG), (["--crop=0,0,0,1,1,1,1"], CROP_MSG), (["--crop=0,0,0,1,1,nan"], CROP_MSG),
    (["--crop=0,0,0,inf,1,1"], CROP_MSG), (["--crop=0,0,0,1,1,x"], CROP_MSG), (["--crop=2,0,0,1,1,1"], CROP_MSG), (["--crop=0,0,2,1,1,1"], CROP_MSG),
    (["--crop=0;0;0;1;1;1"], CROP_MSG),
])
def test_command_line_refusals(tool, tmp_path, args, message):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((2, 3), F))
    out = run(tool, good, good, "--tolerances=0.1", *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message + "\n"


def test_a_degenerate_crop_box_and_the_library_s_refusal(tool, tmp_path):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.array([[0, 0, 0], [1, 1, 1], [4e6, 0, 0]], F))
    out = run(tool, good, good, "--tolerances=0.1", "--crop=1,1,1,1,1,1", "--voxel=1")          # a box of one point is a box
    rec = json.loads(out.stdout.splitlines()[-1])
    assert out.returncode == 0 and rec["n_recon_valid"] == 1 and rec["n_recon_cropped"] == 2 and rec["n_recon_voxels"] == 1 and rec["accuracy_voxel"] == [1.0]
    out = run(tool, good, good, "--tolerances=0.1", "--voxel=1")                                  # 4e6 cells on x: the library's message is passed on
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "tsar_cloud_voxels: 2^21 cells or more on an axis\n"


def test_a_library_without_the_entry_refuses_the_switch_in_one_line(old_tool, clouds, tmp_path):
    recon, gt = clouds
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt)
    out = run(old_tool, a, b, "--tolerances=0.05", "--voxel=0.1")
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "--voxel: this libtsar_hip.so has no tsar_cloud_voxels\n"
    out = run(old_tool, a, b, "--tolerances=0.05", "--crop=0,0,0,0.5,0.5,0.5")                    # the crop needs no new entry
    assert out.returncode == 0 and json.loads(out.stdout.splitlines()[-1])["n_recon_cropped"] > 0
    assert run(old_tool, a, b, "--tolerances=0.05").returncode == 0

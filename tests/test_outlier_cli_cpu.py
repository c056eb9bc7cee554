"""tsar_evaluate --clean_* on the CPU: host/tsar_evaluate.cpp linked against tests/cli_stub/tsar_stub_neighbors.cpp (the earlier stand-ins'
entries plus tsar_cloud_neighbors by brute force on the host).  Every integer field of the JSON record and every float64 ratio equals the
numpy restatement's (tests/cloud_neighbors_ref.py); without the switch the output is what it was; every refusal gives one line and a non-zero
exit; against the stand-ins without the entry the tool refuses the switch in one line and still runs without it."""
import json
import os
import subprocess

import numpy as np
import pytest

from cloud_neighbors_ref import evaluate_clean_ref, stray_scene
from cloud_voxels_ref import evaluate_voxel_ref
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_neighbors.cpp")
OLD_STUBS = {"voxels": os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_voxels.cpp"), "cloud": os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_cloud.cpp")}
F = np.float32


def build(d, stub):
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", stub],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_evaluate"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_neighbors")), STUB)


@pytest.fixture(scope="module", params=sorted(OLD_STUBS))
def old_tool(request, tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_no_neighbors_" + request.param)), OLD_STUBS[request.param])


def run(tool, *args):
    return subprocess.run([tool, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a thinned copy of the stray scene as RECON (with a few non-finite records), its surface as GT"""
    d = tmp_path_factory.mktemp("outlier_cli_clouds")
    scene = stray_scene()
    recon = np.concatenate([scene[:3000:4], scene[3000:3100]])
    recon[5] = [np.nan, 0, 0]
    recon[11, 2] = np.inf
    gt = scene[1:3000:4].copy()
    a, b = str(d / "recon.ply"), str(d / "gt.ply")
    tio.write_ply(a, recon)
    tio.write_ply(b, gt)
    return recon, gt, a, b


CASES = [dict(radius=0.12, min_neighbors=6), dict(radius=0.12, k=8), dict(radius=0.12, k=8, ratio=1.25), dict(radius=0.12, min_neighbors=4, k=3, ratio=3.0),
         dict(radius=0.001, k=2)]


def switches(clean):
    names = {"radius": "radius", "min_neighbors": "min_neighbors", "k": "knn", "ratio": "ratio"}
    return ["--clean_%s=%.9g" % (names[k], v) for k, v in clean.items()]


@pytest.mark.parametrize("clean", CASES, ids=lambda c: "-".join("%s%g" % kv for kv in c.items()))
@pytest.mark.parametrize("more", [{}, {"voxel": 0.11, "crop": (0.1, 0.0, 0.05, 0.9, 1.0, 0.8)}], ids=["plain", "voxel-crop"])
def test_json_equals_the_restatement(tool, files, tmp_path, clean, more):
    recon, gt, a, b = files
    tol = [0.01, 0.03]
    args = ["--tolerances=0.01,0.03", "--json=" + str(tmp_path / "r.json")] + switches(clean)
    if more:
        args += ["--voxel=%.9g" % more["voxel"], "--crop=" + ",".join("%.9g" % v for v in more["crop"])]
    out = run(tool, a, b, *args)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    ref = evaluate_clean_ref(recon, gt, tol, clean, **more)
    for k in ("n_recon_valid", "n_gt_valid", "n_recon_cleaned"):
        assert rec[k] == ref[k], k
    for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1"):
        assert rec[k] == ref[k].tolist(), k                                       # float64 for float64: %.17g names the double
    if more:
        for k in ("n_recon_voxels", "n_gt_voxels", "n_recon_cropped", "n_gt_cropped"):
            assert rec[k] == ref[k], k
        for k in ("accuracy_voxel", "completeness_voxel", "f1_voxel"):
            assert rec[k] == ref[k].tolist(), k
    c = rec["clean"]
    assert list(c) == ["radius", "min_neighbors", "k", "ratio"]
    assert F(c["radius"]) == F(clean["radius"]) and c["min_neighbors"] == clean.get("min_neighbors") and c["k"] == clean.get("k") and F(c["ratio"]) == F(clean.get("ratio", 2.0))
    assert rec["n_recon"] == len(recon) and list(rec)[-2:] == ["clean", "n_recon_cleaned"]
    n_cand = len(recon) - 2
    if clean["radius"] == 0.001:                                                  # no finite k-th distance: nothing passes
        assert ref["n_recon_cleaned"] == n_cand and rec["n_recon_valid"] == 0 and rec["accuracy"] == [0.0, 0.0]
    else:                                                                         # the case says something: strays go, the surface stays
        assert 50 <= ref["n_recon_cleaned"] <= n_cand // 2 and (more or rec["n_recon_valid"] == n_cand - ref["n_recon_cleaned"])
        assert ref["accuracy"][1] > evaluate_voxel_ref(recon, gt, tol, **more)["accuracy"][1]


def test_without_the_switch_the_output_is_as_before(tool, old_tool, files):
    """the same record and table as the tool built against a stand-in without the entry, the two times apart; no new key"""
    _, _, a, b = files
    outs = [run(t, a, b, "--tolerances=0.02,0.05") for t in (tool, old_tool)]
    assert all(o.returncode == 0 and o.stderr == "" for o in outs)
    recs = [json.loads(o.stdout.splitlines()[-1]) for o in outs]
    assert list(recs[0]) == ["recon", "gt", "n_recon", "n_gt", "n_recon_valid", "n_gt_valid", "tolerances", "n_accurate", "n_complete", "accuracy", "completeness",
                             "f1", "pairs_accuracy", "pairs_completeness", "ms_accuracy", "ms_completeness"]
    assert "clean" not in recs[0] and "n_recon_cleaned" not in recs[0]
    for r in recs:
        r.pop("ms_accuracy"), r.pop("ms_completeness")
    assert recs[0] == recs[1] and outs[0].stdout.splitlines()[:-1] == outs[1].stdout.splitlines()[:-1]


R_MSG = "--clean_radius=R must be a finite number > 0"
N_MSG = "--clean_min_neighbors=N must be an integer >= 1"
K_MSG = "--clean_knn=K must be an integer in 1..32"
Q_MSG = "--clean_ratio=Q must be a finite number > 0"
NEED_RULE = "--clean_radius=R needs --clean_min_neighbors=N, --clean_knn=K or both"
NEED_RADIUS = "--clean_min_neighbors=, --clean_knn= and --clean_ratio= need --clean_radius=R"


@pytest.mark.parametrize("args,message", [
    (["--clean_radius=0.1"], NEED_RULE), (["--clean_radius=0.1", "--clean_ratio=2"], NEED_RULE),
    (["--clean_radius=0.1", "--clean_min_neighbors=0"], N_MSG), (["--clean_radius=0.1", "--clean_min_neighbors=-3"], N_MSG),
    (["--clean_radius=0.1", "--clean_min_neighbors=2.5"], N_MSG), (["--clean_radius=0.1", "--clean_min_neighbors="], N_MSG),
    (["--clean_radius=0.1", "--clean_knn=0"], K_MSG), (["--clean_radius=0.1", "--clean_knn=33"], K_MSG), (["--clean_radius=0.1", "--clean_knn=x"], K_MSG),
    (["--clean_radius=0.1", "--clean_knn=4", "--clean_ratio=0"], Q_MSG), (["--clean_radius=0.1", "--clean_knn=4", "--clean_ratio=-1"], Q_MSG),
    (["--clean_radius=0.1", "--clean_knn=4", "--clean_ratio=inf"], Q_MSG), (["--clean_radius=0.1", "--clean_knn=4", "--clean_ratio=nan"], Q_MSG),
    (["--clean_radius=0.1", "--clean_knn=4", "--clean_ratio=2x"], Q_MSG),
    (["--clean_radius=0", "--clean_knn=4"], R_MSG), (["--clean_radius=-1", "--clean_knn=4"], R_MSG), (["--clean_radius=inf", "--clean_knn=4"], R_MSG),
    (["--clean_radius=nan", "--clean_knn=4"], R_MSG), (["--clean_radius=", "--clean_knn=4"], R_MSG), (["--clean_radius=1e60", "--clean_knn=4"], R_MSG),
    (["--clean_radius=1e-60", "--clean_knn=4"], R_MSG),
    (["--clean_min_neighbors=3"], NEED_RADIUS), (["--clean_knn=3"], NEED_RADIUS), (["--clean_ratio=3"], NEED_RADIUS), (["--clean_knn=3", "--clean_ratio=3"], NEED_RADIUS),
    (["--clean_radius=0.1", "--clean_min_neighbors=3", "--clean_ratio=3"], "--clean_ratio=Q needs --clean_knn=K"),
])
def test_command_line_refusals(tool, tmp_path, args, message):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((2, 3), F))
    out = run(tool, good, good, "--tolerances=0.1", *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message + "\n"


def test_the_library_s_refusal_is_passed_on(tool, tmp_path):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((2, 3), F))
    out = run(tool, good, good, "--tolerances=0.1", "--clean_radius=1e-30", "--clean_knn=2")           # R is a float32, R * R is not
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "tsar_cloud_neighbors: radius must be finite and > 0\n"


def test_a_library_without_the_entry_refuses_the_switch_in_one_line(old_tool, files):
    _, _, a, b = files
    out = run(old_tool, a, b, "--tolerances=0.05", "--clean_radius=0.1", "--clean_knn=4")
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "--clean_radius: this libtsar_hip.so has no tsar_cloud_neighbors\n"
    assert run(old_tool, a, b, "--tolerances=0.05").returncode == 0

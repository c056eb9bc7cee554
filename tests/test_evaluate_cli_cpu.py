"""tsar_evaluate on the CPU: host/tsar_evaluate.cpp linked against tests/cli_stub/tsar_stub_cloud.cpp, which implements the cloud-distance
entries by brute force on the host.  ASCII and binary PLYs with extra properties, double coordinates and a trailing face element go in;
the JSON record's counts equal the numpy restatement's exactly; every refusal gives its one-line message and a non-zero exit."""
import json
import os
import subprocess

import numpy as np
import pytest

from cloud_distance_ref import evaluate_ref
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_cloud.cpp")
F = np.float32
XYZ = b"property float x\nproperty float y\nproperty float z\n"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_stub_cloud"))
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", d + "/libtsar_hip.so", STUB],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_evaluate"


def run(tool, *args):
    return subprocess.run([tool, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(11)
    gt = rng.random((700, 3), dtype=F)
    recon = (gt[:500] + rng.normal(scale=0.02, size=(500, 3))).astype(F)
    recon[7] = [np.nan, 0, 0]
    gt[9, 2] = np.inf
    return recon, gt


def write_rich_binary(path, xyz):
    """binary little-endian: a colour byte first, double z, float x, a normal component, double y; one face afterwards"""
    rec = np.zeros(len(xyz), np.dtype([("red", "u1"), ("z", "<f8"), ("x", "<f4"), ("nx", "<f4"), ("y", "<f8")]))
    rec["x"], rec["y"], rec["z"], rec["red"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 200
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\ncomment extra properties\nelement vertex %d\nproperty uchar red\nproperty double z\nproperty float x\n"
                b"property float nx\nproperty double y\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n" % len(xyz))
        f.write(rec.tobytes() + bytes([3, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0]))


def write_rich_ascii(path, xyz):
    with open(path, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex %d\nproperty int id\nproperty double y\nproperty float z\nproperty float x\nelement face 1\n"
                b"property list uchar int vertex_indices\nend_header\n" % len(xyz))
        f.write("".join("%d %.9g %.9g %.9g\n" % (k, r[1], r[2], r[0]) for k, r in enumerate(xyz.tolist())).encode())
        f.write(b"3 0 1 2\n")


def check_record(rec, recon, gt, tol):
    ref = evaluate_ref(recon, gt, tol)
    assert rec["n_recon"] == len(recon) and rec["n_gt"] == len(gt)
    assert rec["n_recon_valid"] == ref["n_recon_valid"] and rec["n_gt_valid"] == ref["n_gt_valid"]
    assert [F(t) for t in rec["tolerances"]] == [F(t) for t in tol]                    # nine significant digits name the float32
    assert rec["n_accurate"] == ref["n_accurate"].tolist() and rec["n_complete"] == ref["n_complete"].tolist()
    assert rec["accuracy"] == ref["accuracy"].tolist() and rec["completeness"] == ref["completeness"].tolist() and rec["f1"] == ref["f1"].tolist()
    assert rec["ms_accuracy"] >= 0 and rec["ms_completeness"] >= 0
    return ref


@pytest.mark.parametrize("writers", ["binary_ascii", "rich_binary_rich_ascii", "rich_ascii_plain"])
def test_json_equals_the_numpy_counts(tool, clouds, tmp_path, writers):
    recon, gt = clouds
    a, b = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply")
    if writers == "binary_ascii":
        tio.write_ply(a, recon, binary=True)
        tio.write_ply(b, gt, binary=False)
    elif writers == "rich_binary_rich_ascii":
        write_rich_binary(a, recon)
        write_rich_ascii(b, gt)
    else:
        write_rich_ascii(a, recon)
        tio.write_ply(b, gt)
    tol = [0.01, 0.03, 0.1]
    out = run(tool, a, b, "--tolerances=0.01,0.03,0.1", "--json=" + str(tmp_path / "r.json"))
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["tolerance", "accuracy", "completeness", "f1", "n_accurate", "n_complete"] and len(lines) == 1 + len(tol) + 1
    rec = json.loads(lines[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read()) and rec["recon"] == a and rec["gt"] == b
    ref = check_record(rec, recon, gt, tol)
    assert 0 < ref["n_accurate"][0] < ref["n_accurate"][2] <= 499 and 0 < ref["n_complete"][0] < ref["n_complete"][2] < 699    # the case says something
    assert rec["pairs_accuracy"] == 499 * 699 and rec["pairs_completeness"] == 499 * 699              # the stand-in's brute force
    for k, row in enumerate(lines[1:-1]):
        assert int(row.split()[4]) == ref["n_accurate"][k] and int(row.split()[5]) == ref["n_complete"][k]


def test_the_readers_agree(clouds, tmp_path):
    """io.read_ply reads what the tool's reader is given above: the same three columns out of every layout"""
    recon, _ = clouds
    for k, write in enumerate((write_rich_binary, write_rich_ascii)):
        p = str(tmp_path / ("c%d.ply" % k))
        write(p, recon)
        assert np.array_equal(tio.read_ply(p).view(np.uint32), recon.view(np.uint32))


def test_empty_clouds(tool, tmp_path):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    tio.write_ply(a, np.zeros((0, 3), F))
    tio.write_ply(b, np.ones((4, 3), F), binary=False)
    out = run(tool, a, b, "--tolerances=0.5")
    rec = json.loads(out.stdout.splitlines()[-1])
    assert out.returncode == 0 and rec["accuracy"] == [0.0] and rec["completeness"] == [0.0] and rec["f1"] == [0.0] and rec["n_gt_valid"] == 4


def _ply(tmp_path, name, header, body):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(header + body)
    return p


@pytest.mark.parametrize("header,body,message", [
    (b"ply\nformat binary_big_endian 1.0\nelement vertex 1\n" + XYZ + b"end_header\n", b"\0" * 12, "format binary_big_endian is not supported (ascii and binary_little_endian are)"),
    (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty list uchar int k\nproperty float y\nproperty float z\nend_header\n", b"0 0 0 0\n",
     "a list property inside the vertex element"),
    (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n", b"0 0\n", "the vertex element has no property z"),
    (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty int y\nproperty float z\nend_header\n", b"0 0 0\n", "property y is neither float nor double"),
    (b"ply\nformat binary_little_endian 1.0\nelement vertex 1000000000000\n" + XYZ + b"end_header\n", b"\0" * 24, "the file holds fewer than 1000000000000 vertices"),
    (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\n" + XYZ + b"end_header\n", b"\0" * 30, "the file holds fewer than 3 vertices"),
    (b"ply\nformat ascii 1.0\nelement vertex 2\n" + XYZ + b"end_header\n", b"0 0 0\n1 1\n", "the file holds fewer than 2 vertices"),
    (b"ply\nformat ascii 1.0\nelement vertex 2\n" + XYZ, b"", "the header does not end"),
    (b"plx\n", b"", "not a PLY file"),
])
def test_ply_refusals(tool, tmp_path, header, body, message):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((2, 3), F))
    bad = _ply(tmp_path, "bad.ply", header, body)
    for args in ((bad, good), (good, bad)):
        out = run(tool, *args, "--tolerances=0.1")
        assert out.returncode != 0 and out.stdout == ""
        assert out.stderr == bad + ": " + message + "\n"


@pytest.mark.parametrize("args,message", [
    (["--tolerances="], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=0.1,"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=0.1;0.2"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=0.1,x"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=0.1,-1"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=0"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=inf"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    (["--tolerances=nan"], "--tolerances=T1[,T2...]: every tolerance must be a finite number > 0"),
    ([], "--tolerances=T1[,T2...] is required"),
    (["--tolerances=0.1", "--max_pairs=-3"], "--max_pairs=N must be an integer >= 0"),
    (["--tolerances=0.1", "--max_pairs=1e6"], "--max_pairs=N must be an integer >= 0"),
    (["--tolerances=0.1", "--device=x"], "--device=D must be an integer >= 0"),
    (["--tolerances=0.1", "--frobnicate"], "unknown option --frobnicate"),
])
def test_command_line_refusals(tool, tmp_path, args, message):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((2, 3), F))
    out = run(tool, good, good, *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message + "\n"


def test_a_missing_file_and_a_refused_call(tool, tmp_path):
    good = str(tmp_path / "good.ply")
    tio.write_ply(good, np.zeros((5, 3), F))
    out = run(tool, good, str(tmp_path / "none.ply"), "--tolerances=0.1")
    assert out.returncode != 0 and out.stderr == "cannot open " + str(tmp_path / "none.ply") + "\n"
    out = run(tool, good, good, "--tolerances=0.1", "--max_pairs=24")          # 5 x 5 pairs: the library's message is passed on
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "tsar_cloud_distance: more than max_pairs pairs\n"
    assert run(tool, good, good, "--tolerances=0.1", "--max_pairs=25").returncode == 0
    out = run(tool, good)
    assert out.returncode != 0 and out.stderr.startswith("usage: tsar_evaluate RECON.ply GT.ply --tolerances=")

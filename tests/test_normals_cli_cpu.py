"""tsar_evaluate --normals= on the CPU: host/tsar_evaluate.cpp linked against tests/cli_stub/tsar_stub_normals.cpp (the earlier stand-ins'
entries plus tsar_cloud_normals and tsar_cloud_normal_compare by brute force on the host).  Every integer field of the JSON record and every
float64 ratio equals the numpy restatement's (tests/cloud_normals_ref.py); without the switch the output is what the previous stand-in's tool
prints; every refusal gives one line and a non-zero exit; against a stand-in without the entries the tool refuses the switch in one line and
still runs without it; and the stand-in's normals equal the restatement's bit for bit: a third statement of the header."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cloud_normals_ref import cloud_normals_ref, evaluate_normals_ref, normal_compare_ref, stray_surface
from cloud_voxels_ref import evaluate_voxel_ref
from tsar_mvs_amd import api
from tsar_mvs_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tsar-mvs_amd", "host", "tsar_evaluate.cpp")
STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_normals.cpp")
OLD_STUB = os.path.join(ROOT, "tests", "cli_stub", "tsar_stub_neighbors.cpp")
F = np.float32


def build(d, stub):
    for cmd in (["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tests", "cli_stub"), "-o", d + "/libtsar_hip.so", stub],
                ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", d + "/tsar_evaluate", SRC, "-L" + d, "-ltsar_hip", "-lz", "-Wl,-rpath," + d]):
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    return d + "/tsar_evaluate"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_normals")), STUB)


@pytest.fixture(scope="module")
def old_tool(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("cli_stub_no_normals")), OLD_STUB)


def run(tool, *args):
    return subprocess.run([tool, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """every third point of the stray scene's surface with a perturbed analytic normal as RECON (a few records without a usable normal or
    position), another third as GT, which carries no normals"""
    d = tmp_path_factory.mktemp("normals_cli_clouds")
    pts, nrm = stray_surface()
    rng = np.random.default_rng(5)
    recon = np.zeros((1000, 6), F)
    recon[:, :3] = pts[::3]
    recon[:, 3:6] = nrm + rng.normal(scale=0.08, size=(1000, 3))
    recon[::2, 3:6] *= -1                                                 # half of them point the other way: lines agree, directions do not
    recon[5, 0] = np.nan
    recon[11, 2] = np.inf
    recon[20, 3:6] = 0
    recon[21, 4] = np.nan
    gt = pts[1::3].copy()
    a, b = str(d / "recon.ply"), str(d / "gt.ply")
    tio.write_ply(a, recon[:, :3], normals=recon[:, 3:6])
    tio.write_ply(b, gt)
    return recon, gt, a, b


CASES = [dict(k=16, radius=0.08), dict(k=8, radius=0.1, min_neighbors=4, tolerances_deg=(5.0, 10.0, 30.0, 90.0)), dict(k=16, radius=0.08, signed=True),
         dict(k=32, radius=0.005)]


def switches(nm):
    s = ["--normals=%d" % nm["k"], "--normal_radius=%.9g" % nm["radius"]]
    if "min_neighbors" in nm:
        s.append("--normal_min_neighbors=%d" % nm["min_neighbors"])
    if "tolerances_deg" in nm:
        s.append("--normal_tolerances=" + ",".join("%.17g" % v for v in nm["tolerances_deg"]))
    return s + (["--normal_signed"] if nm.get("signed") else [])


@pytest.mark.parametrize("nm", CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
@pytest.mark.parametrize("more", [{}, {"crop": (0.1, 0.0, 0.05, 0.9, 1.0, 0.8)}], ids=["plain", "crop"])
def test_json_equals_the_restatement(tool, files, tmp_path, nm, more):
    recon, gt, a, b = files
    tol = [0.01, 0.03]
    args = ["--tolerances=0.01,0.03", "--json=" + str(tmp_path / "r.json")] + switches(nm)
    if more:
        args.append("--crop=" + ",".join("%.9g" % v for v in more["crop"]))
    out = run(tool, a, b, *args)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rec = json.loads(out.stdout.splitlines()[-1])
    assert rec == json.loads(open(str(tmp_path / "r.json")).read())
    base = evaluate_voxel_ref(recon[:, :3], gt, tol, **more)              # what the record held before: unchanged by the switch
    for k in ("n_recon_valid", "n_gt_valid"):
        assert rec[k] == base[k], k
    for k in ("n_accurate", "n_complete", "accuracy", "completeness", "f1"):
        assert rec[k] == base[k].tolist(), k
    ref = evaluate_normals_ref(recon, gt, tol, nm, **more)
    for k in ("n_gt_normals", "n_normal_compared"):
        assert rec[k] == ref[k], k
    for k in ("normal_tolerances_deg", "n_normal_within", "normal_accuracy"):
        assert rec[k] == ref[k].tolist(), k                               # float64 for float64: %.17g names the double
    s = rec["normals"]
    assert list(s) == ["k", "radius", "min_neighbors", "signed"] and list(rec)[-6:] == ["normals", "normal_tolerances_deg", "n_gt_normals", "n_normal_compared",
                                                                                          "n_normal_within", "normal_accuracy"]
    assert (s["k"], F(s["radius"]), s["min_neighbors"], s["signed"]) == (nm["k"], F(nm["radius"]), nm.get("min_neighbors", 5), nm.get("signed", False))
    assert "not a benchmark's program" in out.stdout and "no orientation propagated" in out.stdout
    if nm["radius"] == 0.005:                                             # too small a radius: GT gets no normals, nothing is compared, the ratios are 0
        assert ref["n_gt_normals"] == 0 and rec["n_normal_compared"] == 0 and rec["normal_accuracy"] == [0.0, 0.0]
    elif nm.get("signed"):                                                # directions: the flipped half fails
        assert 0.3 < ref["normal_accuracy"][1] < 0.7
    else:                                                                 # the case says something: most lines agree within the widest angle, fewer within the first
        assert ref["n_normal_compared"] > 300 and ref["normal_accuracy"][-1] > 0.95 and ref["n_normal_within"][0] < ref["n_normal_within"][-1]


def test_without_the_switch_the_output_is_as_before(tool, old_tool, files):
    """the same record and table as the tool built against the previous stand-in, the two times apart; no new key.  RECON's extra properties
    are skipped by the reader the tool used before"""
    _, _, a, b = files
    outs = [run(t, a, b, "--tolerances=0.02,0.05") for t in (tool, old_tool)]
    assert all(o.returncode == 0 and o.stderr == "" for o in outs)
    recs = [json.loads(o.stdout.splitlines()[-1]) for o in outs]
    assert list(recs[0]) == ["recon", "gt", "n_recon", "n_gt", "n_recon_valid", "n_gt_valid", "tolerances", "n_accurate", "n_complete", "accuracy", "completeness",
                             "f1", "pairs_accuracy", "pairs_completeness", "ms_accuracy", "ms_completeness"]
    for r in recs:
        r.pop("ms_accuracy"), r.pop("ms_completeness")
    assert recs[0] == recs[1] and outs[0].stdout.splitlines()[:-1] == outs[1].stdout.splitlines()[:-1]


K_MSG = "--normals=K must be an integer in 3..32"
R_MSG = "--normal_radius=R must be a finite number > 0"
N_MSG = "--normal_min_neighbors=N must be an integer in 2..K"
T_MSG = "--normal_tolerances=D1[,D2...]: up to 16 angles in degrees, each a number in [0, 180]"
NEED_K = "--normal_radius=, --normal_min_neighbors=, --normal_tolerances= and --normal_signed need --normals=K"


@pytest.mark.parametrize("args,message", [
    (["--normals=2", "--normal_radius=0.1"], K_MSG), (["--normals=33", "--normal_radius=0.1"], K_MSG), (["--normals=", "--normal_radius=0.1"], K_MSG),
    (["--normals=8.5", "--normal_radius=0.1"], K_MSG), (["--normals=x", "--normal_radius=0.1"], K_MSG),
    (["--normals=8"], "--normals=K needs --normal_radius=R"),
    (["--normals=8", "--normal_radius=0"], R_MSG), (["--normals=8", "--normal_radius=-1"], R_MSG), (["--normals=8", "--normal_radius=inf"], R_MSG),
    (["--normals=8", "--normal_radius=nan"], R_MSG), (["--normals=8", "--normal_radius="], R_MSG), (["--normals=8", "--normal_radius=1e60"], R_MSG),
    (["--normals=8", "--normal_radius=1e-60"], R_MSG), (["--normals=8", "--normal_radius=0.1x"], R_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_min_neighbors=1"], N_MSG), (["--normals=8", "--normal_radius=0.1", "--normal_min_neighbors=9"], N_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_min_neighbors=x"], N_MSG), (["--normals=8", "--normal_radius=0.1", "--normal_min_neighbors=40"], N_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_tolerances="], T_MSG), (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=10,"], T_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=-1"], T_MSG), (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=10,181"], T_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=nan"], T_MSG), (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=10;20"], T_MSG),
    (["--normals=8", "--normal_radius=0.1", "--normal_tolerances=" + ",".join(["10"] * 17)], T_MSG),
    (["--normal_radius=0.1"], NEED_K), (["--normal_min_neighbors=3"], NEED_K), (["--normal_tolerances=10"], NEED_K), (["--normal_signed"], NEED_K),
])
def test_command_line_refusals(tool, files, args, message):
    _, _, a, b = files
    out = run(tool, a, b, "--tolerances=0.1", *args)
    assert out.returncode != 0 and out.stdout == "" and out.stderr == message + "\n"


def test_a_recon_without_normals_and_the_library_s_refusal_are_one_line(tool, files, tmp_path):
    _, _, a, b = files
    out = run(tool, b, b, "--tolerances=0.1", "--normals=8", "--normal_radius=0.1")                    # GT as RECON: it has no nx
    assert out.returncode != 0 and out.stdout == "" and out.stderr == b + ": the vertex element has no property nx\n"
    out = run(tool, a, b, "--tolerances=0.1", "--normals=8", "--normal_radius=1e-30")                  # R is a float32, R * R is not
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "tsar_cloud_normals: radius must be finite and > 0\n"


def test_a_library_without_the_entries_refuses_the_switch_in_one_line(old_tool, files):
    _, _, a, b = files
    out = run(old_tool, a, b, "--tolerances=0.05", "--normals=8", "--normal_radius=0.1")
    assert out.returncode != 0 and out.stdout == "" and out.stderr == "--normals: this libtsar_hip.so has no tsar_cloud_normals\n"
    assert run(old_tool, a, b, "--tolerances=0.05").returncode == 0


def test_the_stand_in_is_a_third_statement_of_the_header(tool):
    """its outputs against the restatement's, bit for bit: the three orientation modes, ties, duplicates, non-finite records, too few neighbours"""
    L = C.CDLL(os.path.join(os.path.dirname(tool), "libtsar_hip.so"))
    ctx = C.c_void_p()
    assert L.tsar_create(0, C.byref(ctx)) == 0
    rng = np.random.default_rng(6)
    pts, _ = stray_surface()
    cloud = np.zeros((700, 6), F)
    cloud[:500, :3] = pts[:500]
    cloud[500:600, :3] = rng.integers(0, 4, (100, 3))                     # a lattice with duplicates: ties
    cloud[600:, :3] = rng.random((100, 3))
    cloud[:, 3:6] = rng.normal(size=(700, 3))
    cloud[::40, 4] = np.nan
    cloud[3, 0], cloud[650, 2] = np.nan, -np.inf
    bits = lambda x: x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
    for k, mn, orient, R in ((16, 5, 0, 0.08), (8, 2, 1, 0.08), (32, 7, 2, 0.1), (3, 3, 0, 1.0), (17, 5, 2, 1.5)):
        ref = cloud_normals_ref(cloud, R, k, mn, orient, (0.5, 0.5, 3.0))
        p = api.CloudNormalsParams(R, k, mn, orient, (C.c_float * 3)(0.5, 0.5, 3.0), 1 << 40)
        out = {"knn_index": np.empty((700, k), np.int32), "n_used": np.empty(700, np.int32), "normal": np.empty((700, 3), F), "curvature": np.empty(700, F),
               "cov": np.empty((700, 6), np.float64)}
        cnt = [C.c_int64(-1) for _ in range(3)]
        rc = L.tsar_cloud_normals_ctx(ctx, cloud.ctypes.data_as(C.c_void_p), C.c_int64(700), 6, C.byref(p), *(v.ctypes.data_as(C.c_void_p) for v in out.values()),
                                      *(C.byref(c) for c in cnt), api.MEM_HOST)
        assert rc == 0 and (cnt[0].value, cnt[1].value) == (ref["n_valid"], ref["n_normals"]) and 100 < ref["n_normals"] <= 698
        for key, v in out.items():
            assert np.array_equal(bits(v), bits(ref[key])), (key, k, orient)
    a, b = cloud[:, 3:6].copy(), rng.normal(size=(50, 3)).astype(F)
    b[:3] = 0
    idx, d2 = rng.integers(-2, 52, 700).astype(np.int32), rng.random(700).astype(F)
    mc = np.cos(np.deg2rad(np.array([0.0, 20.0, 60.0, 90.0, 180.0])))
    for signed in (0, 1):
        ref = normal_compare_ref(a, b, idx, mc, d2, 0.7, bool(signed))
        cos, within, n_cmp = np.empty(700, F), np.empty(5, np.int64), C.c_int64(-1)
        rc = L.tsar_cloud_normal_compare_ctx(ctx, a.ctypes.data_as(C.c_void_p), 3, C.c_int64(700), b.ctypes.data_as(C.c_void_p), 3, C.c_int64(50), idx.ctypes.data_as(C.c_void_p),
                                             d2.ctypes.data_as(C.c_void_p), C.c_float(0.7), 5, mc.ctypes.data_as(C.c_void_p), signed, cos.ctypes.data_as(C.c_void_p),
                                             within.ctypes.data_as(C.c_void_p), C.byref(n_cmp), api.MEM_HOST)
        assert rc == 0 and n_cmp.value == ref["n_compared"] > 100 and within.tolist() == ref["within"].tolist() and np.array_equal(bits(cos), bits(ref["cos"]))
    L.tsar_destroy(ctx)

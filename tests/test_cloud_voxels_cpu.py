"""The numpy restatement of tsar_cloud_voxels (tests/cloud_voxels_ref.py) against answers known by hand, the density case that tells the
voxel-averaged accuracy from the point-wise one, and the code objects of csrc/cloud_voxel_kernels.hip: no scratch, few registers."""
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_voxels_ref import cloud_voxels_ref, crop_ref, density_case, evaluate_voxel_ref, voxel_share

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_4x4x1_lattice_of_cells_with_hand_placed_points():
    """V = 1, the origin is a point at (0, 0, 0); every cell (x, y) holds an off-centre point and then its centre; voxel number = 4 y + x"""
    pts = [[0.0, 0.0, 0.0]]
    for y in range(4):
        for x in range(4):
            pts += [[x + 0.25, y + 0.5, 0.5], [x + 0.5, y + 0.5, 0.5]]
    r = cloud_voxels_ref(np.array(pts, F), 1.0)
    assert r["n_voxels"] == 16 and r["n_valid"] == 33
    assert r["keys"].tolist() == [(y << 21) | x for y in range(4) for x in range(4)]
    assert r["count"].tolist() == [3] + [2] * 15
    assert r["rep"].tolist() == [2 + 2 * v for v in range(16)]                       # the centre points: d2f = 0
    assert r["rank"].tolist() == [0] + [v for v in range(16) for _ in range(2)]
    assert r["d2f"][1] == F(0.0625) and r["d2f"][0] == F(0.75) and r["d2f"][2] == 0
    # a second layer in z: the z field is the most significant
    up = np.array(pts, F) + np.array([0, 0, 1], F)
    r = cloud_voxels_ref(np.concatenate([np.array(pts, F), up[1:]]), 1.0)
    assert r["n_voxels"] == 32 and r["keys"][16:].tolist() == [(1 << 42) | (y << 21) | x for y in range(4) for x in range(4)]
    assert r["rank"][33:].tolist() == [16 + v for v in range(16) for _ in range(2)]


def test_two_points_symmetric_about_a_centre_the_smaller_index_wins():
    a, b = [0.25, 0.5, 0.5], [0.75, 0.5, 0.5]
    for pts, want in (([[0, 0, 0], a, b], 1), ([[0, 0, 0], b, a], 1), ([a, [0, 0, 0], b], 0), ([b, a, [0, 0, 0]], 0)):
        r = cloud_voxels_ref(np.array(pts, F), 1.0)
        assert r["n_voxels"] == 1 and r["rep"].tolist() == [want] and r["count"].tolist() == [3]


def test_duplicates():
    p = [0.5, 0.5, 0.5]
    r = cloud_voxels_ref(np.array([[0, 0, 0], [1.5, 0.5, 0.5], p, p, p, [1.5, 0.5, 0.5]], F), 1.0)
    assert r["rep"].tolist() == [2, 1] and r["count"].tolist() == [4, 2] and r["rank"].tolist() == [0, 1, 0, 0, 0, 1]


def test_a_point_on_a_cell_face_and_its_float32_neighbours():
    face = F(0.5)                                                                      # V = 0.25: the face between cells 1 and 2
    below, above = np.nextafter(face, F(0)), np.nextafter(face, F(1))
    pts = np.array([[0, 0, 0], [below, 0, 0], [face, 0, 0], [above, 0, 0]], F)
    r = cloud_voxels_ref(pts, 0.25)
    assert r["keys"].tolist() == [0, 1, 2] and r["rank"].tolist() == [0, 1, 2, 2] and r["count"].tolist() == [1, 1, 2]
    assert r["rep"].tolist() == [0, 1, 3]                                              # `above` is the nearer to the centre 0.625 of cell 2
    # an origin that is no multiple of V: the cells follow the origin
    pts = np.array([[0.125, 0, 0], [0.375, 0, 0], [np.nextafter(F(0.375), F(0)), 0, 0], [0.625, 0, 0]], F)     # faces at 0.125 + 0.25 k
    r = cloud_voxels_ref(pts, 0.25)
    assert r["rank"].tolist() == [0, 1, 0, 2] and r["keys"].tolist() == [0, 1, 2]


def test_non_finite_records_take_no_part():
    pts = np.array([[np.nan, 0, 0], [0, 0, 0], [0.5, np.inf, 0], [1.5, 0, 0], [0, 0, -np.inf], [-7, np.nan, 3]], F)
    r = cloud_voxels_ref(pts, 1.0, dist2=np.array([0, 0, 0, np.nan, 0, 0], F), tolerances=[0.5])
    assert r["n_valid"] == 2 and r["n_voxels"] == 2 and r["rank"].tolist() == [-1, 0, -1, 1, -1, -1] and r["rep"].tolist() == [1, 3]
    assert r["within"].tolist() == [[1], [0]]                                          # a NaN dist2 never passes
    r = cloud_voxels_ref(np.full((5, 3), np.nan, F), 1.0, dist2=np.zeros(5, F), tolerances=[1.0, 2.0])
    assert r["n_voxels"] == 0 and r["n_valid"] == 0 and r["within"].shape == (0, 2) and (r["rank"] == -1).all()
    assert cloud_voxels_ref(np.zeros((0, 3), F), 1.0)["n_voxels"] == 0


def test_within_counts_per_voxel_and_tolerance():
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [1.5, 0, 0], [1.25, 0, 0], [0.75, 0, 0]], F)
    d2 = np.array([0.0, 0.01, np.inf, 0.04, F(0.1) * F(0.1)], F)
    r = cloud_voxels_ref(pts, 1.0, dist2=d2, tolerances=[0.1, 0.2, 0.05])
    assert r["within"].tolist() == [[3, 3, 1], [0, 1, 0]]                              # dist2 == fl(tol * tol) passes; +inf never
    assert voxel_share(r["within"], r["count"]).tolist() == [(1.0 + 0.0) / 2, (1.0 + 0.5) / 2, (1.0 / 3.0 + 0.0) / 2]


def test_the_share_is_a_sequential_sum():
    """thirds do not add exactly: the definition is the left-to-right float64 sum, which np.sum (pairwise) does not give for long arrays"""
    rng = np.random.default_rng(1)
    count = rng.integers(1, 50, size=5000)
    within = (rng.random(5000) * (count + 1)).astype(np.int64).clip(0, count)[:, None]
    s = 0.0
    for w, c in zip(within[:, 0].tolist(), count.tolist()):
        s += w / c
    assert voxel_share(within, count).tolist() == [s / 5000]


def test_the_density_case_point_wise_one_eleventh_voxel_averaged_one_half():
    recon, gt, tau, voxel = density_case()
    r = evaluate_voxel_ref(recon, gt, [tau], voxel=voxel)
    assert r["n_recon_valid"] == 352 and r["n_accurate"].tolist() == [32]
    assert r["accuracy"].tolist() == [32 / 352] and abs(r["accuracy"][0] - 1 / 11) < 1e-16
    assert r["n_recon_voxels"] == 64 and r["accuracy_voxel"].tolist() == [0.5]        # exactly
    assert r["n_gt_voxels"] == 64 and r["completeness"].tolist() == [0.5] and r["completeness_voxel"].tolist() == [0.5] and r["f1_voxel"].tolist() == [0.5]
    v = r["recon_voxels"]
    want_rank = [8 * y + x for y in range(8) for x in range(4) for _ in range(10)] + [8 * y + x for y in range(8) for x in range(4, 8)]
    assert v["rank"].tolist() == want_rank
    assert v["count"].reshape(8, 8).tolist() == [[10] * 4 + [1] * 4] * 8 and v["within"].reshape(8, 8).tolist() == [[0] * 4 + [1] * 4] * 8
    # a crop to the sparse half: every figure is 1
    r = evaluate_voxel_ref(recon, gt, [tau], voxel=voxel, crop=(4, 0, -1, 8, 8, 1))
    assert (r["n_recon_cropped"], r["n_gt_cropped"]) == (320, 32) and r["n_recon_valid"] == 32
    assert r["accuracy"].tolist() == [1.0] and r["accuracy_voxel"].tolist() == [1.0] and r["completeness_voxel"].tolist() == [1.0] and r["n_recon_voxels"] == 32


def test_the_crop_box_is_closed_and_skips_non_candidates():
    c = np.array([[0, 0, 0], [1, 1, 1], [1.0000001, 1, 1], [np.nan, 0, 0], [0.5, 0.5, np.inf], [-0.0, 0, 0]], F)
    out, removed = crop_ref(c, (0, 0, 0, 1, 1, 1))
    assert removed == 1 and np.isnan(out[2, :3]).all() and np.isnan(out[3:5, :3]).all() and np.array_equal(out[[0, 1, 5]], c[[0, 1, 5]])


# ---- the kernels' code objects ----------------------------------------------------------------------------------------------------------
def test_voxel_kernels_use_no_scratch_and_the_reduce_kernel_few_registers(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    src = os.path.join(ROOT, "tsar-mvs_amd", "csrc", "cloud_voxel_kernels.hip")
    out = str(tmp_path / "cv.s")
    try:
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S",
                        src, "-o", out], check=True, capture_output=True, timeout=900)
    except FileNotFoundError:
        pytest.skip("hipcc not available")
    txt = open(out).read()
    meta = {}
    for block in txt.split("  - .agpr_count")[1:]:                                     # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if re.search(r"cv_\w+_kernel", name):                                          # (the file also instantiates rocPRIM's sort and scan kernels)
            meta[re.search(r"cv_\w+_kernel", name).group(0)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                                                                for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")}
    assert set(meta) >= {"cv_keys_kernel", "cv_heads_kernel", "cv_reduce_kernel", "cv_finish_kernel"}, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
    assert meta["cv_reduce_kernel"]["vgpr_count"] <= 64, meta["cv_reduce_kernel"]

"""cloud_distance_ref (tests/cloud_distance_ref.py), the numpy restatement the GPU operator is held to bit for bit, against known answers;
the float64 cell function of include/tsar.h on adversarial pairs: every pair the float32 d2 keeps differs by at most 1 per cell coordinate,
which is what lets the 27-cell search stand for the brute-force definition; io.read_ply / write_ply round trips."""
import numpy as np
import pytest

from cloud_distance_ref import candidates, cell_coords, cell_edge, cloud_distance_ref, grid_of, pairs_ref
from tsar_mvs_amd import io as tio

F = np.float32


def test_identical_clouds_give_zero_and_the_identity():
    rng = np.random.default_rng(1)
    a = rng.random((500, 3), dtype=F)
    r = cloud_distance_ref(a, a, 0.5, [0.25, 0.5])
    assert np.array_equal(r["dist2"], np.zeros(500, F)) and np.array_equal(r["index"], np.arange(500))
    assert r["within"].tolist() == [500, 500] and r["n_valid_query"] == 500


def test_duplicated_targets_give_the_smallest_index():
    t = np.array([[5, 5, 5], [1, 2, 3], [0, 0, 0], [1, 2, 3], [1, 2, 3]], F)
    q = np.array([[1, 2, 3.5], [0, 0, 0.25]], F)
    r = cloud_distance_ref(q, t, 1.0)
    assert r["index"].tolist() == [1, 2] and r["dist2"].tolist() == [0.25, 0.0625]
    # an equal distance to two different points: still the smaller index
    r = cloud_distance_ref(np.array([[0, 0, 0]], F), np.array([[9, 9, 9], [0, 1, 0], [1, 0, 0]], F), 2.0)
    assert r["index"].tolist() == [1] and r["dist2"].tolist() == [1.0]


@pytest.mark.parametrize("R", [0.1, 0.3, 1.7, 3.0])
def test_the_radius_itself_is_kept_and_the_next_float_is_not(R):
    r32 = F(R)
    r2 = F(r32 * r32)
    # a target at distance d along x has d2 = fl(d * d): find d with fl(d * d) == r2, and the smallest d' with fl(d' * d') > r2
    d = r32
    while F(d * d) <= r2:
        d = np.nextafter(d, F(np.inf))
    above = d
    at = np.nextafter(above, F(0))
    assert F(at * at) == r2 and F(above * above) > r2
    q = np.zeros((1, 3), F)
    kept = cloud_distance_ref(q, np.array([[at, 0, 0]], F), R, [R])
    assert kept["index"].tolist() == [0] and kept["dist2"][0] == r2 and kept["within"].tolist() == [1]
    dropped = cloud_distance_ref(q, np.array([[above, 0, 0]], F), R, [R])
    assert dropped["index"].tolist() == [-1] and np.isposinf(dropped["dist2"][0]) and dropped["within"].tolist() == [0]


def test_non_finite_records_take_no_part():
    t = np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, np.inf, 0], [0.2, 0, 0], [0, 0, -np.inf]], F)
    q = np.array([[0.19, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.01, 0, 0]], F)
    r = cloud_distance_ref(q, t, 1.0, [0.05, 1.0])
    assert r["index"].tolist() == [3, -1, -1, 0] and r["n_valid_query"] == 2
    assert np.isposinf(r["dist2"][1:3]).all() and r["within"].tolist() == [2, 2]
    assert candidates(t).tolist() == [True, False, False, True, False]
    assert pairs_ref(q, t, 1.0) == 4


def test_empty_sides():
    q = np.random.default_rng(2).random((7, 3), dtype=F)
    r = cloud_distance_ref(q, np.zeros((0, 3), F), 1.0, [0.5])
    assert r["index"].tolist() == [-1] * 7 and np.isposinf(r["dist2"]).all() and r["within"].tolist() == [0] and r["n_valid_query"] == 7
    r = cloud_distance_ref(np.zeros((0, 3), F), q, 1.0, [0.5])
    assert r["dist2"].shape == (0,) and r["index"].shape == (0,) and r["within"].tolist() == [0] and r["n_valid_query"] == 0
    assert pairs_ref(q, np.zeros((0, 3), F), 1.0) == 0 and pairs_ref(np.zeros((0, 3), F), q, 1.0) == 0
    assert grid_of(np.full((3, 3), np.nan, F), 1.0) is None


def test_a_tolerance_equal_to_the_radius_counts_every_hit():
    rng = np.random.default_rng(3)
    q, t = rng.random((400, 3), dtype=F), rng.random((300, 3), dtype=F)
    r = cloud_distance_ref(q, t, 0.07, [0.07, 0.035])
    assert r["within"][0] == np.count_nonzero(r["index"] >= 0) and 0 < r["within"][1] < r["within"][0] < 400


def test_strided_records_and_chunking_change_nothing():
    rng = np.random.default_rng(4)
    q, t = rng.random((300, 9), dtype=F), rng.random((200, 4), dtype=F)
    a = cloud_distance_ref(q, t, 0.1, [0.05])
    b = cloud_distance_ref(q[:, :3], t[:, :3], 0.1, [0.05], chunk_elems=1000)
    assert np.array_equal(a["dist2"], b["dist2"]) and np.array_equal(a["index"], b["index"]) and a["within"].tolist() == b["within"].tolist()


def test_agrees_with_ckdtree_in_float64():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    q, t = rng.random((2000, 3), dtype=F), rng.random((1500, 3), dtype=F)       # random points: no near-ties
    R = 0.08
    r = cloud_distance_ref(q, t, R)
    d, j = spatial.cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=1, distance_upper_bound=R)
    hit = np.isfinite(d)
    margin = np.abs(d - R) > 1e-5 * R                                            # a pair on the radius itself may fall either side
    assert np.array_equal((r["index"] >= 0)[margin], hit[margin])
    both = hit & (r["index"] >= 0)
    assert np.array_equal(r["index"][both], j[both])
    assert np.allclose(np.sqrt(r["dist2"][both].astype(np.float64)), d[both], rtol=1e-6, atol=0)


# ---- the cell function ---------------------------------------------------------------------------------------------------------------------
def _kept(q, t, R):
    """the pairs (q[k], t[k]) whose float32 d2 is <= fl(R * R)"""
    r32 = F(R)
    dx, dy, dz = q[:, 0] - t[:, 0], q[:, 1] - t[:, 1], q[:, 2] - t[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F
    return d2 <= F(r32 * r32)


def _assert_neighbouring(q, t, origin, R, least):
    keep = _kept(q, t, R)
    assert np.count_nonzero(keep) >= least, "the construction must produce kept pairs"
    assert (t >= origin[None, :]).all(), "the origin is the targets' per-axis minimum"
    diff = np.abs(cell_coords(q[keep], origin, R) - cell_coords(t[keep], origin, R))
    assert diff.max() <= 1, "a kept pair lies outside the 27 cells: max cell difference %g" % diff.max()


@pytest.mark.parametrize("R", [0.01, 0.37, 1.0, 3.3])
@pytest.mark.parametrize("max_cell", [10, 4000, 900000])
def test_kept_pairs_differ_by_at_most_one_cell(R, max_cell):
    """targets just below and just above a cell border, queries at R (1 +- 2^-k), k = 10 .. 26, along an axis and along random directions"""
    rng = np.random.default_rng(int(R * 1000) + max_cell)
    e = cell_edge(R)
    origin = np.array([-3.25, 0.0, 17.5], F) * F(R)
    n = 20000
    cells = rng.integers(1, max_cell, size=(n, 3)).astype(np.float64)
    k = rng.integers(10, 27, size=n)
    sign = rng.choice([-1.0, 1.0], size=n)
    dist = np.float64(F(R)) * (1.0 + sign * 2.0 ** -k)
    for along_axis in (True, False):
        if along_axis:
            u = np.zeros((n, 3))
            u[np.arange(n), rng.integers(0, 3, size=n)] = rng.choice([-1.0, 1.0], size=n)
        else:
            u = rng.normal(size=(n, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
        # the target sits within a few float32 steps of a border of its cell, on either side of it
        border = origin.astype(np.float64)[None, :] + cells * e
        t = (border * (1.0 + rng.integers(-3, 4, size=(n, 3)) * 2.0 ** -24)).astype(F)
        t = np.maximum(t, origin[None, :])
        q = (t.astype(np.float64) + u * dist[:, None]).astype(F)
        _assert_neighbouring(q, t, origin, R, least=n // 8)


@pytest.mark.parametrize("R", [0.01, 0.37, 3.3])
def test_coordinates_that_are_multiples_of_the_cell_edge(R):
    rng = np.random.default_rng(7)
    e = cell_edge(R)
    origin = np.zeros(3, F)
    n = 20000
    t = (rng.integers(0, 900000, size=(n, 3)) * e).astype(F)
    step = rng.integers(-1, 2, size=(n, 3)) * rng.choice([0.0, 1.0], size=(n, 3), p=[0.6, 0.4])
    scale = 1.0 - 2.0 ** -rng.integers(10, 27, size=(n, 1)).astype(np.float64)
    q = (t.astype(np.float64) + step * np.float64(F(R)) * scale / np.maximum(np.linalg.norm(step, axis=1, keepdims=True), 1.0)).astype(F)
    _assert_neighbouring(q, t, origin, R, least=n // 8)


def test_pairs_ref_counts_the_27_cells():
    # a 3 x 3 x 3 block of cells around the query's cell, one target per cell, and one target two cells away
    R = 1.0
    e = cell_edge(R)
    centres = np.array([[x, y, z] for z in range(5) for y in range(5) for x in range(5)], np.float64) * e + 0.5 * e
    t = centres.astype(F)
    assert pairs_ref(np.array([[2.5 * e] * 3], F), t, R) == 27
    assert pairs_ref(np.array([[0.5 * e] * 3], F), t, R) == 8                   # a corner cell of the grid has 8 cells around it
    assert pairs_ref(np.array([[-0.5 * e, 0.5 * e, 0.5 * e]], F), t, R) == 4    # one cell outside the grid
    assert pairs_ref(np.array([[-1.5 * e, 0.5 * e, 0.5 * e]], F), t, R) == 0    # two cells outside
    assert pairs_ref(np.array([[1e30, 0, 0], [np.nan, 0, 0]], F), t, R) == 0


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip(tmp_path, binary):
    rng = np.random.default_rng(8)
    a = (rng.normal(size=(257, 5)) * 100).astype(F)
    a[3, :3] = [np.nan, np.inf, -np.inf]
    p = str(tmp_path / "c.ply")
    tio.write_ply(p, a, binary=binary)
    b = tio.read_ply(p)
    assert b.dtype == F and b.shape == (257, 3) and np.array_equal(b.view(np.uint32)[4:], a[4:, :3].copy().view(np.uint32))
    assert np.isnan(b[3, 0]) and np.isposinf(b[3, 1]) and np.isneginf(b[3, 2])


def test_ply_with_extra_properties_doubles_and_faces(tmp_path):
    p = str(tmp_path / "d.ply")
    rec = np.zeros(3, np.dtype([("red", "u1"), ("z", "<f8"), ("x", "<f4"), ("nx", "<f4"), ("y", "<f8")]))
    rec["x"], rec["y"], rec["z"] = [1, 2, 3], [0.1, 0.2, 0.3], [1e-3, 1 / 3, 7]
    with open(p, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex 3\nproperty uchar red\nproperty double z\nproperty float x\n"
                b"property float nx\nproperty double y\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
        f.write(rec.tobytes() + bytes([3, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0]))
    b = tio.read_ply(p)
    assert np.array_equal(b, np.stack([rec["x"], rec["y"].astype(F), rec["z"].astype(F)], axis=1))


@pytest.mark.parametrize("header,body,message", [
    (b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n", b"\0" * 12, "not supported"),
    (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty list uchar int k\nproperty float y\nproperty float z\nend_header\n", b"0 0 0 0\n", "list property"),
    (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n", b"0 0\n", "no property z"),
    (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n", b"\0" * 30, "fewer than 3 vertices"),
    (b"ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n", b"0 0 0\n1 1\n", "fewer than 2 vertices"),
])
def test_read_ply_refusals(tmp_path, header, body, message):
    p = str(tmp_path / "bad.ply")
    with open(p, "wb") as f:
        f.write(header + body)
    with pytest.raises(ValueError, match=message):
        tio.read_ply(p)

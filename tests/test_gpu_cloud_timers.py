"""The timer names include/tsar.h promises for the cloud operators, and the number of launches each entry records under them: one context
with kernel timing on, every entry called once on one small cloud, the context's record read after each call and held to the table below.
No output decides which name a launch is timed under, so nothing else notices a launch that moves to another name, is timed twice or not at
all.  Also: the max_pairs and max_splats refusals carry the refused entry's own name and wording, and a refused call has timed only what ran
before the refusal.

The cloud: 257 records (a partial last block of 256 lanes), one of them with a NaN coordinate (so the fill kernels of the two searches
run), in front of a camera of 65 x 33 pixels."""
import numpy as np
import pytest

from tsar_mvs_amd import api

pytestmark = pytest.mark.gpu
F = np.float32
N, W, H = 257, 65, 33
K = np.array([[60, 0, 32], [0, 60, 16], [0, 0, 1]], F)
R = np.eye(3, dtype=F)
T = np.zeros(3, F)
RADIUS = 0.5                                  # of the two searches: tens of neighbours per point
FOOT = 0.05                                   # of the renders: a footprint of one pixel around the landing (60 * 0.05 / z, z in 4..6)

GRID = {"cloud_bounds": 1, "cloud_keys": 1, "cloud_sort": 1, "cloud_gather": 1, "cloud_pairs": 1}      # what a search's prelude records
SQUARE3 = {"cloud_render_count": 1, "cloud_render_scatter": 1, "cloud_render_resolve": 1}              # min_points 1, no count_out: no support pass
SQUARE4 = dict(SQUARE3, cloud_render_support=1)
SPLAT3 = {"cloud_splat_count": 1, "cloud_splat_scatter": 1, "cloud_splat_resolve": 1}
SPLAT4 = dict(SPLAT3, cloud_splat_support=1)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    cloud = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-0.8, 0.8, N), rng.uniform(4.0, 6.0, N)], 1).astype(F)
    cloud[100, 1] = np.nan
    normals = rng.normal(size=(N, 3)).astype(F)
    return cloud, normals


@pytest.fixture(scope="module")
def matcher():
    m = api.Matcher()
    m.enable_kernel_timing(True)
    yield m
    m.close()


def launches(m, call):
    """name -> launches recorded by call()"""
    m.reset_kernel_timing()
    call()
    return {name: n for name, (n, _) in m.kernel_timing().items()}


def test_every_cloud_entry_is_timed_under_its_own_names(matcher, data):
    m = matcher
    cloud, normals = data
    index = np.arange(N, dtype=np.int32)
    render = lambda **kw: api.cloud_render(cloud, K, R, T, W, H, matcher=m, **kw)
    depth = render(want=("depth",))["depth"]
    table = [
        # (the fill kernel and the search kernel are two launches under the entry's name)
        ("neighbors k=0", lambda: api.cloud_neighbors(cloud, RADIUS, k=0, want=("count",), matcher=m), dict(GRID, cloud_neighbors=2)),
        ("neighbors k=8", lambda: api.cloud_neighbors(cloud, RADIUS, k=8, matcher=m), dict(GRID, cloud_neighbors=2)),
        ("normals", lambda: api.cloud_normals(cloud, RADIUS, k=8, min_neighbors=3, matcher=m), dict(GRID, cloud_normals=2)),
        ("normal_compare", lambda: api.normal_compare(normals, normals, index, (10.0, 30.0), matcher=m), {"cloud_normal_compare": 1}),
        ("render radius 0", lambda: render(want=("depth",)), SQUARE3),
        ("render radius 0, count", lambda: render(want=("depth", "count")), SQUARE4),
        ("render radius > 0", lambda: render(radius=FOOT, want=("depth", "index")), SQUARE3),
        ("render radius > 0, count", lambda: render(radius=FOOT, want=("depth", "count")), SQUARE4),
        ("oriented", lambda: render(radius=FOOT, normals=normals, want=("depth", "occluder")), SPLAT3),
        ("oriented, count", lambda: render(radius=FOOT, normals=normals, want=("depth", "count", "index", "occluder")), SPLAT4),
        ("depth_compare", lambda: api.depth_compare(depth, depth, (0.01, 0.1), matcher=m), {"depth_compare": 1}),
    ]
    for what, call, expected in table:
        got = launches(m, call)
        print(what, got)
        assert got == expected, what


def test_refusals_name_their_entry_and_time_only_what_ran(matcher, data):
    m = matcher
    cloud, normals = data
    pairs = api.cloud_neighbors(cloud, RADIUS, k=0, want=("count",), matcher=m)["pairs"]
    assert pairs == api.cloud_normals(cloud, RADIUS, k=8, min_neighbors=3, matcher=m)["pairs"] and pairs > 1
    splats = api.cloud_render(cloud, K, R, T, W, H, radius=FOOT, matcher=m)["n_splats"]
    assert splats == api.cloud_render(cloud, K, R, T, W, H, radius=FOOT, normals=normals, matcher=m)["n_splats"] and splats > 1
    refused = [
        (lambda: api.cloud_neighbors(cloud, RADIUS, k=4, max_pairs=pairs - 1, matcher=m), GRID,
         "tsar_cloud_neighbors: the call would look at %d pairs, more than max_pairs = %d: lower radius or raise max_pairs" % (pairs, pairs - 1)),
        (lambda: api.cloud_normals(cloud, RADIUS, k=8, min_neighbors=3, max_pairs=pairs - 1, matcher=m), GRID,
         "tsar_cloud_normals: the call would look at %d pairs, more than max_pairs = %d: lower radius or raise max_pairs" % (pairs, pairs - 1)),
        (lambda: api.cloud_render(cloud, K, R, T, W, H, radius=FOOT, max_splats=splats - 1, matcher=m), {"cloud_render_count": 1},
         "tsar_cloud_render: the call would issue %d footprint atomics, more than max_splats = %d: lower radius or max_px, or raise max_splats"
         % (splats, splats - 1)),
        (lambda: api.cloud_render(cloud, K, R, T, W, H, radius=FOOT, normals=normals, max_splats=splats - 1, matcher=m), {"cloud_splat_count": 1},
         "tsar_cloud_render_oriented: the call would examine %d footprint pixels, more than max_splats = %d: lower radius or max_px, or raise max_splats"
         % (splats, splats - 1)),
    ]
    for call, expected, text in refused:
        m.reset_kernel_timing()
        with pytest.raises(api.TsarError) as e:
            call()
        assert str(e.value).endswith(": " + text), str(e.value)
        assert {name: n for name, (n, _) in m.kernel_timing().items()} == expected, text

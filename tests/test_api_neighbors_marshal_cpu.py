"""api.cloud_neighbors / api.remove_outliers / api.evaluate_cloud(clean=) without a GPU: the library is replaced by a recorder that notes
every argument of tsar_cloud_neighbors_ctx in order and fills the outputs from the numpy restatement.  Holds the argument order and the
None handling of the binding, and the host path of the outlier rules (np.partition, the two float32 products) to the restatement."""
import ctypes as C

import numpy as np
import pytest

from cloud_neighbors_ref import cloud_neighbors_ref, remove_outliers_ref, stray_scene
from tsar_mvs_amd import api

F = np.float32


class Recorder:
    """stands for libtsar_hip.so: the two entries cloud_neighbors calls"""

    def __init__(self, rc=api.TSAR_OK, pairs=None):
        self.calls, self.rc, self.pairs = [], rc, pairs

    def tsar_default_cloud_neighbors_params(self, ref):
        p = ref._obj
        p.radius, p.k, p.max_pairs = 0.0, 0, 1 << 40

    def tsar_cloud_neighbors_ctx(self, ctx, cloud, n, stride, p, count, knn, n_valid, pairs, mem):
        p = p._obj
        self.calls.append(dict(ctx=ctx, cloud=cloud, n=n, stride=stride, radius=p.radius, k=p.k, max_pairs=p.max_pairs, count=count, knn=knn, mem=mem))
        if self.pairs is not None:
            pairs._obj.value = self.pairs
        if self.rc != api.TSAR_OK:
            return self.rc
        pts = np.ctypeslib.as_array(C.cast(cloud, C.POINTER(C.c_float)), (n, stride)) if n else np.zeros((0, stride), F)
        ref = cloud_neighbors_ref(pts, p.radius, p.k)
        if count is not None and n:
            np.ctypeslib.as_array(C.cast(count, C.POINTER(C.c_int32)), (n,))[:] = ref["count"]
        if knn is not None and n:
            np.ctypeslib.as_array(C.cast(knn, C.POINTER(C.c_float)), (n, p.k))[:] = ref["knn_dist2"]
        n_valid._obj.value, pairs._obj.value = ref["n_valid"], ref["pairs"]
        return api.TSAR_OK

    def tsar_last_error(self, ctx):
        return b"the recorder's refusal"


class FakeMatcher:
    _ctx = "the context"


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(api, "load_library", lambda *a: rec)
    return rec


def test_argument_order_and_defaults(lib):
    cloud = np.arange(45, dtype=F).reshape(5, 9)
    res = api.cloud_neighbors(cloud, 20.0, k=3, matcher=FakeMatcher())
    (c,) = lib.calls
    assert c["ctx"] == "the context" and c["cloud"].value == cloud.ctypes.data and (c["n"], c["stride"]) == (5, 9)
    assert (c["radius"], c["k"], c["max_pairs"], c["mem"]) == (20.0, 3, 1 << 40, api.MEM_HOST)
    assert c["count"].value == res["count"].ctypes.data and c["knn"].value == res["knn_dist2"].ctypes.data
    ref = cloud_neighbors_ref(cloud, 20.0, 3)
    assert res["count"].dtype == np.int32 and res["knn_dist2"].dtype == F and res["knn_dist2"].shape == (5, 3)
    assert np.array_equal(res["count"], ref["count"]) and np.array_equal(res["knn_dist2"].view(np.uint32), ref["knn_dist2"].view(np.uint32))
    assert res["n_valid"] == 5 and res["pairs"] == ref["pairs"]


def test_unwanted_outputs_and_k_zero_are_null_pointers(lib):
    cloud = np.zeros((4, 3), F)
    res = api.cloud_neighbors(cloud, 1.0, k=0, max_pairs=77, matcher=FakeMatcher())
    assert lib.calls[-1]["knn"] is None and lib.calls[-1]["count"] is not None and lib.calls[-1]["max_pairs"] == 77 and "knn_dist2" not in res
    res = api.cloud_neighbors(cloud, 1.0, k=2, want=("knn_dist2",), matcher=FakeMatcher())
    assert lib.calls[-1]["count"] is None and lib.calls[-1]["knn"] is not None and "count" not in res
    res = api.cloud_neighbors(cloud, 1.0, k=2, want=(), matcher=FakeMatcher())
    assert lib.calls[-1]["count"] is None and lib.calls[-1]["knn"] is None and set(res) == {"n_valid", "pairs"}
    res = api.cloud_neighbors(np.zeros((0, 3), F), 1.0, k=2, matcher=FakeMatcher())          # an empty cloud goes in as NULL
    assert lib.calls[-1]["cloud"] is None and lib.calls[-1]["n"] == 0 and res["knn_dist2"].shape == (0, 2)
    api.cloud_neighbors(np.zeros((2, 3)), 1.0, matcher=FakeMatcher())                         # float64 goes through one float32 copy
    assert lib.calls[-1]["stride"] == 3


def test_a_refusal_carries_the_pairs(monkeypatch):
    rec = Recorder(rc=api.TSAR_ERR_INVALID, pairs=1234)
    monkeypatch.setattr(api, "load_library", lambda *a: rec)
    with pytest.raises(api.TsarError) as e:
        api.cloud_neighbors(np.zeros((2, 3), F), 1.0, max_pairs=5, matcher=FakeMatcher())
    assert e.value.pairs == 1234 and "the recorder's refusal" in str(e.value)
    rec.pairs = None
    with pytest.raises(api.TsarError) as e:
        api.cloud_neighbors(np.zeros((2, 3), F), 1.0, matcher=FakeMatcher())
    assert e.value.pairs is None


@pytest.mark.parametrize("rules", [dict(min_neighbors=6), dict(k=8), dict(k=8, ratio=1.25), dict(min_neighbors=3, k=4, ratio=3.0), dict(k=1, ratio=1.6)])
def test_remove_outliers_on_the_host_equals_the_restatement(lib, rules):
    cloud = np.concatenate([stray_scene()[::4], np.arange(800, dtype=F)[:, None]], axis=1)   # [800, 4]: a fourth column rides along
    cloud[3, 1] = np.nan
    rows, keep = api.remove_outliers(cloud, 0.12, return_mask=True, matcher=FakeMatcher(), **rules)
    ref_rows, ref_keep = remove_outliers_ref(cloud, 0.12, **rules)
    assert keep.dtype == bool and np.array_equal(keep, ref_keep) and np.array_equal(rows, ref_rows) and 0 < keep.sum() < 799
    assert np.array_equal(api.remove_outliers(cloud, 0.12, matcher=FakeMatcher(), **rules), ref_rows)
    c = lib.calls[-1]
    assert c["k"] == rules.get("k", 0) and (c["knn"] is None) == ("k" not in rules) and len(lib.calls) == 2          # one library call each


def test_remove_outliers_without_a_finite_kth_distance_keeps_nothing(lib):
    cloud = stray_scene()[:50]
    rows, keep = api.remove_outliers(cloud, 1e-4, k=2, return_mask=True, matcher=FakeMatcher())
    assert rows.shape == (0, 3) and not keep.any()


@pytest.mark.parametrize("kw", [dict(), dict(min_neighbors=0), dict(k=0), dict(k=33), dict(k=2, ratio=0.0), dict(k=2, ratio=float("nan")), dict(k=2, ratio=float("inf"))])
def test_remove_outliers_refuses_bad_settings(lib, kw):
    with pytest.raises(ValueError):
        api.remove_outliers(np.zeros((3, 3), F), 1.0, matcher=FakeMatcher(), **kw)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            api.remove_outliers(np.zeros((3, 3), F), radius, min_neighbors=1, matcher=FakeMatcher())
    assert lib.calls == []

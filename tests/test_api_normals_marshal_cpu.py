"""api.cloud_normals / api.normal_compare without a GPU: the library is replaced by a recorder that notes every argument of
tsar_cloud_normals_ctx and tsar_cloud_normal_compare_ctx in order and fills the outputs from the numpy restatement.  Holds the argument
order, the params struct, the None handling and the host side (degrees to thresholds, counts to ratios) of the binding."""
import ctypes as C

import numpy as np
import pytest

from cloud_normals_ref import cloud_normals_ref, normal_compare_ref
from tsar_mvs_amd import api

F = np.float32


def view(ptr, ctype, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape)


class Recorder:
    """stands for libtsar_hip.so: the entries cloud_normals and normal_compare call"""

    def __init__(self, rc=api.TSAR_OK, pairs=None):
        self.calls, self.rc, self.pairs = [], rc, pairs

    def tsar_default_cloud_normals_params(self, ref):
        p = ref._obj
        p.radius, p.k, p.min_neighbors, p.orient, p.max_pairs = 0.0, 16, 5, 0, 1 << 40

    def tsar_cloud_normals_ctx(self, ctx, cloud, n, stride, p, knn, used, normal, curv, cov, n_valid, n_normals, pairs, mem):
        p = p._obj
        self.calls.append(dict(ctx=ctx, cloud=cloud, n=n, stride=stride, radius=p.radius, k=p.k, min_neighbors=p.min_neighbors, orient=p.orient,
                               viewpoint=tuple(p.viewpoint), max_pairs=p.max_pairs, knn=knn, used=used, normal=normal, curv=curv, cov=cov, mem=mem))
        if self.pairs is not None:
            pairs._obj.value = self.pairs
        if self.rc != api.TSAR_OK:
            return self.rc
        pts = view(cloud, C.c_float, (n, stride)) if n else np.zeros((0, stride), F)
        ref = cloud_normals_ref(pts, p.radius, p.k, p.min_neighbors, p.orient, tuple(p.viewpoint))
        for ptr, key, ctype, shape in ((knn, "knn_index", C.c_int32, (n, p.k)), (used, "n_used", C.c_int32, (n,)), (normal, "normal", C.c_float, (n, 3)),
                                       (curv, "curvature", C.c_float, (n,)), (cov, "cov", C.c_double, (n, 6))):
            if ptr is not None and n:
                view(ptr, ctype, shape)[:] = ref[key]
        n_valid._obj.value, n_normals._obj.value, pairs._obj.value = ref["n_valid"], ref["n_normals"], ref["pairs"]
        return api.TSAR_OK

    def tsar_cloud_normal_compare_ctx(self, ctx, a, stride_a, n, b, stride_b, n_b, index, dist2, max_dist, n_tol, min_cos, is_signed, cos, within, n_compared, mem):
        mc = view(min_cos, C.c_double, (n_tol,)).copy() if n_tol else np.zeros(0)
        self.calls.append(dict(ctx=ctx, a=a, stride_a=stride_a, n=n, b=b, stride_b=stride_b, n_b=n_b, index=index, dist2=dist2, max_dist=max_dist, min_cos=mc,
                               is_signed=is_signed, cos=cos, mem=mem))
        if self.rc != api.TSAR_OK:
            return self.rc
        ref = normal_compare_ref(view(a, C.c_float, (n, stride_a)), view(b, C.c_float, (n_b, stride_b)), view(index, C.c_int32, (n,)), mc,
                                 None if dist2 is None else view(dist2, C.c_float, (n,)), max_dist, bool(is_signed))
        if cos is not None:
            view(cos, C.c_float, (n,))[:] = ref["cos"]
        view(within, C.c_int64, (n_tol,))[:] = ref["within"]
        n_compared._obj.value = ref["n_compared"]
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


def test_the_params_struct_is_the_headers():
    P = api.CloudNormalsParams
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("radius", 0), ("k", 4), ("min_neighbors", 8), ("orient", 12), ("viewpoint", 16), ("max_pairs", 32)]
    assert C.sizeof(P) == 40


def test_argument_order_and_defaults(lib):
    rng = np.random.default_rng(0)
    cloud = rng.random((60, 9)).astype(F)
    want = ("knn_index", "n_used", "normal", "curvature", "cov")
    res = api.cloud_normals(cloud, 0.6, want=want, matcher=FakeMatcher())
    (c,) = lib.calls
    assert c["ctx"] == "the context" and c["cloud"].value == cloud.ctypes.data and (c["n"], c["stride"], c["mem"]) == (60, 9, api.MEM_HOST)
    assert (c["radius"], c["k"], c["min_neighbors"], c["orient"], c["viewpoint"], c["max_pairs"]) == (F(0.6), 16, 5, 0, (0.0, 0.0, 0.0), 1 << 40)
    for arg, key in (("knn", "knn_index"), ("used", "n_used"), ("normal", "normal"), ("curv", "curvature"), ("cov", "cov")):
        assert c[arg].value == res[key].ctypes.data, key
    ref = cloud_normals_ref(cloud, 0.6)
    for key, dt, shape in (("knn_index", np.int32, (60, 16)), ("n_used", np.int32, (60,)), ("normal", F, (60, 3)), ("curvature", F, (60,)), ("cov", np.float64, (60, 6))):
        assert res[key].dtype == dt and res[key].shape == shape and np.array_equal(res[key], ref[key]), key
    assert (res["n_valid"], res["n_normals"], res["pairs"]) == (60, ref["n_normals"], ref["pairs"]) and ref["n_normals"] > 30


def test_orientation_settings_and_unwanted_outputs(lib):
    cloud = np.zeros((4, 6), F)
    res = api.cloud_normals(cloud, 1.0, k=3, min_neighbors=2, orient="viewpoint", viewpoint=(1, 2.5, -3), max_pairs=77, matcher=FakeMatcher())
    c = lib.calls[-1]
    assert (c["k"], c["min_neighbors"], c["orient"], c["viewpoint"], c["max_pairs"]) == (3, 2, 1, (1.0, 2.5, -3.0), 77)
    assert c["knn"] is None and c["used"] is None and c["cov"] is None and c["normal"] is not None and c["curv"] is not None
    assert sorted(res) == ["curvature", "n_normals", "n_valid", "normal", "pairs"]
    api.cloud_normals(cloud, 1.0, orient="record", want=("knn_index",), matcher=FakeMatcher())
    c = lib.calls[-1]
    assert c["orient"] == 2 and c["knn"] is not None and c["normal"] is None and c["curv"] is None
    res = api.cloud_normals(np.zeros((0, 3), F), 1.0, k=8, want=("knn_index", "cov"), matcher=FakeMatcher())      # an empty cloud goes in as NULL
    assert lib.calls[-1]["cloud"] is None and res["knn_index"].shape == (0, 8) and res["cov"].shape == (0, 6)
    for kw in (dict(orient="outwards"), dict(orient="viewpoint"), dict(viewpoint=(0, 0, 0))):
        with pytest.raises(AssertionError):
            api.cloud_normals(cloud, 1.0, matcher=FakeMatcher(), **kw)


def test_a_refusal_carries_the_pairs(monkeypatch):
    rec = Recorder(rc=api.TSAR_ERR_INVALID, pairs=1234)
    monkeypatch.setattr(api, "load_library", lambda *a: rec)
    with pytest.raises(api.TsarError) as e:
        api.cloud_normals(np.zeros((2, 3), F), 1.0, max_pairs=5, matcher=FakeMatcher())
    assert e.value.pairs == 1234 and "the recorder's refusal" in str(e.value)
    rec.pairs = None
    with pytest.raises(api.TsarError) as e:
        api.cloud_normals(np.zeros((2, 3), F), 1.0, matcher=FakeMatcher())
    assert e.value.pairs is None


def test_normal_compare_marshals_thresholds_and_forms_the_ratios(lib):
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(50, 6)).astype(F), rng.normal(size=(20, 3)).astype(F)
    idx = rng.integers(-1, 20, 50).astype(np.int32)
    d2 = rng.random(50).astype(F)
    res = api.normal_compare(a, b, idx, [10, 30, 90], dist2=d2, max_dist=0.8, signed=True, want_cos=True, matcher=FakeMatcher())
    (c,) = lib.calls
    assert c["ctx"] == "the context" and (c["a"].value, c["stride_a"], c["n"]) == (a.ctypes.data, 6, 50) and (c["b"].value, c["stride_b"], c["n_b"]) == (b.ctypes.data, 3, 20)
    assert c["index"].value == idx.ctypes.data and c["dist2"].value == d2.ctypes.data and c["max_dist"] == 0.8 and c["is_signed"] == 1 and c["mem"] == api.MEM_HOST
    assert c["min_cos"].tolist() == np.cos(np.deg2rad(np.array([10.0, 30.0, 90.0]))).tolist() and c["cos"].value == res["cos"].ctypes.data
    ref = normal_compare_ref(a, b, idx, c["min_cos"], d2, 0.8, True)
    assert res["n_compared"] == ref["n_compared"] > 5 and res["within"].tolist() == ref["within"].tolist()
    assert res["accuracy"].tolist() == (ref["within"] / np.float64(ref["n_compared"])).tolist() and res["tolerances_deg"].tolist() == [10.0, 30.0, 90.0]
    res = api.normal_compare(a, b, idx, [45], matcher=FakeMatcher())
    c = lib.calls[-1]
    assert c["dist2"] is None and c["is_signed"] == 0 and c["cos"] is None and "cos" not in res
    res = api.normal_compare(a, b, np.full(50, -1), [45], matcher=FakeMatcher())              # nothing compared: the ratio is 0, not NaN
    assert res["n_compared"] == 0 and res["accuracy"].tolist() == [0.0]
    with pytest.raises(AssertionError):
        api.normal_compare(a, b, idx, [45], dist2=d2, matcher=FakeMatcher())

"""The binding's marshalling helpers on the CPU (tsar-mvs_amd/api.py): a caller's buffer in, the outputs out, the camera array, the
harmonic mean.  Arrays of a few elements; no library call is made."""
import ctypes as C

import numpy as np
import pytest

from tsar_mvs_amd import api


def _address(p):
    return C.cast(p, C.c_void_p).value


def test_none_is_a_null_host_pointer():
    a, p, kind = api._buf(None, np.float32, (2, 3), "x")
    assert a is None and p is None and kind == api.MEM_HOST
    assert api._one_kind([(a, p, kind)], "x") == api.MEM_HOST


@pytest.mark.parametrize("tensors", (None, "device", "any"))
def test_a_strided_float64_slice_is_copied_once_to_contiguous_float32(tensors):
    src = (np.arange(60, dtype=np.float64) / 7.0).reshape(5, 12)[:, ::4]         # [5, 3], neither contiguous nor float32
    assert not src.flags["C_CONTIGUOUS"]
    a, p, kind = api._buf(src, np.float32, (5, 3), "x", tensors=tensors)
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.shape == (5, 3) and kind == api.MEM_HOST
    assert np.array_equal(a, src.astype(np.float32))
    assert _address(p) == a.ctypes.data                                          # the pointer is the returned array's, which the caller holds
    same = np.zeros((5, 3), np.float32)
    assert api._buf(same, np.float32, (5, 3), "x", tensors=tensors)[0] is same   # nothing to do: no copy


def test_a_cpu_tensor_stays_or_goes_through_numpy_as_the_call_says():
    import torch
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert api._buf(t, np.float32, (2, 3), "x", tensors="any")[0] is t
    for tensors in (None, "device"):
        a, p, kind = api._buf(t, np.float32, (2, 3), "x", tensors=tensors)
        assert isinstance(a, np.ndarray) and np.array_equal(a, t.numpy()) and kind == api.MEM_HOST
    with pytest.raises(AssertionError, match="float32"):
        api._buf(t.double(), np.float32, None, "x", tensors="any")
    assert api._buf(t.double(), np.float32, None, "x", tensors="any", typed=False)[0].dtype == torch.float64   # the older entries' contract


def test_a_wrong_shape_is_refused_with_the_shape_found():
    with pytest.raises(AssertionError, match=r"depth map 2 has shape \(4, 3\), not \(3, 4\)"):
        api._buf(np.zeros((4, 3)), np.float32, (3, 4), "depth map 2")


def test_buffers_of_two_kinds_are_refused():
    host = api._buf(np.zeros(3), np.float32)
    device = (host[0], host[1], api.MEM_DEVICE)            # what _buf returns for a device tensor, as far as the kinds go
    assert api._one_kind([host, host, api._buf(None, np.float32)], "x") == api.MEM_HOST
    with pytest.raises(AssertionError, match="the maps must live in the same memory space"):
        api._one_kind([host, device], "the maps")


def test_outputs_are_the_ones_wanted():
    spec = {"count": ((3, 5), np.uint8), "depth": ((3, 5), np.float32), "normal": ((3, 5, 3), np.float32)}
    res = api._outputs(spec, ("count",))
    assert list(res) == ["count"]
    assert res["count"].dtype == np.uint8 and res["count"].shape == (3, 5) and res["count"].flags["C_CONTIGUOUS"]
    res = api._outputs(spec, ("normal", "depth", "other"))
    assert list(res) == ["depth", "normal"] and res["normal"].shape == (3, 5, 3) and res["normal"].dtype == np.float32
    import torch
    res = api._outputs(spec, ("count", "depth"), torch.device("cpu"))
    assert [(k, v.dtype, tuple(v.shape), v.is_contiguous()) for k, v in res.items()] == [("count", torch.uint8, (3, 5), True), ("depth", torch.float32, (3, 5), True)]


def test_cameras_hold_k_r_t_byte_for_byte():
    rng = np.random.default_rng(5)
    K, R, t = rng.standard_normal((2, 3, 3)), rng.standard_normal((2, 3, 3)), rng.standard_normal((2, 3))
    K[1, 0, 0], t[0, 2] = np.nan, -0.0
    cams = api._cameras(K, R, t, 2)
    assert len(cams) == 2 and C.sizeof(cams) == 2 * 21 * 4
    for i in range(2):
        for field, src in (("K", K), ("R", R), ("t", t)):
            assert bytes(getattr(cams[i], field)) == src[i].astype(np.float32).tobytes(), (i, field)


def test_f1_is_the_harmonic_mean_in_float64():
    a = np.array([0.0, 0.0, 0.5, 1.0, 1.0 / 3.0])
    c = np.array([0.0, 0.7, 0.25, 1.0, 2.0 / 7.0])
    f = api._f1(a, c)
    assert f.dtype == np.float64 and f[0] == 0.0 and f[1] == 0.0
    assert np.array_equal(f[2:], 2.0 * a[2:] * c[2:] / (a[2:] + c[2:]))

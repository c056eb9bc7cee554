"""ctypes binding of libtsar_hip.so (include/tsar.h) and a thin `Matcher` object mirroring the reference's
operator sequence (`firstcuda` / `sliccuda` / `fakecuda` / `fillcuda`, reference gipuma.h:2-6, called from
runGipuma, reference main.cpp:1493-1783).

There is no CPU fallback: if the HIP library is missing or no GPU is present the calls raise.
Buffers may be numpy arrays (host) or torch CUDA tensors (device, zero-copy via data_ptr()).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSAR_LIB") or os.path.join(_HERE, "libtsar_hip.so")     # TSAR_LIB: A/B builds only

TSAR_OK = 0
TSAR_ERR_INVALID, TSAR_ERR_HIP, TSAR_ERR_STATE, TSAR_ERR_NOMEM = -1, -2, -3, -4
MEM_HOST, MEM_DEVICE = 0, 1
COMB_ALL, COMB_BEST_N, COMB_ANGLE, COMB_GOOD = 0, 1, 2, 3
FLAG_FIX_DOWN_FAR_SEED, FLAG_FIX_RIGHT_FAR_CMP, FLAG_STRICT_DIV = 1, 2, 4
FLAG_FIX_PLANE_FIT = 8
FLAG_NO_LINE_CLOSING = 16
FLAG_TEX_FILTER_8BIT = 32
FLAG_FIX_INIT_RADIUS = 64
MAXCOST = 2.0
MAX_VIEWS = 64


class TsarError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tsar error {code}: {msg}")
        self.code = code


class Camera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3)]


class Params(C.Structure):
    _fields_ = [("box_hsize", C.c_int32), ("box_vsize", C.c_int32), ("n_best", C.c_int32), ("cost_comb", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float), ("cam_scale", C.c_float), ("flags", C.c_uint32),
                ("seed", C.c_uint64)]


class SlicSettings(C.Structure):
    _fields_ = [("spixel_size", C.c_int32), ("no_iters", C.c_int32), ("coh_weight", C.c_float),
                ("do_enforce_connectivity", C.c_int32), ("color_space", C.c_int32)]


class FusionParams(C.Structure):
    _fields_ = [("num_consistent", C.c_int32), ("reproj_error", C.c_float), ("depth_diff", C.c_float), ("angle_deg", C.c_float),
                ("used_list", C.c_int32)]


class GeomCheckParams(C.Structure):
    _fields_ = [("reproj_error", C.c_float), ("depth_diff", C.c_float), ("min_consistent", C.c_int32)]


class GeomReprojectParams(C.Structure):
    _fields_ = [("depth_diff", C.c_float), ("min_views", C.c_int32)]


class PlanePriorParams(C.Structure):
    _fields_ = [("weight_depth", C.c_float), ("weight_normal", C.c_float), ("depth_clip", C.c_float), ("normal_clip", C.c_float)]


class PlanePriorBuildParams(C.Structure):
    _fields_ = [("cell", C.c_int32), ("max_levels", C.c_int32)]


class CloudDistanceParams(C.Structure):
    _fields_ = [("max_dist", C.c_float), ("max_pairs", C.c_int64)]


class CloudVoxelsParams(C.Structure):
    _fields_ = [("voxel", C.c_float)]


class CloudNeighborsParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("k", C.c_int32), ("max_pairs", C.c_int64)]


class CloudNormalsParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("k", C.c_int32), ("min_neighbors", C.c_int32), ("orient", C.c_int32), ("viewpoint", C.c_float * 3), ("max_pairs", C.c_int64)]


class CloudRenderParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("max_px", C.c_int32), ("occlusion_diff", C.c_float), ("depth_diff", C.c_float), ("min_points", C.c_int32),
                ("max_splats", C.c_int64)]


class KernelTiming(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int32), ("total_ms", C.c_float)]


# the reference's spixel_info (gSLICr_spixel_info.h:11-17), the record of tsar_selftest_slic_stage's centre arrays
SPIXEL_DTYPE = np.dtype([("center", np.float32, 2), ("color", np.float32, 4), ("id", np.int32), ("n", np.int32)])

# every function include/tsar.h declares, in the header's order: name -> (restype, argtypes).  tests/test_abi.py holds the names, the
# argument counts and the return types to the header; __graft_entry__.build() holds the built library to the names.
_P, _I, _F, _Z, _L, _U64, _p = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64, C.c_uint64, C.POINTER
_SET_VIEWS = (_I, [_P, _I, _I, _I, _p(_P), _I, _p(Camera)])
_FUSE = (_I, [_I, _I, _I, _I, _p(Camera), _p(_P), _p(_P), _p(_P), _I, _P, _P, _p(FusionParams), _P, _L, _p(_L)])
_CLOUD_DISTANCE = (_I, [_I, _P, _L, _I, _P, _L, _I, _p(CloudDistanceParams), _I, _P, _P, _P, _P, _p(_L), _p(_L), _I])
_CLOUD_VOXELS = (_I, [_I, _P, _L, _I, _p(CloudVoxelsParams), _P, _I, _P, _P, _L, _P, _P, _P, _p(_L), _p(_L), _I])
_CLOUD_NEIGHBORS = (_I, [_I, _P, _L, _I, _p(CloudNeighborsParams), _P, _P, _p(_L), _p(_L), _I])
_CLOUD_NORMALS = (_I, [_I, _P, _L, _I, _p(CloudNormalsParams), _P, _P, _P, _P, _P, _p(_L), _p(_L), _p(_L), _I])
_CLOUD_NORMAL_COMPARE = (_I, [_I, _P, _I, _L, _P, _I, _L, _P, _P, _F, _I, _P, _I, _P, _P, _p(_L), _I])

_CLOUD_RENDER = (_I, [_I, _P, _L, _I, _p(Camera), _I, _I, _p(CloudRenderParams), _P, _P, _P, _p(_L), _I])
_CLOUD_RENDER_ORIENTED = (_I, [_I, _P, _L, _I, _P, _I, _p(Camera), _I, _I, _p(CloudRenderParams), _P, _P, _P, _P, _p(_L), _p(_L), _I])
_DEPTH_COMPARE = (_I, [_I, _P, _P, _P, _L, _I, _P, _p(_L), _p(_L), _P, _p(_L), _p(_L), _P, _I])


def _on_ctx(sig):
    """the signature of a context-free entry's _ctx twin: the context in place of the device index"""
    return sig[0], [_P] + sig[1][1:]


_ABI = {
    "tsar_create": (_I, [_I, _p(_P)]),
    "tsar_destroy": (_I, [_P]),
    "tsar_last_error": (C.c_char_p, [_P]),
    "tsar_version": (C.c_char_p, []),
    "tsar_get_stream": (_I, [_P, _p(_P)]),
    "tsar_synchronize": (_I, [_P]),
    "tsar_default_params": (None, [_p(Params)]),
    "tsar_set_params": (_I, [_P, _p(Params)]),
    "tsar_set_views": _SET_VIEWS,
    "tsar_set_views_u8": _SET_VIEWS,
    "tsar_set_view_subset": (_I, [_P, _I, _P]),
    "tsar_pm_init": (_I, [_P]),
    "tsar_pm_iterate": (_I, [_P, _I]),
    "tsar_pm_iterate_final": (_I, [_P, _I, _P, _I]),
    "tsar_pm_cost_planes": (_I, [_P, _P, _I, _P, _P, _P]),
    "tsar_set_plane": (_I, [_P, _P, _P, _I]),
    "tsar_pm_sweep": (_I, [_P, _I, _I, _I]),
    "tsar_set_sweep_counter": (_I, [_P, _I]),
    "tsar_get_plane": (_I, [_P, _P, _P, _P, _P, _I]),
    "tsar_load_planes": (_I, [_P, _P, _P, _I]),
    "tsar_compute_disp": (_I, [_P]),
    "tsar_compute_disp_final": (_I, [_P, _P, _P, _I]),
    "tsar_depth_to_plane": (_I, [_P]),
    "tsar_pyramid_views": (_I, [_P, _P]),
    "tsar_upsample_planes": (_I, [_P, _P]),
    "tsar_compute_disp_final_upsampled": (_I, [_P, _P, _I]),
    "tsar_get_view_image": (_I, [_P, _I, _P, _I]),
    "tsar_set_geom_depths": (_I, [_P, _I, _p(_P), _I, _F, _F]),
    "tsar_clear_geom": (_I, [_P]),
    "tsar_pm_rescore": (_I, [_P]),
    "tsar_get_geom_matrices": (_I, [_P, _I, _P, _P]),
    "tsar_geom_pyramid": (_I, [_P, _P]),
    "tsar_pyramid_planes": (_I, [_P, _P]),
    "tsar_upsample_merge": (_I, [_P, _P]),
    "tsar_default_geom_check_params": (None, [_p(GeomCheckParams)]),
    "tsar_geom_check": (_I, [_P, _P, _p(GeomCheckParams), _P, _P, _I]),
    "tsar_default_geom_reproject_params": (None, [_p(GeomReprojectParams)]),
    "tsar_geom_reproject": (_I, [_P, _p(GeomReprojectParams), _P, _P, _I]),
    "tsar_pm_merge_depths": (_I, [_P, _P, _I, _p(_L)]),
    "tsar_default_plane_prior_params": (None, [_p(PlanePriorParams)]),
    "tsar_set_plane_prior": (_I, [_P, _P, _P, _I, _p(PlanePriorParams)]),
    "tsar_clear_plane_prior": (_I, [_P]),
    "tsar_get_plane_prior": (_I, [_P, _P, _I]),
    "tsar_default_plane_prior_build_params": (None, [_p(PlanePriorBuildParams)]),
    "tsar_build_plane_prior": (_I, [_P, _P, _P, _I, _p(PlanePriorBuildParams), _P, _P, _P]),
    "tsar_get_result": (_I, [_P, _P, _P, _P, _P, _I]),
    "tsar_set_reliable_mask": (_I, [_P, _P, _I]),
    "tsar_get_reliable_mask": (_I, [_P, _P, _I]),
    "tsar_lrdiff": (_I, [_P]),
    "tsar_getview": (_I, [_P]),
    "tsar_wmf": (_I, [_P, _I, _I]),
    "tsar_set_regions": (_I, [_P, _P, _I, _P, _P, _I]),
    "tsar_detect_weak_texture": (_I, [_P, _P, _I, _p(_I), _P, _P, _I]),
    "tsar_ransac_regions": (_I, [_P, _P, _P]),
    "tsar_set_region_planes": (_I, [_P, _P]),
    "tsar_fake_depth": (_I, [_P, _P, _I]),
    "tsar_fill_textureless": (_I, [_P]),
    "tsar_default_slic_settings": (None, [_p(SlicSettings)]),
    "tsar_slic": (_I, [_P, _P, _I, _I, _p(SlicSettings), _P, _I]),
    "tsar_default_fusion_params": (None, [_p(FusionParams)]),
    "tsar_fuse_ctx": _on_ctx(_FUSE),
    "tsar_fuse": _FUSE,
    "tsar_default_cloud_distance_params": (None, [_p(CloudDistanceParams)]),
    "tsar_cloud_distance_ctx": _on_ctx(_CLOUD_DISTANCE),
    "tsar_cloud_distance": _CLOUD_DISTANCE,
    "tsar_default_cloud_voxels_params": (None, [_p(CloudVoxelsParams)]),
    "tsar_cloud_voxels_ctx": _on_ctx(_CLOUD_VOXELS),
    "tsar_cloud_voxels": _CLOUD_VOXELS,
    "tsar_default_cloud_neighbors_params": (None, [_p(CloudNeighborsParams)]),
    "tsar_cloud_neighbors_ctx": _on_ctx(_CLOUD_NEIGHBORS),
    "tsar_cloud_neighbors": _CLOUD_NEIGHBORS,
    "tsar_default_cloud_normals_params": (None, [_p(CloudNormalsParams)]),
    "tsar_cloud_normals_ctx": _on_ctx(_CLOUD_NORMALS),
    "tsar_cloud_normals": _CLOUD_NORMALS,
    "tsar_cloud_normal_compare_ctx": _on_ctx(_CLOUD_NORMAL_COMPARE),
    "tsar_cloud_normal_compare": _CLOUD_NORMAL_COMPARE,
    "tsar_default_cloud_render_params": (None, [_p(CloudRenderParams)]),
    "tsar_cloud_render_ctx": _on_ctx(_CLOUD_RENDER),
    "tsar_cloud_render": _CLOUD_RENDER,
    "tsar_cloud_render_oriented_ctx": _on_ctx(_CLOUD_RENDER_ORIENTED),
    "tsar_cloud_render_oriented": _CLOUD_RENDER_ORIENTED,
    "tsar_depth_compare_ctx": _on_ctx(_DEPTH_COMPARE),
    "tsar_depth_compare": _DEPTH_COMPARE,
    "tsar_host_alloc": (_P, [_Z]),
    "tsar_host_free": (None, [_P]),
    "tsar_device_alloc": (_P, [_I, _Z]),
    "tsar_device_free": (None, [_I, _P]),
    "tsar_device_write": (_I, [_I, _P, _P, _Z]),
    "tsar_device_read": (_I, [_I, _P, _P, _Z]),
    "tsar_peer_copy": (_I, [_I, _P, _I, _P, _Z]),
    "tsar_enable_kernel_timing": (_I, [_P, _I]),
    "tsar_reset_kernel_timing": (_I, [_P]),
    "tsar_get_kernel_timing": (_I, [_P, _p(KernelTiming), _I, _p(_I)]),
    "tsar_selftest_sqrt": (_I, [_P, _I, _U64, _p(_U64)]),
    "tsar_selftest_divide": (_I, [_P, _P, _P, _P, _Z, _P, _P, _I]),
    "tsar_selftest_divide_random": (_I, [_P, _I, _U64, _I, _I, _p(_U64), _p(_U64)]),
    "tsar_selftest_sweep_census": (_I, [_P, _I, _p(_U64)]),
    "tsar_selftest_sweep_repeat": (_I, [_P, _I, _P, _p(_U64)]),
    "tsar_selftest_prune_census": (_I, [_P, _I, _p(C.c_uint32)]),
    "tsar_selftest_slic_stage": (_I, [_P, _I, _I, _I, _I, _I, _p(SlicSettings), _P, _P, _P]),
}
ABI_SYMBOLS = list(_ABI)      # (tests check that the library exports exactly these)

_lib = None


def load_library(path: str = LIB_PATH):
    """Load libtsar_hip.so; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `make -C tsar-mvs_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(L, name, None)       # None: a library built before the entry, loaded through TSAR_LIB for an A/B run; a call raises AttributeError
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def default_params(**kw) -> Params:
    p = Params()
    load_library().tsar_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _ptr(a):
    """(pointer, mem kind) of a numpy array or torch tensor; None -> (NULL, host)."""
    if a is None:
        return None, MEM_HOST
    if _is_torch(a):
        assert a.is_contiguous(), "tensor must be contiguous"
        if a.is_cuda:
            # include/tsar.h: device buffers must be complete before the call — the context's stream is not ordered
            # against torch's.  Whatever produced (or still reads) this tensor ran on torch's current stream.
            import torch
            torch.cuda.current_stream(a.device).synchronize()
        return C.c_void_p(a.data_ptr()), (MEM_DEVICE if a.is_cuda else MEM_HOST)
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.c_void_p), MEM_HOST


def _coerce(a, dtype, shape=None, name="the array", tensors=None, typed=True):
    """a caller's array (or None) as the library takes it.  tensors says which torch tensors stay as they are: None = none, "device" =
    device tensors, "any" = CPU tensors too; a tensor that stays must be of `dtype` if `typed`.  Everything else goes through numpy and
    comes back C-contiguous and of `dtype`, copied only where it is not that already.  shape: the exact shape to insist on."""
    if a is None:
        return None
    if _is_torch(a) and (tensors == "any" or (tensors == "device" and a.is_cuda)):
        assert not typed or str(a.dtype) == "torch." + np.dtype(dtype).name, "%s must be a %s tensor" % (name, np.dtype(dtype).name)
    else:
        a = np.ascontiguousarray(a.numpy() if tensors and _is_torch(a) else a, dtype)
    assert shape is None or tuple(a.shape) == tuple(shape), "%s has shape %s, not %s" % (name, tuple(a.shape), tuple(shape))
    return a


def _buf(a, dtype, shape=None, name="the array", tensors=None, typed=True):
    """_coerce's array, which the caller keeps alive over the call, with _ptr's pointer and memory kind: (array, pointer, kind)"""
    a = _coerce(a, dtype, shape, name, tensors, typed)
    return (a,) + _ptr(a)


def _ptr_array(bufs, n):
    """the n pointers of the _buf triples (NULL past the last) as a void* array"""
    return (C.c_void_p * n)(*(p for _, p, _ in bufs))


def _one_kind(bufs, what):
    """the memory kind that the _buf triples share (None arrays aside; MEM_HOST if nothing is left); device tensors lie on one device"""
    kinds = {kind for a, _, kind in bufs if a is not None}
    assert len(kinds) <= 1, what + " must live in the same memory space"
    assert len({a.device for a, _, kind in bufs if kind == MEM_DEVICE}) <= 1, what + " must live on one device"
    return kinds.pop() if kinds else MEM_HOST


def _outputs(spec, want, target=None, empty=np.empty):
    """uninitialised outputs for the keys of spec = {key: (shape, dtype)} that `want` names: torch tensors on the torch.device `target`,
    or (target None) host arrays from `empty`"""
    spec = {k: v for k, v in spec.items() if k in want}
    if target is None:
        return {k: empty(shape, dt) for k, (shape, dt) in spec.items()}
    import torch
    return {k: torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=target) for k, (shape, dt) in spec.items()}


def _cameras(K, R, t, n):
    """the Camera array of n views from their K [n, 3, 3], R [n, 3, 3] and t [n, 3]"""
    rec = np.concatenate([np.asarray(a, np.float32).reshape(n, k) for a, k in ((K, 9), (R, 9), (t, 3))], axis=1)
    return (Camera * n).from_buffer_copy(rec)


class Matcher:
    """One context = one GPU.  Mirrors the order in which runGipuma drives the GPU operators."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        self._ctx = C.c_void_p()
        rc = self.L.tsar_create(device, C.byref(self._ctx))
        if rc != TSAR_OK:
            raise TsarError(rc, "tsar_create failed (is a HIP device visible?)")
        self.w = self.h = self.n_views = 0
        self.device = device
        self.plane_prior_params = None     # the struct the last set_plane_prior passed, while that prior is installed

    def close(self):
        if self._ctx:
            self.L.tsar_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != TSAR_OK:
            raise TsarError(rc, self.L.tsar_last_error(self._ctx).decode())

    # ---- inputs ----
    def set_params(self, params: Params):
        self._chk(self.L.tsar_set_params(self._ctx, C.byref(params)))
        self.params = params

    def set_views(self, images, K, R, t, u8: bool = False):
        """images: list of [h, w] float32 arrays/tensors (view 0 = reference); K, R, t: per-view
        intrinsics and world->camera extrinsics as in cams/%08d_cam.txt.  u8: the images are uint8 (the 8-bit decode itself)
        and go through tsar_set_views_u8, which widens them on the device."""
        n = len(images)
        first = images[0]
        h, w = int(first.shape[0]), int(first.shape[1])
        bufs = [_buf(im, np.uint8 if u8 else np.float32, (h, w), "image %d" % i, tensors="any", typed=u8) for i, im in enumerate(images)]
        self._chk((self.L.tsar_set_views_u8 if u8 else self.L.tsar_set_views)(self._ctx, n, w, h, _ptr_array(bufs, n), _one_kind(bufs, "all images"),
                                                                              _cameras(K, R, t, n)))
        self.w, self.h, self.n_views = w, h, n
        self.plane_prior_params = None     # tsar_set_views removes a prior

    def set_view_subset(self, idx):
        a = np.ascontiguousarray(idx, np.int32)
        self._chk(self.L.tsar_set_view_subset(self._ctx, len(a), a.ctypes.data_as(C.c_void_p)))

    # ---- PatchMatch ----
    def pm_init(self):
        self._chk(self.L.tsar_pm_init(self._ctx))

    def pm_iterate(self, iters: int):
        self._chk(self.L.tsar_pm_iterate(self._ctx, iters))

    def pm_iterate_final(self, iters: int, text):
        """the kernels' `final == true` mode; text [h, w] = lines->text (-1: pixel is left untouched)"""
        text, p, kind = _buf(text, np.float32, tensors="any", typed=False)
        self._chk(self.L.tsar_pm_iterate_final(self._ctx, iters, p, kind))

    def pm_sweep(self, colour: int, do_prop: bool = True, do_refine: bool = True):
        self._chk(self.L.tsar_pm_sweep(self._ctx, colour, int(do_prop), int(do_refine)))

    def set_sweep_counter(self, n: int):
        self._chk(self.L.tsar_set_sweep_counter(self._ctx, n))

    def pm_cost_planes(self, planes):
        planes = np.ascontiguousarray(planes, np.float32)
        cost = np.empty((self.h, self.w), np.float32)
        bv = np.empty((self.h, self.w), np.int32)
        rt = np.empty((self.h, self.w), np.float32)
        self._chk(self.L.tsar_pm_cost_planes(self._ctx, _ptr(planes)[0], MEM_HOST, _ptr(cost)[0], _ptr(bv)[0], _ptr(rt)[0]))
        return cost, bv, rt

    def set_plane(self, planes, cost):
        planes = np.ascontiguousarray(planes, np.float32)
        cost = np.ascontiguousarray(cost, np.float32)
        self._chk(self.L.tsar_set_plane(self._ctx, _ptr(planes)[0], _ptr(cost)[0], MEM_HOST))

    def get_plane(self):
        planes = np.empty((self.h, self.w, 4), np.float32)
        cost = np.empty((self.h, self.w), np.float32)
        bv = np.empty((self.h, self.w), np.int32)
        rt = np.empty((self.h, self.w), np.float32)
        self._chk(self.L.tsar_get_plane(self._ctx, _ptr(planes)[0], _ptr(cost)[0], _ptr(bv)[0], _ptr(rt)[0], MEM_HOST))
        return planes, cost, bv, rt

    # ---- plane <-> depth ----
    def load_planes(self, depth, normal_world):
        d = _buf(depth, np.float32, tensors="any", typed=False)
        n = _buf(normal_world, np.float32, tensors="any", typed=False)
        self._chk(self.L.tsar_load_planes(self._ctx, d[1], n[1], _one_kind((d, n), "depth and normal_world")))

    def compute_disp(self):
        self._chk(self.L.tsar_compute_disp(self._ctx))

    def compute_disp_final(self, resize_planes, text):
        r = np.ascontiguousarray(resize_planes, np.float32)
        t = np.ascontiguousarray(text, np.float32)
        self._chk(self.L.tsar_compute_disp_final(self._ctx, _ptr(r)[0], _ptr(t)[0], MEM_HOST))

    def depth_to_plane(self):
        self._chk(self.L.tsar_depth_to_plane(self._ctx))

    # ---- coarse-to-fine ----
    def pyramid_from(self, fine: "Matcher"):
        """install fine's views downsampled by 2 (pyrDown) with K / 2, fine's params and view subset (tsar_pyramid_views)"""
        self._chk(self.L.tsar_pyramid_views(self._ctx, fine._ctx))
        self.w, self.h, self.n_views = (fine.w + 1) // 2, (fine.h + 1) // 2, fine.n_views
        self.params = fine.params

    def upsample_planes(self, coarse: "Matcher"):
        """start this context's plane state from coarse's (each pixel keeps the cheapest of its four nearest coarse planes) and keep
        the chosen planes for compute_disp_final_upsampled (tsar_upsample_planes)"""
        self._chk(self.L.tsar_upsample_planes(self._ctx, coarse._ctx))

    def get_view_image(self, view: int):
        """the image of `view` as the context holds it: [h, w] float32"""
        out = np.empty((self.h, self.w), np.float32)
        self._chk(self.L.tsar_get_view_image(self._ctx, view, _ptr(out)[0], MEM_HOST))
        return out

    def compute_disp_final_upsampled(self, text):
        """compute_disp_final with the planes the last upsample_planes kept; text [h, w] = lines->text (-1 textureless, 1 otherwise),
        a numpy array or a torch device tensor"""
        text, p, kind = _buf(text, np.float32, tensors="any", typed=False)
        self._chk(self.L.tsar_compute_disp_final_upsampled(self._ctx, p, kind))

    # ---- geometric consistency ----
    def set_geom_depths(self, depths, weight: float = 0.2, clip: float = 3.0):
        """install the source views' depth maps for the geometric-consistency term (tsar_set_geom_depths): depths[v] is view v's
        [h, w] depth in its own camera (numpy or torch; <= 0 = no estimate) or None (no term for v); depths[0] is ignored.
        weight = lambda, clip = tau in pixels (ACMM's defaults)."""
        bufs = [_buf(d if v else None, np.float32, (self.h, self.w), "depth map %d" % v, tensors="any", typed=False) for v, d in enumerate(depths)]
        n = len(bufs)
        self._chk(self.L.tsar_set_geom_depths(self._ctx, n, _ptr_array(bufs, n), _one_kind(bufs, "all depth maps"), float(weight), float(clip)))

    def clear_geom(self):
        """remove the geometric-consistency term (tsar_clear_geom)"""
        self._chk(self.L.tsar_clear_geom(self._ctx))

    def rescore(self):
        """score the current planes with the context's cost, the geometric term included; pixels whose plane is not a valid hypothesis
        get tsar_pm_init's draw (tsar_pm_rescore)"""
        self._chk(self.L.tsar_pm_rescore(self._ctx))

    def get_geom_matrices(self, view: int):
        """(forward, back): the two float32 3 x 4 matrices of view's geometric term as the kernels read them (include/tsar.h)"""
        f = np.empty((3, 4), np.float32)
        b = np.empty((3, 4), np.float32)
        self._chk(self.L.tsar_get_geom_matrices(self._ctx, view, _ptr(f)[0], _ptr(b)[0]))
        return f, b

    # ---- plane prior ----
    def set_plane_prior(self, depth, normal_world, weight_depth: float = 0.1, weight_normal: float = 0.05, depth_clip: float = 0.02,
                        angle_clip_deg: float = 30.0):
        """install a per-pixel prior plane (tsar_set_plane_prior): depth [h, w] and unit world normals [h, w, 3], numpy arrays or torch
        device tensors; a pixel whose depth is not in (0, inf) or whose normal is not finite has no prior.  Every plane-scoring entry then
        adds weight_depth * min(|D - Dp| / Dp / depth_clip, 1) + weight_normal * min((1 - n.q) / normal_clip, 1) to a valid hypothesis's
        cost, normal_clip = 1 - cos(angle_clip_deg) rounded once from float64.  The struct passed is kept as plane_prior_params."""
        d = _buf(depth, np.float32, (self.h, self.w), "the prior's depth", tensors="any", typed=False)
        n = _buf(normal_world, np.float32, (self.h, self.w, 3), "the prior's normal_world", tensors="any", typed=False)
        p = PlanePriorParams(float(weight_depth), float(weight_normal), float(depth_clip), float(1.0 - np.cos(np.deg2rad(np.float64(angle_clip_deg)))))
        self._chk(self.L.tsar_set_plane_prior(self._ctx, d[1], n[1], _one_kind((d, n), "depth and normal_world"), C.byref(p)))
        self.plane_prior_params = p

    def clear_plane_prior(self):
        """remove the plane prior (tsar_clear_plane_prior)"""
        self._chk(self.L.tsar_clear_plane_prior(self._ctx))
        self.plane_prior_params = None

    def get_plane_prior(self):
        """the prior as the context holds it: [h, w, 4] float32 (normal in reference-camera coordinates, depth), all zero where the pixel has none"""
        out = np.empty((self.h, self.w, 4), np.float32)
        self._chk(self.L.tsar_get_plane_prior(self._ctx, _ptr(out)[0], MEM_HOST))
        return out

    def build_plane_prior(self, depth, score=None, cell: int = 4, max_levels: int = 0, want=("depth", "normal", "level"), device: bool = False):
        """a plane prior built from a checked depth map (tsar_build_plane_prior): depth [h, w] float32 is the filtered map, 0 where a
        pixel was dropped (geom_check's "depth"); score [h, w] float32 or None, lower is better (a stored cost).  A lattice of cells of
        edge cell << level keeps each cell's best candidate, neighbouring candidates span triangles, and every pixel gets the plane of
        the first triangle that contains it, finest level first (max_levels = 0: every level that fits).  Inputs are numpy arrays or
        torch device tensors (both the same).  Returns a dict with "depth" ([h, w] float32), "normal" ([h, w, 3] float32 world normals:
        what set_plane_prior takes) and / or "level" ([h, w] uint8, 255 = no prior; depth and normal are 0 there), as `want` names
        them: torch tensors on the device when the inputs are, or with device=True; numpy arrays otherwise.  Nothing in the context
        changes."""
        bufs = [_buf(a, np.float32, (self.h, self.w), name, tensors="device") for a, name in ((depth, "the depth map"), (score, "the score"))]
        kind = _one_kind(bufs, "depth and score")
        if device and kind == MEM_HOST:
            import torch
            dev = torch.device("cuda", self.device)
            bufs = [_buf(None if a is None else torch.from_numpy(a).to(dev), np.float32, tensors="device") for a, _, _ in bufs]
            kind = _one_kind(bufs, "depth and score")
        (depth, d, _), (score, s, _) = bufs
        res = _outputs({"depth": ((self.h, self.w), np.float32), "normal": ((self.h, self.w, 3), np.float32), "level": ((self.h, self.w), np.uint8)},
                       want, depth.device if kind == MEM_DEVICE else None)
        p = PlanePriorBuildParams(int(cell), int(max_levels))
        self._chk(self.L.tsar_build_plane_prior(self._ctx, d, s, kind, C.byref(p), _ptr(res.get("depth"))[0],
                                                _ptr(res.get("normal"))[0], _ptr(res.get("level"))[0]))
        return res

    # ---- the geometric-consistency pass coarse to fine ----
    def geom_pyramid_from(self, fine: "Matcher"):
        """install fine's term one level down (tsar_geom_pyramid): this context must hold fine's views from pyramid_from"""
        self._chk(self.L.tsar_geom_pyramid(self._ctx, fine._ctx))

    def pyramid_planes_from(self, fine: "Matcher"):
        """start this context's plane state from fine's planes at (2x, 2y), rescored with this context's cost (tsar_pyramid_planes)"""
        self._chk(self.L.tsar_pyramid_planes(self._ctx, fine._ctx))

    def upsample_merge(self, coarse: "Matcher"):
        """each pixel keeps the cheapest of its own plane and its four nearest coarse planes, the own plane winning ties
        (tsar_upsample_merge)"""
        self._chk(self.L.tsar_upsample_merge(self._ctx, coarse._ctx))

    # ---- the geometric-consistency check on its own ----
    def geom_check(self, depth=None, reproj_error: float = 2.0, depth_diff: float = 0.01, min_consistent: int = 2, want=("count", "depth")):
        """which pixels of `depth` ([h, w], the reference view's map; None = the context's own result) do the installed source maps
        confirm (tsar_geom_check; set_geom_depths installs the maps, weight 0 for checking only)?  Returns a dict with "count" ([h, w]
        uint8: the number of consistent source views) and / or "depth" ([h, w] float32: `depth` where count >= min_consistent, else 0),
        as `want` names them: numpy arrays, or torch tensors on depth's device when depth is a torch device tensor.  The mask itself
        is left in the context (get_reliable_mask)."""
        p = GeomCheckParams(float(reproj_error), float(depth_diff), int(min_consistent))
        depth, d, kind = _buf(depth, np.float32, (self.h, self.w), "the depth map", tensors="device")
        res = _outputs({"count": ((self.h, self.w), np.uint8), "depth": ((self.h, self.w), np.float32)}, want, depth.device if kind == MEM_DEVICE else None)
        self._chk(self.L.tsar_geom_check(self._ctx, d, C.byref(p), _ptr(res.get("count"))[0], _ptr(res.get("depth"))[0], kind))
        return res

    # ---- the sources' maps rendered into the reference camera, and offered to the matcher ----
    def geom_reproject(self, depth_diff: float = 0.01, min_views: int = 1, want=("depth", "count"), device: bool = False):
        """the installed source maps rendered into the reference camera (tsar_geom_reproject; set_geom_depths installs the maps, weight 0
        for this only): per pixel the front-most depth Z that lands there and the number of views with a landing within depth_diff * Z of
        it.  Returns a dict with "depth" ([h, w] float32: Z where count >= min_views, else 0) and / or "count" ([h, w] uint8), as `want`
        names them: numpy arrays, or torch tensors on the context's device with device=True.  Nothing in the context changes."""
        p = GeomReprojectParams(float(depth_diff), int(min_views))
        target = None
        if device:
            import torch
            target = torch.device("cuda", self.device)
        res = _outputs({"depth": ((self.h, self.w), np.float32), "count": ((self.h, self.w), np.uint8)}, want, target)
        self._chk(self.L.tsar_geom_reproject(self._ctx, C.byref(p), _ptr(res.get("depth"))[0], _ptr(res.get("count"))[0], MEM_DEVICE if device else MEM_HOST))
        return res

    def merge_depths(self, depth) -> int:
        """offer `depth` ([h, w] float32 in the reference camera, numpy or a torch device tensor; values outside [depth_min, depth_max] or
        not finite offer nothing) to the matcher (tsar_pm_merge_depths): the state is rescored, and each pixel takes the plane with its
        own normal through the offered depth where that scores strictly lower.  Returns the number of pixels that took it."""
        depth, d, kind = _buf(depth, np.float32, (self.h, self.w), "the depth map", tensors="device")
        taken = C.c_int64(0)
        self._chk(self.L.tsar_pm_merge_depths(self._ctx, d, kind, C.byref(taken)))
        return int(taken.value)

    def get_result(self, want=("depth", "normal", "cost", "confid"), pinned=False, out=None):
        """pinned=True: the result arrays are page-locked (tsar_host_alloc), so the D2H copies run at PCIe rate.
        out: dict of caller-owned arrays to fill instead (e.g. page-locked ones allocated once and reused per view)."""
        spec = {k: ((self.h, self.w, 3) if k == "normal" else (self.h, self.w), np.float32) for k in ("depth", "normal", "cost", "confid")}
        if out is None:
            res = _outputs(spec, want, empty=pinned_empty if pinned else np.empty)
        else:
            res = {k: out[k] for k in spec if k in out}
            for k, a in res.items():
                assert a.dtype == np.float32 and tuple(a.shape) == spec[k][0] and a.flags["C_CONTIGUOUS"]
        self._chk(self.L.tsar_get_result(self._ctx, _ptr(res.get("depth"))[0], _ptr(res.get("normal"))[0], _ptr(res.get("cost"))[0],
                                         _ptr(res.get("confid"))[0], MEM_HOST))
        return res

    def get_result_device(self, depth=None, normal=None, cost=None, confid=None):
        """Write results into caller-provided torch CUDA tensors."""
        self._chk(self.L.tsar_get_result(self._ctx, _ptr(depth)[0], _ptr(normal)[0], _ptr(cost)[0], _ptr(confid)[0], MEM_DEVICE))

    # ---- TSAR refinement ----
    def set_reliable_mask(self, scale):
        s = np.ascontiguousarray(scale, np.float32)
        self._chk(self.L.tsar_set_reliable_mask(self._ctx, _ptr(s)[0], MEM_HOST))

    def get_reliable_mask(self):
        s = np.empty((self.h, self.w), np.float32)
        self._chk(self.L.tsar_get_reliable_mask(self._ctx, _ptr(s)[0], MEM_HOST))
        return s

    def lrdiff(self):
        self._chk(self.L.tsar_lrdiff(self._ctx))

    # ---- self-tests ----
    def selftest_divide(self, X, Y, Z, ieee: bool = False, mode: int | None = None):
        """(u, v) = (X / Z, Y / Z) as strict mode's tap loops compute them (mode 0); as the device's IEEE division does (ieee /
        mode 1); as the fast mode computes them, X * v_rcp_f32(Z) (mode 2)."""
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, Y, Z))
        assert X.shape == Y.shape == Z.shape
        u, v = np.empty_like(X), np.empty_like(X)
        self._chk(self.L.tsar_selftest_divide(self._ctx, _ptr(X)[0], _ptr(Y)[0], _ptr(Z)[0], X.size, _ptr(u)[0], _ptr(v)[0], int(ieee) if mode is None else mode))
        return u, v

    def selftest_sqrt(self, mode: int, seed: int = 0) -> int:
        """mismatches of the cost tail's square root (sqrt_rsq_exact) against sqrtf on the device; mode 0: all 2^24 mantissa / parity cases"""
        bad = C.c_uint64(0)
        self._chk(self.L.tsar_selftest_sqrt(self._ctx, mode, seed, C.byref(bad)))
        return bad.value

    def selftest_sweep_census(self, colour: int) -> dict:
        out = (C.c_uint64 * 8)()
        self._chk(self.L.tsar_selftest_sweep_census(self._ctx, colour, out))
        keys = ("waves", "arms_any_lane", "max_lane_survivors", "max_lane_survivors_nodup", "lane_survivors", "lane_survivors_nodup", "pixels", "arms_present")
        return dict(zip(keys, [int(v) for v in out]))

    def selftest_prune_census(self, on: bool):
        """on: start counting in the sweeps that follow; off: stop and return [step][checked, views, views_left, repeats] (8 x 4)"""
        if on:
            self._chk(self.L.tsar_selftest_prune_census(self._ctx, 1, None))
            return None
        out = (C.c_uint32 * 32)()
        self._chk(self.L.tsar_selftest_prune_census(self._ctx, 0, out))
        return np.array(out, np.int64).reshape(8, 4)

    def selftest_divide_random(self, log2_triples: int, seed: int, mode: int, guarded: bool = True):
        """(quotients differing from IEEE division, triples outside the operand guard) over 2^log2_triples device-generated triples."""
        bad, out = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.tsar_selftest_divide_random(self._ctx, log2_triples, seed, mode, int(guarded), C.byref(bad), C.byref(out)))
        return bad.value, out.value

    # one stage of tsar_slic on host arrays (include/tsar.h tsar_selftest_slic_stage); centres are SPIXEL_DTYPE records
    def _slic_stage(self, stage, w, h, mw, mh, settings, in0, in1, inout):
        p1 = _ptr(in1)[0] if in1 is not None else None
        self._chk(self.L.tsar_selftest_slic_stage(self._ctx, stage, w, h, mw, mh, C.byref(settings), _ptr(in0)[0], p1, _ptr(inout)[0]))
        return inout

    def slic_convert(self, bgra, color_space=0):
        img = np.ascontiguousarray(bgra, np.uint8).reshape(-1, 4)
        return self._slic_stage(0, img.shape[0], 1, 0, 0, SlicSettings(20, 0, 5.0, 0, color_space), img, None, np.zeros((img.shape[0], 4), np.float32))

    def slic_init_centers(self, lab, mw, mh, S):
        lab = np.ascontiguousarray(lab, np.float32)
        h, w = lab.shape[:2]
        return self._slic_stage(1, w, h, mw, mh, SlicSettings(S, 0, 5.0, 0, 0), lab, None, np.zeros(mw * mh, SPIXEL_DTYPE))

    def slic_find_association(self, lab, centres, mw, mh, S, weight, labels_before=None):
        lab = np.ascontiguousarray(lab, np.float32)
        h, w = lab.shape[:2]
        labels = np.zeros((h, w), np.int32) if labels_before is None else np.ascontiguousarray(labels_before, np.int32).copy()
        return self._slic_stage(2, w, h, mw, mh, SlicSettings(S, 0, weight, 0, 0), lab, np.ascontiguousarray(centres), labels)

    def slic_update_centers(self, lab, labels, S):
        lab = np.ascontiguousarray(lab, np.float32)
        h, w = lab.shape[:2]
        return self._slic_stage(3, w, h, w // S, h // S, SlicSettings(S, 0, 5.0, 0, 0), lab, np.ascontiguousarray(labels, np.int32), np.zeros((w // S) * (h // S), SPIXEL_DTYPE))

    def slic_connectivity(self, labels):
        labels = np.ascontiguousarray(labels, np.int32)
        h, w = labels.shape
        return self._slic_stage(4, w, h, 0, 0, SlicSettings(20, 0, 5.0, 0, 0), labels, None, np.zeros((h, w), np.int32))

    def getview(self):
        self._chk(self.L.tsar_getview(self._ctx))

    def wmf(self, iters: int, final_pass: bool):
        self._chk(self.L.tsar_wmf(self._ctx, iters, int(final_pass)))

    def set_regions(self, labels, region_text, region_size=None):
        tx = np.ascontiguousarray(region_text, np.float32)
        sz = np.ascontiguousarray(region_size, np.float32) if region_size is not None else None
        if _is_torch(labels) and labels.is_cuda:
            # labels on the device; the (small) region tables travel to the device the same way
            import torch
            assert labels.dtype == torch.int32
            txd = torch.from_numpy(tx).to(labels.device)
            szd = torch.from_numpy(sz).to(labels.device) if sz is not None else None
            self._chk(self.L.tsar_set_regions(self._ctx, _ptr(labels)[0], len(tx), _ptr(txd)[0], _ptr(szd)[0], MEM_DEVICE))
        else:
            lb = np.ascontiguousarray(labels, np.int32)
            self._chk(self.L.tsar_set_regions(self._ctx, _ptr(lb)[0], len(tx), _ptr(tx)[0], _ptr(sz)[0], MEM_HOST))
        self.n_regions = len(tx)

    def detect_weak_texture(self, cap: int = 1 << 16, want_labels: bool = True):
        """-> (labels [h, w] int32, region_text [n], region_size [n]); also installs them as the regions.
        want_labels=False: labels_out = NULL, the call tsar_gipuma makes (the labels stay on the device for the next operators;
        no [h, w] int32 D2H copy) -> labels is None"""
        labels = np.empty((self.h, self.w), np.int32) if want_labels else None
        text = np.empty(cap, np.float32)
        size = np.empty(cap, np.float32)
        n = C.c_int(0)
        self._chk(self.L.tsar_detect_weak_texture(self._ctx, _ptr(labels)[0] if want_labels else None, MEM_HOST, C.byref(n), _ptr(text)[0], _ptr(size)[0], cap))
        self.n_regions = n.value
        k = min(n.value, cap)
        return labels, text[:k].copy(), size[:k].copy()

    def ransac_regions(self):
        planes = np.empty((self.n_regions, 4), np.float32)
        ratio = np.empty((self.n_regions,), np.float32)
        self._chk(self.L.tsar_ransac_regions(self._ctx, _ptr(planes)[0], _ptr(ratio)[0]))
        return planes, ratio

    def set_region_planes(self, planes):
        pl = np.ascontiguousarray(planes, np.float32)
        self._chk(self.L.tsar_set_region_planes(self._ctx, _ptr(pl)[0]))

    def fake_depth(self):
        out = np.empty((self.h, self.w), np.float32)
        self._chk(self.L.tsar_fake_depth(self._ctx, _ptr(out)[0], MEM_HOST))
        return out

    def fill_textureless(self):
        self._chk(self.L.tsar_fill_textureless(self._ctx))

    def slic(self, bgra, settings: SlicSettings | None = None):
        img = np.ascontiguousarray(bgra, np.uint8)
        h, w = img.shape[:2]
        if settings is None:
            settings = SlicSettings()
            self.L.tsar_default_slic_settings(C.byref(settings))
        labels = np.empty((h, w), np.int32)
        self._chk(self.L.tsar_slic(self._ctx, _ptr(img)[0], w, h, C.byref(settings), _ptr(labels)[0], MEM_HOST))
        return labels

    # ---- measurement ----
    @property
    def stream(self) -> int:
        s = C.c_void_p()
        self._chk(self.L.tsar_get_stream(self._ctx, C.byref(s)))
        return s.value or 0

    def synchronize(self):
        self._chk(self.L.tsar_synchronize(self._ctx))

    def enable_kernel_timing(self, on: bool = True):
        self._chk(self.L.tsar_enable_kernel_timing(self._ctx, int(on)))

    def reset_kernel_timing(self):
        self._chk(self.L.tsar_reset_kernel_timing(self._ctx))

    def kernel_timing(self):
        buf = (KernelTiming * 32)()
        n = C.c_int(0)
        self._chk(self.L.tsar_get_kernel_timing(self._ctx, buf, 32, C.byref(n)))
        return {buf[i].name.decode(): (buf[i].launches, buf[i].total_ms) for i in range(min(n.value, 32))}


def matcher_from_scene(scene, box=11, n_best=1, cost_comb=COMB_BEST_N, flags=0, seed=2024, device=0, subset=None, box_v=None) -> Matcher:
    """Convenience used by tests/bench: a Matcher loaded with a tsar_mvs_amd.synth.Scene."""
    m = Matcher(device)
    m.set_params(default_params(box_hsize=box, box_vsize=box if box_v is None else box_v, n_best=n_best, cost_comb=cost_comb, depth_min=scene.depth_min,
                                depth_max=scene.depth_max, flags=flags, seed=seed))
    m.set_views(scene.images, scene.K, scene.R, scene.t)
    if subset is not None:
        m.set_view_subset(subset)
    return m


def _pyramid_chain(matcher: Matcher, levels: int, coarse, prepare=None):
    """`coarse` (the coarse contexts of an earlier call, finest first, or None) grown to `levels` contexts, and the chain [matcher] +
    coarse[:levels] with matcher's views carried down it (pyramid_from); every context of the chain goes through `prepare` first
    (tsar_pyramid_views refuses a context that holds a term or a prior).  Returns (coarse, chain)."""
    coarse = list(coarse or [])
    while len(coarse) < levels:
        coarse.append(Matcher(matcher.device))
    chain = [matcher] + coarse[:levels]
    if prepare is not None:
        for m in chain:
            prepare(m)
    for finer, coarser in zip(chain[:-1], chain[1:]):
        coarser.pyramid_from(finer)
    return coarse, chain


def run_multiscale(matcher: Matcher, levels: int, coarse_iters: int, fine_iters: int, coarse=None):
    """Coarse-to-fine PatchMatch on `matcher`'s views: init + `coarse_iters` iterations at the coarsest of `levels` pyramid levels,
    then at every finer level (matcher's own included) upsample + `fine_iters` iterations.  levels = 0 is plain init + coarse_iters.
    coarse: the coarse contexts of an earlier call (finest first), reused; returns the list used, for the next call."""
    if levels < 0 or coarse_iters < 0 or fine_iters < 0:
        raise ValueError("levels and iteration counts must be >= 0")
    coarse, chain = _pyramid_chain(matcher, levels, coarse)
    chain[-1].pm_init()
    chain[-1].pm_iterate(coarse_iters)
    for k in range(levels - 1, -1, -1):
        chain[k].upsample_planes(chain[k + 1])
        chain[k].pm_iterate(fine_iters)
    return coarse


def _cross_view_merge(matcher: Matcher, cross_view: int, cross_view_depth_diff: float) -> int:
    """the sources' maps rendered into the reference camera (kept where `cross_view` views agree) and offered to the matcher, on the
    device; the merge rescores first, so it stands in for rescore()"""
    r = matcher.geom_reproject(cross_view_depth_diff, cross_view, want=("depth",), device=True)
    return matcher.merge_depths(r["depth"])


def _install_prior(matcher: Matcher, prior, prior_params):
    """prior = (depth, normal_world); prior_params = None (the defaults) or a dict of set_plane_prior's keyword arguments"""
    depth, normal_world = prior
    matcher.set_plane_prior(depth, normal_world, **(prior_params or {}))


_BUILD_PRIOR_KEYS = {"cell": "cell", "max_levels": "max_levels", "reproj_error": "check", "depth_diff": "check", "min_consistent": "check"}


def _check_geom_pass(counts, what, cross_view, cross_view_depth_diff, prior, prior_params, build_prior):
    """the argument checks of both geometric passes; counts: the pass's own iteration (and level) counts, `what` names them"""
    if any(c < 0 for c in counts):
        raise ValueError(what + " must be >= 0")
    if int(cross_view) != cross_view or not 0 <= cross_view <= MAX_VIEWS - 1:
        raise ValueError("cross_view must be an integer in 0..63")
    if cross_view and not (cross_view_depth_diff > 0 and np.isfinite(cross_view_depth_diff)):
        raise ValueError("cross_view_depth_diff must be finite and > 0")
    if prior is not None and build_prior is not None:
        raise ValueError("prior and build_prior are mutually exclusive")
    if prior is None and build_prior is None and prior_params is not None:
        raise ValueError("prior_params without a prior")
    if build_prior is not None and set(build_prior) - set(_BUILD_PRIOR_KEYS):
        raise ValueError("build_prior: unknown settings %s" % sorted(set(build_prior) - set(_BUILD_PRIOR_KEYS)))


def _build_prior(matcher: Matcher, own_depth, build_prior, prior_params):
    """the prior built from the view's own depth, after the maps are installed: rescore; the stored cost is the score; geom_check(own
    depth) keeps the confirmed depths; build_plane_prior; set_plane_prior; rescore again (installing a prior voids the costs).  The
    built maps stay on the device."""
    check = {k: v for k, v in build_prior.items() if _BUILD_PRIOR_KEYS[k] == "check"}
    build = {k: v for k, v in build_prior.items() if _BUILD_PRIOR_KEYS[k] != "check"}
    matcher.rescore()
    score = matcher.get_plane()[1]
    kept = matcher.geom_check(own_depth, want=("depth",), **check)["depth"]
    if _is_torch(kept) and kept.is_cuda:
        import torch
        score = torch.from_numpy(score).to(kept.device)
    built = matcher.build_plane_prior(kept, score, want=("depth", "normal"), device=True, **build)
    matcher.set_plane_prior(built["depth"], built["normal"], **(prior_params or {}))
    matcher.rescore()


def _open_geom_pass(matcher: Matcher, own_depth, own_normal_world, src_depths, weight, clip, cross_view, cross_view_depth_diff, prior, prior_params,
                    build_prior) -> bool:
    """the opening of both geometric passes on the full-resolution matcher: the view's own planes, the sources' maps, the prior (given
    or built), the cross-view merge.  Returns whether the planes are scored on the way out (_build_prior ends with a rescore, the merge
    begins with one)."""
    matcher.load_planes(own_depth, own_normal_world)
    matcher.set_geom_depths(src_depths, weight=weight, clip=clip)
    if prior is not None:
        _install_prior(matcher, prior, prior_params)
    if build_prior is not None:
        _build_prior(matcher, own_depth, build_prior, prior_params)
    if cross_view:
        _cross_view_merge(matcher, cross_view, cross_view_depth_diff)
    return bool(cross_view) or build_prior is not None


def run_geom_pass(matcher: Matcher, own_depth, own_normal_world, src_depths, iters: int, weight: float = 0.2, clip: float = 3.0,
                  cross_view: int = 0, cross_view_depth_diff: float = 0.01, prior=None, prior_params=None, build_prior=None):
    """The geometric-consistency pass of one reference view: start from its own photometric result (depth [h, w], world normals
    [h, w, 3]), install the source views' depth maps (src_depths[v] for view v of the matcher, [0] ignored, None = no term), rescore,
    run `iters` iterations with the term, compute_disp.  The term stays installed (clear_geom removes it).
    cross_view = K >= 1: in place of the rescore, the source maps are rendered into this view (geom_reproject with min_views = K and
    depth_diff = cross_view_depth_diff) and offered to the matcher (merge_depths, which rescores first).
    prior = (depth, normal_world): installed as the plane prior right after the maps (set_plane_prior; prior_params = its keyword
    arguments as a dict, None = the defaults); it stays installed too (clear_plane_prior removes it).
    build_prior = a dict (in place of prior): the prior is built from the view's own depth (_build_prior says how; the dict holds
    build_plane_prior's "cell" and "max_levels" and geom_check's "reproj_error", "depth_diff" and "min_consistent", each optional) and
    installed with prior_params."""
    term = (weight, clip, cross_view, cross_view_depth_diff, prior, prior_params, build_prior)
    _check_geom_pass((iters,), "iters", *term[2:])
    if not _open_geom_pass(matcher, own_depth, own_normal_world, src_depths, *term):
        matcher.rescore()
    matcher.pm_iterate(iters)
    matcher.compute_disp()


def run_geom_pass_multiscale(matcher: Matcher, own_depth, own_normal_world, src_depths, levels: int, coarse_iters: int, fine_iters: int,
                             weight: float = 0.2, clip: float = 3.0, coarse=None, cross_view: int = 0, cross_view_depth_diff: float = 0.01,
                             prior=None, prior_params=None, build_prior=None):
    """The geometric-consistency pass coarse to fine (include/tsar.h tsar_geom_pyramid): `levels` pyramid levels below `matcher`; the
    view's own result and the term are carried down the chain, `coarse_iters` iterations run at the coarsest level, then every finer
    level (matcher's own included) merges the coarser planes into its own and runs `fine_iters` iterations; compute_disp.  levels = 0
    is run_geom_pass(matcher, ..., fine_iters).  coarse: the coarse contexts of an earlier call (finest first), reused; returns the
    list used.  The terms stay installed (clear_geom removes them).
    cross_view = K >= 1: as in run_geom_pass, on the full-resolution matcher right after its term is installed and before the chain is
    carried down (the coarser levels then start from the merged planes).
    prior, prior_params: as in run_geom_pass, on the full-resolution matcher only (a prior is not carried to coarser levels: they score
    with their own cost); any prior the chain's contexts still hold is removed first, since tsar_pyramid_views refuses it.
    build_prior: as in run_geom_pass, on the full-resolution matcher only, right after its term is installed."""
    term = (weight, clip, cross_view, cross_view_depth_diff, prior, prior_params, build_prior)
    _check_geom_pass((levels, coarse_iters, fine_iters), "levels and iteration counts", *term[2:])
    if levels == 0:
        run_geom_pass(matcher, own_depth, own_normal_world, src_depths, fine_iters, *term)
        return list(coarse or [])
    def clear(m):
        m.clear_geom()
        if prior is not None or build_prior is not None:
            m.clear_plane_prior()
    coarse, chain = _pyramid_chain(matcher, levels, coarse, prepare=clear)
    _open_geom_pass(matcher, own_depth, own_normal_world, src_depths, *term)
    for finer, coarser in zip(chain[:-1], chain[1:]):
        coarser.geom_pyramid_from(finer)
        coarser.pyramid_planes_from(finer)
    chain[-1].pm_iterate(coarse_iters)
    for k in range(levels - 1, -1, -1):
        chain[k].upsample_merge(chain[k + 1])
        chain[k].pm_iterate(fine_iters)
    matcher.compute_disp()
    return coarse


def fuse(depths, normals, grays, K, R, t, pairs, params: FusionParams | None = None, cap: int | None = None, device: int = 0, matcher=None,
         return_count: bool = False):
    """Fuse per-view depth [h, w] / world-normal [h, w, 3] maps into a point cloud (tsar_fuse; with `matcher`, tsar_fuse_ctx on that
    context: its stream, temporaries from its scratch arena).
    pairs: {view: [source views]} or list of lists.  Returns an [n, 9] float32 array:
    x y z, nx ny nz, gray, number of agreeing views, reference view — a numpy array, or, when the maps are torch device tensors, a
    torch tensor on their device (include/tsar.h: `mem` names where the maps and points_out lie).  At most `cap` points are returned;
    return_count=True returns (points, number of points found), which may exceed cap."""
    L = load_library()
    n = len(depths)
    h, w = int(depths[0].shape[0]), int(depths[0].shape[1])
    if params is None:
        params = FusionParams()
        L.tsar_default_fusion_params(C.byref(params))
    maps = [[_buf(a, np.float32, shape, "%s map %d" % (name, i), tensors="any") for i, a in enumerate(seq)]
            for name, seq, shape in (("depth", depths, (h, w)), ("normal", normals, (h, w, 3)), ("gray", grays, (h, w)))]
    pd, pn, pg = (_ptr_array(bufs, n) for bufs in maps)
    mem = _one_kind(sum(maps, []), "all maps")
    lists = [list(pairs[v]) for v in range(n)]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    idx = np.asarray([s for x in lists for s in x] or [0], np.int32)
    if cap is None:
        cap = n * h * w
    if mem == MEM_DEVICE:
        # device maps: the cloud is delivered on their device as well, never into a host array
        import torch
        out = torch.empty((max(cap, 1), 9), dtype=torch.float32, device=maps[0][0][0].device)
    else:
        out = np.empty((cap, 9), np.float32)
    out_ptr = _ptr(out)[0]
    cnt = C.c_int64(0)
    tail = (n, w, h, _cameras(K, R, t, n), pd, pn, pg, mem, off.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), C.byref(params),
            out_ptr, cap, C.byref(cnt))
    rc = L.tsar_fuse_ctx(matcher._ctx, *tail) if matcher is not None else L.tsar_fuse(device, *tail)
    if rc != TSAR_OK:
        raise TsarError(rc, L.tsar_last_error(matcher._ctx).decode() if matcher is not None else "tsar_fuse failed")
    pts = out[: min(cnt.value, cap)]
    pts = pts.clone() if mem == MEM_DEVICE else pts.copy()
    return (pts, int(cnt.value)) if return_count else pts


def _cloud(a, name):
    """an [n, k >= 3] float32 cloud as the library takes it: a contiguous numpy array, or a contiguous torch device tensor"""
    a = _coerce(a, np.float32, None, name, tensors="device")
    assert a.ndim == 2 and a.shape[1] >= 3 and (not _is_torch(a) or a.is_contiguous()), name + " must be a contiguous [n, k >= 3] array or tensor"
    return a, _is_torch(a)


@contextlib.contextmanager
def _matcher_for(matcher, device, *inputs):
    """the caller's Matcher; without one, a Matcher made for the block and closed after it, on the device of the first torch device
    tensor among `inputs`, else on `device`"""
    if matcher is not None:
        yield matcher
        return
    m = Matcher(next((a.device.index for a in inputs if _is_torch(a) and a.is_cuda and a.device.index is not None), device))
    try:
        yield m
    finally:
        m.close()


def _error_with_pairs(rc, L, m, pairs):
    """the TsarError of a refused cloud_distance / cloud_neighbors call; .pairs is filled when max_pairs refused it, else None"""
    err = TsarError(rc, L.tsar_last_error(m._ctx).decode())
    err.pairs = int(pairs.value) if pairs.value >= 0 else None
    return err


def cloud_distance(query, target, max_dist, tolerances=None, want=("dist2", "index"), max_pairs=None, matcher=None, device=0):
    """For every point of `query` the squared float32 distance to its nearest point of `target` within max_dist, and that point's index
    (tsar_cloud_distance_ctx; include/tsar.h states the arithmetic).  query, target: [n, k >= 3] float32, x y z first, both numpy arrays
    or both torch device tensors (a fused cloud as api.fuse returns it goes in as it is: the stride is k).  Records with a non-finite
    coordinate take no part.  tolerances: a sequence of distances, each in (0, max_dist].  max_pairs: the call is refused (TsarError,
    TSAR_ERR_INVALID) when it would evaluate more (query, target) pairs; None = the library's default.  matcher: run on that context
    (its device and stream; nothing in it changes); without one a context is created on `device` for the call.
    Returns a dict: "dist2" ([n_query] float32, +inf where nothing lies within max_dist) and / or "index" ([n_query] int32, -1 there), as
    `want` names them (numpy arrays, or torch tensors on the inputs' device); "within" (int64 numpy array: per tolerance the number of
    queries with dist2 <= fl(tol * tol)); "n_valid_query" (queries with finite coordinates); "pairs" (pairs evaluated)."""
    L = load_library()
    q, q_dev = _cloud(query, "query")
    t, t_dev = _cloud(target, "target")
    assert q_dev == t_dev, "query and target must live in the same memory space"
    if q_dev:
        assert q.device == t.device, "query and target must live on one device"
    p = CloudDistanceParams()
    L.tsar_default_cloud_distance_params(C.byref(p))
    p.max_dist = float(max_dist)
    if max_pairs is not None:
        p.max_pairs = int(max_pairs)
    tol = np.ascontiguousarray([] if tolerances is None else tolerances, np.float32).reshape(-1)
    within = np.zeros(len(tol), np.int64)
    nq = int(q.shape[0])
    res = _outputs({"dist2": ((nq,), np.float32), "index": ((nq,), np.int32)}, want, q.device if q_dev else None)
    n_valid, pairs = C.c_int64(0), C.c_int64(-1)
    with _matcher_for(matcher, device, q) as m:
        rc = L.tsar_cloud_distance_ctx(m._ctx, _ptr(q)[0] if nq else None, nq, int(q.shape[1]), _ptr(t)[0] if t.shape[0] else None, int(t.shape[0]), int(t.shape[1]),
                                       C.byref(p), len(tol), tol.ctypes.data_as(C.c_void_p), _ptr(res.get("dist2"))[0], _ptr(res.get("index"))[0],
                                       within.ctypes.data_as(C.c_void_p), C.byref(n_valid), C.byref(pairs), MEM_DEVICE if q_dev else MEM_HOST)
        if rc != TSAR_OK:
            raise _error_with_pairs(rc, L, m, pairs)
    res["within"] = within
    res["n_valid_query"] = int(n_valid.value)
    res["pairs"] = int(pairs.value)
    return res


def cloud_voxels(cloud, voxel, dist2=None, tolerances=None, want=("rank", "rep", "count"), matcher=None, device=0):
    """A voxel grid of edge `voxel` over `cloud` (tsar_cloud_voxels_ctx; include/tsar.h states the arithmetic).  cloud: [n, k >= 3] float32, x y z
    first, a numpy array or a torch device tensor; records with a non-finite coordinate take no part.  The occupied voxels are numbered in
    ascending order of their key z << 42 | y << 21 | x.  dist2 ([n] float32, in the cloud's memory space: cloud_distance's output for this
    cloud) and tolerances go together: with them the dict holds "within".  matcher / device: as cloud_distance.
    Returns a dict: "rank" ([n] int32: the voxel of every point, -1 for a non-candidate), "rep" ([n_voxels] int32: the index of the point
    nearest the voxel's centre, the smallest index among equals), "count" ([n_voxels] int32), as `want` names them; "within" ([n_voxels,
    n_tol] int32: per voxel and tolerance the points with dist2 <= fl(tol * tol)) when tolerances are given; the integers "n_voxels" and
    "n_valid".  Arrays are numpy arrays, or torch tensors on the cloud's device."""
    L = load_library()
    c, dev = _cloud(cloud, "cloud")
    n = int(c.shape[0])
    tol = np.ascontiguousarray([] if tolerances is None else tolerances, np.float32).reshape(-1)
    assert (dist2 is None) == (tolerances is None), "dist2 and tolerances go together"
    d2 = _coerce(dist2.cpu() if _is_torch(dist2) and not dev else dist2, np.float32, (n,), "dist2", tensors="device")
    assert d2 is None or not dev or (_is_torch(d2) and d2.device == c.device and d2.is_contiguous()), "dist2 must be a contiguous tensor on the cloud's device"
    p = CloudVoxelsParams()
    L.tsar_default_cloud_voxels_params(C.byref(p))
    p.voxel = float(voxel)
    spec = {k: ((n,), np.int32) for k in ("rank", "rep", "count")}             # at most n voxels: the per-voxel arrays are trimmed below
    if tolerances is not None:
        spec["within"] = ((n, len(tol)), np.int32)
    out = _outputs(spec, tuple(want) + ("within",), c.device if dev else None)
    n_voxels, n_valid = C.c_int64(0), C.c_int64(0)
    with _matcher_for(matcher, device, c) as m:
        rc = L.tsar_cloud_voxels_ctx(m._ctx, _ptr(c)[0] if n else None, n, int(c.shape[1]), C.byref(p), _ptr(d2)[0], len(tol),
                                     tol.ctypes.data_as(C.c_void_p) if tolerances is not None else None, _ptr(out.get("rank"))[0], n, _ptr(out.get("rep"))[0],
                                     _ptr(out.get("count"))[0], _ptr(out.get("within"))[0] if len(tol) else None, C.byref(n_voxels), C.byref(n_valid),
                                     MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            raise TsarError(rc, L.tsar_last_error(m._ctx).decode())
    nv = int(n_voxels.value)
    for k in ("rep", "count", "within"):
        if k in out:
            out[k] = out[k][:nv].clone() if dev else out[k][:nv].copy()
    out["n_voxels"] = nv
    out["n_valid"] = int(n_valid.value)
    return out


def voxel_downsample(cloud, voxel, matcher=None, device=0):
    """`cloud` thinned to one point per occupied voxel of edge `voxel`: the rows sorted(rep) of cloud_voxels — every voxel's point nearest its
    centre, whole records (normals, colours), in the cloud's own order.  Returns an array or tensor like `cloud`."""
    c, dev = _cloud(cloud, "cloud")
    rep = cloud_voxels(c, voxel, want=("rep",), matcher=matcher, device=device)["rep"]
    if dev:
        return c[rep.sort().values.long()].clone()
    return c[np.sort(rep)].copy()


def cloud_neighbors(cloud, radius, k=0, want=("count", "knn_dist2"), max_pairs=None, matcher=None, device=0):
    """Per point of `cloud` the number of its other points within `radius`, and the k smallest squared float32 distances among those
    (tsar_cloud_neighbors_ctx; include/tsar.h states the arithmetic).  cloud: [n, c >= 3] float32, x y z first, a numpy array or a torch
    device tensor; records with a non-finite coordinate take no part.  The point itself is left out by its index, so a duplicate of it
    counts, at distance 0.  k: 0 .. 32; 0 = counts only ("knn_dist2" is then not returned).  max_pairs: the call is refused (TsarError,
    TSAR_ERR_INVALID, with .pairs) when it would look at more pairs; None = the library's default.  matcher / device: as cloud_distance.
    Returns a dict: "count" ([n] int32, -1 for a non-candidate) and / or "knn_dist2" ([n, k] float32, ascending, +inf where fewer than k
    points lie within radius), as `want` names them (numpy arrays, or torch tensors on the cloud's device); the integers "n_valid"
    (records with finite coordinates) and "pairs" (pairs looked at)."""
    L = load_library()
    c, dev = _cloud(cloud, "cloud")
    n, k = int(c.shape[0]), int(k)
    p = CloudNeighborsParams()
    L.tsar_default_cloud_neighbors_params(C.byref(p))
    p.radius, p.k = float(radius), k
    if max_pairs is not None:
        p.max_pairs = int(max_pairs)
    spec = {"count": ((n,), np.int32)}
    if k > 0:
        spec["knn_dist2"] = ((n, k), np.float32)
    res = _outputs(spec, want, c.device if dev else None)
    n_valid, pairs = C.c_int64(0), C.c_int64(-1)
    with _matcher_for(matcher, device, c) as m:
        rc = L.tsar_cloud_neighbors_ctx(m._ctx, _ptr(c)[0] if n else None, n, int(c.shape[1]), C.byref(p), _ptr(res.get("count"))[0], _ptr(res.get("knn_dist2"))[0],
                                        C.byref(n_valid), C.byref(pairs), MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            raise _error_with_pairs(rc, L, m, pairs)
    res["n_valid"] = int(n_valid.value)
    res["pairs"] = int(pairs.value)
    return res


_ORIENT = {None: 0, "viewpoint": 1, "record": 2}


def cloud_normals(cloud, radius, k=16, min_neighbors=5, orient=None, viewpoint=None, want=("normal", "curvature"), max_pairs=None, matcher=None, device=0):
    """Per point of `cloud` its k nearest neighbours within `radius` and the PCA normal and surface variation of that neighbourhood
    (tsar_cloud_normals_ctx; include/tsar.h states the arithmetic).  cloud: [n, c >= 3] float32, x y z first, a numpy array or a torch
    device tensor (a fused cloud as api.fuse returns it goes in as it is); records with a non-finite coordinate take no part.  k: 3 .. 32;
    a point with fewer than min_neighbors (2 .. k) neighbours within radius gets no normal.  orient: None = the canonical sign (the
    component of largest magnitude is positive), "viewpoint" = towards `viewpoint` (three finite numbers), "record" = along the record's
    own normal, floats 3 .. 5 (c >= 6).  max_pairs, matcher / device: as cloud_neighbors.
    This is the plain PCA normal: no orientation is propagated across the cloud and nothing is meshed.
    Returns a dict: "normal" ([n, 3] float32, 0 0 0 without a normal), "curvature" ([n] float32, -1 without), "knn_index" ([n, k] int32,
    nearest first, -1 padded), "n_used" ([n] int32: the neighbours used, -1 for a non-candidate), "cov" ([n, 6] float64: xx xy xz yy yz zz),
    as `want` names them (numpy arrays, or torch tensors on the cloud's device); the integers "n_valid", "n_normals" and "pairs"."""
    L = load_library()
    c, dev = _cloud(cloud, "cloud")
    n, k = int(c.shape[0]), int(k)
    assert orient in _ORIENT, "orient must be None, \"viewpoint\" or \"record\""
    assert (orient == "viewpoint") == (viewpoint is not None), "viewpoint goes with orient=\"viewpoint\""
    p = CloudNormalsParams()
    L.tsar_default_cloud_normals_params(C.byref(p))
    p.radius, p.k, p.min_neighbors, p.orient = float(radius), k, int(min_neighbors), _ORIENT[orient]
    if viewpoint is not None:
        p.viewpoint[:] = [float(v) for v in np.asarray(viewpoint, np.float32).reshape(3)]
    if max_pairs is not None:
        p.max_pairs = int(max_pairs)
    spec = {"knn_index": ((n, max(k, 0)), np.int32), "n_used": ((n,), np.int32), "normal": ((n, 3), np.float32), "curvature": ((n,), np.float32),
            "cov": ((n, 6), np.float64)}
    res = _outputs(spec, want, c.device if dev else None)
    n_valid, n_normals, pairs = C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    with _matcher_for(matcher, device, c) as m:
        rc = L.tsar_cloud_normals_ctx(m._ctx, _ptr(c)[0] if n else None, n, int(c.shape[1]), C.byref(p), *(_ptr(res.get(key))[0] for key in spec), C.byref(n_valid),
                                      C.byref(n_normals), C.byref(pairs), MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            raise _error_with_pairs(rc, L, m, pairs)
    res["n_valid"] = int(n_valid.value)
    res["n_normals"] = int(n_normals.value)
    res["pairs"] = int(pairs.value)
    return res


def min_cos_of(tolerances_deg):
    """the thresholds tsar_cloud_normal_compare takes for angles in degrees: one float64 cos each"""
    return np.cos(np.deg2rad(np.ascontiguousarray(tolerances_deg, np.float64).reshape(-1)))


def normal_compare(normal_a, normal_b, index, tolerances_deg, dist2=None, max_dist=None, signed=False, want_cos=False, matcher=None, device=0):
    """The normals of cloud a scored against those of cloud b (tsar_cloud_normal_compare_ctx; include/tsar.h).  normal_a: [n, c >= 3] float32,
    the normal in the first three columns; normal_b: [n_b, c >= 3]; index: [n] int32, per row of a the row of b to compare with or -1
    (cloud_distance's "index"); dist2 ([n] float32) with max_dist: only rows with dist2 <= fl(max_dist * max_dist) are compared.  All numpy
    arrays or all torch tensors on one device.  tolerances_deg: up to 16 angles in degrees, each turned into a threshold with one float64 cos.
    A row is compared iff its index names a row of b, its dist2 passes, and both normals are finite and not zero; signed=False compares
    lines (|cos|), signed=True directions.
    Returns a dict: "n_compared"; "within" (int64 array: per tolerance the compared rows whose angle is within it); "tolerances_deg"; "min_cos";
    "accuracy" (float64: within / n_compared, 0 where nothing is compared); with want_cos "cos" ([n] float32, NaN where not compared)."""
    L = load_library()
    a, dev = _cloud(normal_a, "normal_a")
    b, b_dev = _cloud(normal_b, "normal_b")
    n = int(a.shape[0])
    assert dev == b_dev and (not dev or a.device == b.device), "normal_a and normal_b must live in the same memory space"
    assert (dist2 is None) == (max_dist is None), "dist2 and max_dist go together"
    side = lambda x: x.cpu() if _is_torch(x) and not dev else x
    idx = _coerce(side(index), np.int32, (n,), "index", tensors="device")
    d2 = _coerce(side(dist2), np.float32, (n,), "dist2", tensors="device")
    for x, name in ((idx, "index"), (d2, "dist2")):
        assert x is None or not dev or (_is_torch(x) and x.device == a.device and x.is_contiguous()), name + " must be a contiguous tensor on the normals' device"
    deg = np.ascontiguousarray(tolerances_deg, np.float64).reshape(-1)
    mc = min_cos_of(deg)
    within = np.zeros(len(mc), np.int64)
    out = _outputs({"cos": ((n,), np.float32)}, ("cos",) if want_cos else (), a.device if dev else None)
    n_cmp = C.c_int64(0)
    with _matcher_for(matcher, device, a) as m:
        rc = L.tsar_cloud_normal_compare_ctx(m._ctx, _ptr(a)[0] if n else None, int(a.shape[1]), n, _ptr(b)[0] if b.shape[0] else None, int(b.shape[1]), int(b.shape[0]),
                                             _ptr(idx)[0] if n else None, _ptr(d2)[0] if n else None, 0.0 if max_dist is None else float(max_dist), len(mc),
                                             mc.ctypes.data_as(C.c_void_p), 1 if signed else 0, _ptr(out.get("cos"))[0], within.ctypes.data_as(C.c_void_p), C.byref(n_cmp),
                                             MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            raise TsarError(rc, L.tsar_last_error(m._ctx).decode())
    nc = int(n_cmp.value)
    res = {"n_compared": nc, "within": within, "tolerances_deg": deg, "min_cos": mc,
           "accuracy": within / np.float64(nc) if nc else np.zeros(len(mc), np.float64)}
    res.update(out)
    return res


def _outlier_settings(radius, min_neighbors, k, ratio):
    """the settings of remove_outliers as (float, int or None, int or None, float); ValueError on what the tools refuse as well"""
    radius, ratio = float(radius), float(ratio)
    if min_neighbors is None and k is None:
        raise ValueError("outlier removal needs min_neighbors, k or both")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be a finite number > 0")
    if min_neighbors is not None and int(min_neighbors) < 1:
        raise ValueError("min_neighbors must be at least 1")
    if k is not None and not 1 <= int(k) <= 32:
        raise ValueError("k must be in 1..32")
    if not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("ratio must be a finite number > 0")
    return radius, None if min_neighbors is None else int(min_neighbors), None if k is None else int(k), ratio


def _outlier_mask(c, dev, radius, min_neighbors, k, ratio, matcher, device):
    """the keep mask of remove_outliers over the rows of the cloud c (_cloud's), a bool numpy array or tensor like c"""
    res = cloud_neighbors(c, radius, k or 0, want=("count",) + (("knn_dist2",) if k else ()), matcher=matcher, device=device)
    keep = res["count"] >= (0 if min_neighbors is None else min_neighbors)              # count is -1 for a non-candidate
    if k:
        s = res["knn_dist2"][:, k - 1]
        if dev:
            import torch
            finite = s[torch.isfinite(s)]
            m = int(finite.numel())
            med = float(torch.kthvalue(finite, (m - 1) // 2 + 1).values.item()) if m else None
        else:
            finite = s[np.isfinite(s)]
            m = int(finite.size)
            med = np.partition(finite, (m - 1) // 2)[(m - 1) // 2] if m else None
        if m == 0:
            keep = keep & False
        else:
            T = np.float32(np.float32(np.float32(ratio) * np.float32(ratio)) * np.float32(med))      # two float32 products
            keep = keep & (s <= float(T))                                                              # (a float32 value: exact as a Python float)
    return keep


def remove_outliers(cloud, radius, min_neighbors=None, k=None, ratio=2.0, return_mask=False, matcher=None, device=0):
    """`cloud` without its stray points: the rows that are candidates (finite x y z) and pass every rule given, whole records (normals,
    colours), in the cloud's own order; an array or tensor like `cloud`.  One cloud_neighbors call at `radius`.
      radius rule (min_neighbors=N): at least N other points lie within radius of the point.
      k-th-neighbour rule (k=K, ratio=Q): s = the squared distance to the point's K-th nearest neighbour within radius (+inf if it has
        fewer); med = the lower median of the finite s (element (m - 1) // 2 of the m finite values in ascending order); the point is kept
        iff s <= fl(fl(Q * Q) * med), two float32 products: its K-th neighbour lies within Q times the cloud's median K-th-neighbour
        distance.  Without a finite s nothing passes.
    At least one of min_neighbors and k must be given.  The k-th-neighbour rule is the scale-free form of statistical outlier removal: an
    order statistic and two products, the same bits wherever it is computed.  It is NOT PCL's StatisticalOutlierRemoval, whose threshold is
    the mean plus a multiple of the standard deviation of the mean neighbour distances: float sums that depend on their order.
    return_mask=True returns (rows, the boolean keep mask over the cloud's rows)."""
    radius, min_neighbors, k, ratio = _outlier_settings(radius, min_neighbors, k, ratio)
    c, dev = _cloud(cloud, "cloud")
    keep = _outlier_mask(c, dev, radius, min_neighbors, k, ratio, matcher, device)
    rows = c[keep].clone() if dev else c[keep].copy()
    return (rows, keep) if return_mask else rows


def _clean_cloud(cloud, clean, matcher):
    """-> (a copy of `cloud` with x y z of every record remove_outliers(**clean) removes replaced by NaN, the number of candidate records so
    removed, the settings as a dict)"""
    radius, min_neighbors, k, ratio = _outlier_settings(clean.get("radius"), clean.get("min_neighbors"), clean.get("k"), clean.get("ratio", 2.0))
    c, dev = _cloud(cloud, "cloud")
    keep = _outlier_mask(c, dev, radius, min_neighbors, k, ratio, matcher, 0)
    out = c.clone() if dev else c.copy()
    out[~keep, :3] = float("nan")
    if dev:
        import torch
        n_removed = int((torch.isfinite(c[:, :3]).all(dim=1) & ~keep).sum().item())
    else:
        n_removed = int(np.count_nonzero(np.isfinite(c[:, :3]).all(axis=1) & ~keep))
    return out, n_removed, {"radius": radius, "min_neighbors": min_neighbors, "k": k, "ratio": ratio}


def _crop_cloud(cloud, crop):
    """-> (a copy of `cloud` with x y z of every record outside the closed box replaced by NaN, the number of candidate records so removed)"""
    c, dev = _cloud(cloud, "cloud")
    lo, hi = np.asarray(crop[:3], np.float32), np.asarray(crop[3:], np.float32)
    if dev:
        import torch
        xyz = c[:, :3]
        cand = torch.isfinite(xyz).all(dim=1)
        inside = ((xyz >= torch.from_numpy(lo).to(c.device)) & (xyz <= torch.from_numpy(hi).to(c.device))).all(dim=1)
        out = c.clone()
        out[:, :3] = torch.where((cand & inside)[:, None], xyz, torch.full_like(xyz, float("nan")))
        return out, int((cand & ~inside).sum().item())
    xyz = c[:, :3]
    cand = np.isfinite(xyz).all(axis=1) if len(c) else np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        inside = ((xyz >= lo) & (xyz <= hi)).all(axis=1) if len(c) else np.zeros(0, bool)
    out = c.copy()
    out[~(cand & inside), :3] = np.nan
    return out, int(np.count_nonzero(cand & ~inside))


def _voxel_share(within, count):
    """per tolerance (sum over the voxels, in ascending order, of within / count) / n_voxels: each term one float64 division, the terms added one
    after another in float64 (np.cumsum adds sequentially; np.sum adds pairwise), 0 without voxels"""
    within = (within.cpu().numpy() if _is_torch(within) else within).astype(np.float64)
    count = (count.cpu().numpy() if _is_torch(count) else count).astype(np.float64)
    if len(count) == 0:
        return np.zeros(within.shape[1], np.float64)
    return np.cumsum(within / count[:, None], axis=0)[-1] / np.float64(len(count))


def _f1(a, c):
    """the harmonic mean of two arrays of shares, in float64; 0 where both are 0"""
    s = a + c
    return np.where(s > 0, 2.0 * a * c / np.where(s > 0, s, 1.0), 0.0)


def evaluate_cloud(recon, gt, tolerances, matcher=None, device=0, voxel=None, crop=None, clean=None, normals=None):
    """Accuracy and completeness of the cloud `recon` against the cloud `gt` at each of `tolerances`: the point-wise precision / recall /
    F-score.  Two cloud_distance calls with max_dist = max(tolerances):
      accuracy[k]     = the share of recon's candidate points (finite coordinates) with a gt point within tolerances[k];
      completeness[k] = the share of gt's candidate points with a recon point within tolerances[k];
      f1[k]           = their harmonic mean (0 where both are 0).
    voxel=V adds the voxel-averaged figures, so that dense areas do not dominate: a grid of edge V over each cloud (cloud_voxels), and
      accuracy_voxel[k]     = the mean over recon's occupied voxels of the share of the voxel's points with a gt point within tolerances[k];
      completeness_voxel[k] = the same over gt's voxels;  f1_voxel[k] = their harmonic mean.
    (Each share is one float64 division of two integer counts; the shares are added in ascending voxel order, one after another.)
    crop=(x0, y0, z0, x1, y1, z1) first makes every record of either cloud outside the closed box a non-candidate (on a copy: its
    coordinates become NaN), before anything else is computed.
    clean=dict(radius=, min_neighbors=, k=, ratio=) first removes recon's stray points by remove_outliers' rules (on a copy: the removed
    records' coordinates become NaN), before crop and before any scoring; gt is left as it is.
    normals=dict(radius=, k=16, min_neighbors=5, tolerances_deg=(10, 30), signed=False) also scores recon's normals (columns 3 .. 5 of its
    records) against normals estimated from gt's points (cloud_normals with the canonical sign, after crop): one normal_compare of every
    recon point with the gt point nearest to it within max(tolerances).  The plain PCA normal over the k nearest neighbours within radius:
    no orientation is propagated and nothing is meshed; with signed=False (the default) lines are compared, not directions.
    This is NOT the evaluation program of a benchmark.  With voxel and crop it averages over voxels and crops to a box in the manner of
    the benchmarks, but ETH3D's program defines its voxels and its observed volume from the scanner's positions, DTU's applies observation
    masks, and both align the clouds first: nothing is registered here, there are no occlusion or observation masks, and the clouds are
    compared where they lie.  Without voxel and crop nothing is down-sampled or cropped either: every point counts once.
    Returns {"tolerances", "accuracy", "completeness", "f1"} as float64 numpy arrays (ratios formed on the host from the integer
    counts; 0 where a denominator is 0), {"n_accurate", "n_complete"} as int64 arrays, and the integers "n_recon_valid", "n_gt_valid",
    "pairs_accuracy", "pairs_completeness"; with voxel also "accuracy_voxel", "completeness_voxel", "f1_voxel" (float64 arrays),
    "n_recon_voxels" and "n_gt_voxels"; with crop also "n_recon_cropped" and "n_gt_cropped" (the candidate records outside the box); with clean also "clean" (the settings)
    and "n_recon_cleaned" (the candidate records of recon removed); with normals also "normals" (the settings), "normal_tolerances_deg",
    "n_gt_normals", "n_normal_compared", "n_normal_within" (int64 array) and "normal_accuracy" (float64 array: within / compared)."""
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    if tol.size == 0:
        raise ValueError("evaluate_cloud needs at least one tolerance")
    r = float(tol.max())
    if clean is not None:
        with _matcher_for(matcher, device, recon) as m:        # one context for the cleaning and the scoring
            recon, n_cleaned, settings = _clean_cloud(recon, dict(clean), m)
            res = evaluate_cloud(recon, gt, tol, matcher=m, voxel=voxel, crop=crop, normals=normals)
        res.update({"clean": settings, "n_recon_cleaned": n_cleaned})
        return res
    cropped = None
    if crop is not None:
        crop = tuple(float(v) for v in crop)
        if len(crop) != 6 or not all(np.isfinite(crop)) or any(crop[a] > crop[3 + a] for a in range(3)):
            raise ValueError("crop must be six finite numbers (x0, y0, z0, x1, y1, z1) with x0 <= x1, y0 <= y1, z0 <= z1")
        (recon, n_rc), (gt, n_gc) = _crop_cloud(recon, crop), _crop_cloud(gt, crop)
        cropped = {"n_recon_cropped": n_rc, "n_gt_cropped": n_gc}
    vox = nrm = None
    if normals is not None:
        normals = dict(normals)
        settings = {"k": int(normals.pop("k", 16)), "radius": float(normals.pop("radius")), "min_neighbors": int(normals.pop("min_neighbors", 5)),
                    "signed": bool(normals.pop("signed", False))}
        deg = np.ascontiguousarray(normals.pop("tolerances_deg", (10.0, 30.0)), np.float64).reshape(-1)
        if normals:
            raise ValueError("normals: unknown settings %s" % sorted(normals))
        if recon.shape[1] < 6:
            raise ValueError("normals needs recon's normals in columns 3..5 of its records")
    with _matcher_for(matcher, device, recon) as m:            # one context for every call
        want = () if voxel is None else ("dist2",)
        a = cloud_distance(recon, gt, r, tol, want=want if normals is None else ("dist2", "index"), matcher=m)
        c = cloud_distance(gt, recon, r, tol, want=want, matcher=m)
        if normals is not None:
            g = cloud_normals(gt, settings["radius"], settings["k"], settings["min_neighbors"], want=("normal",), matcher=m)
            rn = recon[:, 3:6].contiguous() if _is_torch(recon) else np.ascontiguousarray(recon[:, 3:6], np.float32)
            s = normal_compare(rn, g["normal"], a["index"], deg, dist2=a["dist2"], max_dist=r, signed=settings["signed"], matcher=m)
            nrm = {"normals": settings, "normal_tolerances_deg": deg, "n_gt_normals": g["n_normals"], "n_normal_compared": s["n_compared"],
                   "n_normal_within": s["within"], "normal_accuracy": s["accuracy"]}
        if voxel is not None:
            va = cloud_voxels(recon, voxel, a["dist2"], tol, want=("count",), matcher=m)
            vc = cloud_voxels(gt, voxel, c["dist2"], tol, want=("count",), matcher=m)
            acc_v, com_v = _voxel_share(va["within"], va["count"]), _voxel_share(vc["within"], vc["count"])
            vox = {"accuracy_voxel": acc_v, "completeness_voxel": com_v, "f1_voxel": _f1(acc_v, com_v),
                   "n_recon_voxels": va["n_voxels"], "n_gt_voxels": vc["n_voxels"]}
    na, nc = a["within"].astype(np.int64), c["within"].astype(np.int64)
    acc = na / np.float64(a["n_valid_query"]) if a["n_valid_query"] else np.zeros(tol.size, np.float64)
    com = nc / np.float64(c["n_valid_query"]) if c["n_valid_query"] else np.zeros(tol.size, np.float64)
    res = {"tolerances": tol.copy(), "accuracy": acc, "completeness": com, "f1": _f1(acc, com), "n_accurate": na, "n_complete": nc,
           "n_recon_valid": a["n_valid_query"], "n_gt_valid": c["n_valid_query"], "pairs_accuracy": a["pairs"], "pairs_completeness": c["pairs"]}
    if vox is not None:
        res.update(vox)
    if cropped is not None:
        res.update(cropped)
    if nrm is not None:
        res.update(nrm)
    return res


def cloud_render(cloud, K, R, t, w, h, radius=0.0, max_px=8, occlusion_diff=0.02, depth_diff=0.01, min_points=1, want=("depth", "count"), max_splats=None,
                 matcher=None, device=0, normals=None):
    """`cloud` rendered into the view (K, R, t) of w x h pixels as a depth map, occlusion by the cloud's own points handled
    (tsar_cloud_render_ctx; include/tsar.h states the arithmetic).  cloud: [n, k >= 3] float32, x y z first, a numpy array or a torch device
    tensor (a fused cloud as api.fuse returns it goes in as it is).  radius (world units): the half-width of a point's occluder footprint, at
    most max_px pixels; a pixel whose front-most landing lies more than occlusion_diff (relative) behind the nearest footprint over it is
    hidden; 0 = a plain one-pixel z-buffer.  A pixel's depth comes only from points that land on it.  max_splats: the call is refused
    (TsarError, TSAR_ERR_INVALID, with .n_splats) when the scatter would issue more atomics; None = the library's default.  matcher / device:
    as cloud_distance.
    Returns a dict: "depth" ([h, w] float32, 0 where nothing is kept), "count" ([h, w] uint8: the landings within depth_diff of the front-most,
    saturated at 255), "index" ([h, w] int32: the front-most point, -1 where nothing is kept), as `want` names them (numpy arrays, or torch
    tensors on the cloud's device), and the integer "n_splats".
    normals: None = the square occluder above.  "record" (the records' floats 3..5, k >= 6) or an [n, 3] float32 array or device tensor,
    living where the cloud does: the normal-oriented occluder (tsar_cloud_render_oriented_ctx): a point occludes as its tangent disc of radius
    `radius`, cut to the square; a point with a zero or non-finite normal keeps the square.  `want` may then name "occluder" ([h, w] float32:
    the occluder buffer, 0 where nothing covers), and the result has "n_covered", the covering (point, pixel) pairs."""
    L = load_library()
    c, dev = _cloud(cloud, "cloud")
    n, w, h = int(c.shape[0]), int(w), int(h)
    assert w >= 1 and h >= 1 and len(want) > 0, "cloud_render needs a size of at least 1 x 1 and at least one output"
    assert normals is not None or "occluder" not in want, "the occluder plane comes with normals"
    p = CloudRenderParams()
    L.tsar_default_cloud_render_params(C.byref(p))
    p.radius, p.max_px, p.occlusion_diff, p.depth_diff, p.min_points = float(radius), int(max_px), float(occlusion_diff), float(depth_diff), int(min_points)
    if max_splats is not None:
        p.max_splats = int(max_splats)
    cam = _cameras(np.asarray(K, np.float32).reshape(1, 3, 3), np.asarray(R, np.float32).reshape(1, 3, 3), np.asarray(t, np.float32).reshape(1, 3), 1)
    spec = {"depth": ((h, w), np.float32), "count": ((h, w), np.uint8), "index": ((h, w), np.int32)}
    if normals is not None:
        spec["occluder"] = ((h, w), np.float32)
    res = _outputs(spec, want, c.device if dev else None)
    n_splats, n_covered = C.c_int64(-1), C.c_int64(-1)
    planes = [_ptr(res.get(key))[0] for key in spec]
    nrm = None
    if normals is not None and not isinstance(normals, str):
        nrm, nrm_dev = _cloud(normals, "normals")
        assert int(nrm.shape[0]) == n and nrm_dev == dev and (not dev or nrm.device == c.device), "normals must be [n, k >= 3] and live where the cloud does"
    else:
        assert normals in (None, "record"), "normals must be None, \"record\" or an [n, 3] array"
    no_points = (C.c_float * 3)()                     # (n == 0: a normals pointer that is not NULL, which would mean "record"; nothing reads it)
    with _matcher_for(matcher, device, c) as m:
        if normals is None:
            rc = L.tsar_cloud_render_ctx(m._ctx, _ptr(c)[0] if n else None, n, int(c.shape[1]), cam, w, h, C.byref(p), *planes, C.byref(n_splats),
                                         MEM_DEVICE if dev else MEM_HOST)
        else:
            rc = L.tsar_cloud_render_oriented_ctx(m._ctx, _ptr(c)[0] if n else None, n, int(c.shape[1]), None if nrm is None else _ptr(nrm)[0] if n else C.cast(no_points, C.c_void_p),
                                                  int(nrm.shape[1]) if nrm is not None else 0, cam, w, h, C.byref(p), *planes, C.byref(n_splats), C.byref(n_covered),
                                                  MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            err = TsarError(rc, L.tsar_last_error(m._ctx).decode())
            err.n_splats = int(n_splats.value) if n_splats.value >= 0 else None     # filled when max_splats refused the call
            raise err
    res["n_splats"] = int(n_splats.value)
    if normals is not None:
        res["n_covered"] = int(n_covered.value)
    return res


def _depth_ratios(rec):
    """the float64 ratios of a record of depth_compare's counts, formed on the host (0 where a denominator is 0)"""
    w = np.asarray(rec["within"], np.int64).astype(np.float64)
    nb, ng = np.float64(rec["n_both"]), np.float64(rec["n_gt"])
    rec["accuracy"] = w / nb if rec["n_both"] else np.zeros(len(w), np.float64)
    rec["completeness"] = w / ng if rec["n_gt"] else np.zeros(len(w), np.float64)
    rec["cover"] = float(nb / ng) if rec["n_gt"] else 0.0
    return rec


def depth_compare(depth, gt, tolerances, mask=None, want_error=False, matcher=None, device=0):
    """The depth map `depth` scored against the ground-truth map `gt` with the per-pixel bars (tsar_depth_compare_ctx; include/tsar.h).  depth and
    gt: float32 arrays of one shape, both numpy arrays or both torch device tensors; mask (uint8 / bool, same shape and memory; None = every
    pixel) names the pixels that count; tolerances: 1 to 16 relative tolerances.  A ground-truth pixel has gt in (0, inf) and a set mask.
    Returns a dict: "n_gt"; "n_both" (ground-truth pixels with a depth in (0, inf)); "within" (int64 array: per tolerance the n_both pixels with
    |D - G| <= fl(tol * G)); "n_front" / "n_behind" (further than tolerances[0] in front of / behind the ground truth); the float64 ratios
    "accuracy" = within / n_both, "completeness" = within / n_gt and "cover" = n_both / n_gt; "tolerances"; and with want_error "error"
    ((D - G) / G on the n_both pixels, NaN elsewhere; like depth)."""
    L = load_library()
    d = _coerce(depth, np.float32, None, "depth", tensors="device")
    g = _coerce(gt, np.float32, tuple(d.shape), "gt", tensors="device")
    dev = _is_torch(d)
    assert dev == _is_torch(g), "depth and gt must live in the same memory space"
    if mask is not None and not _is_torch(mask):
        mask = np.asarray(mask).astype(np.uint8)
    elif mask is not None:
        import torch
        mask = mask.to(torch.uint8).contiguous()
    mk = _coerce(mask, np.uint8, tuple(d.shape), "mask", tensors="device")
    assert mk is None or _is_torch(mk) == dev, "mask must live where depth does"
    assert not dev or (d.is_contiguous() and g.is_contiguous() and d.device == g.device and (mk is None or mk.device == d.device)), "tensors must be contiguous and on one device"
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    n = int(np.prod(d.shape))
    within = np.zeros(len(tol), np.int64)
    out = _outputs({"error": (tuple(d.shape), np.float32)}, ("error",) if want_error else (), d.device if dev else None)
    cnt = [C.c_int64(0) for _ in range(4)]
    with _matcher_for(matcher, device, d) as m:
        rc = L.tsar_depth_compare_ctx(m._ctx, _ptr(d)[0] if n else None, _ptr(g)[0] if n else None, _ptr(mk)[0] if n else None, n, len(tol), tol.ctypes.data_as(C.c_void_p),
                                      C.byref(cnt[0]), C.byref(cnt[1]), within.ctypes.data_as(C.c_void_p), C.byref(cnt[2]), C.byref(cnt[3]), _ptr(out.get("error"))[0],
                                      MEM_DEVICE if dev else MEM_HOST)
        if rc != TSAR_OK:
            raise TsarError(rc, L.tsar_last_error(m._ctx).decode())
    res = {"tolerances": tol.copy(), "n_gt": int(cnt[0].value), "n_both": int(cnt[1].value), "within": within, "n_front": int(cnt[2].value), "n_behind": int(cnt[3].value)}
    res.update(out)
    return _depth_ratios(res)


def evaluate_depth_maps(depths, cloud, K, R, t, tolerances, radius, masks=None, matcher=None, device=0, normals=None, **render_kw):
    """Depth maps scored per pixel against the cloud `cloud` (a scan, a fused cloud as api.fuse returns it) rendered into their own cameras: per
    view v one cloud_render of the cloud into (K[v], R[v], t[v]) at depths[v]'s size with the footprint `radius` (render_kw: max_px,
    occlusion_diff, depth_diff, min_points, max_splats) and one depth_compare of depths[v] against it (masks[v] if given).  The project's own
    per-pixel bars against a rendered cloud: not the evaluation program of a benchmark (no observation masks, no alignment).  normals:
    cloud_render's (None, "record" or an [n, 3] array): the renders use the normal-oriented occluder.
    Returns (views, total): per view depth_compare's dict plus "n_splats" (and "n_covered" with normals); total adds the counts over the views
    first and forms the ratios afterwards."""
    views = []
    c, dev = _cloud(cloud, "cloud")
    with _matcher_for(matcher, device, c) as m:
        for v, d in enumerate(depths):
            h, w = int(d.shape[0]), int(d.shape[1])
            r = cloud_render(c, K[v], R[v], t[v], w, h, radius, want=("depth",), matcher=m, normals=normals, **render_kw)
            if dev != _is_torch(d):                  # the map goes where the cloud's render lies
                if dev:
                    import torch
                    d = torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(c.device)
                else:
                    d = d.cpu().numpy()
            rec = depth_compare(d, r["depth"], tolerances, None if masks is None else masks[v], matcher=m)
            rec["n_splats"] = r["n_splats"]
            if normals is not None:
                rec["n_covered"] = r["n_covered"]
            views.append(rec)
    total = {"tolerances": np.ascontiguousarray(tolerances, np.float32).reshape(-1)}
    for k in ("n_gt", "n_both", "n_front", "n_behind", "n_splats") + (("n_covered",) if normals is not None else ()):
        total[k] = int(sum(rec[k] for rec in views))
    total["within"] = np.sum([rec["within"] for rec in views], axis=0, dtype=np.int64) if views else np.zeros(len(total["tolerances"]), np.int64)
    return views, _depth_ratios(total)


def pinned_empty(shape, dtype=np.float32):
    """numpy array over page-locked host memory from tsar_host_alloc; the memory is released when the last array
    (or view of it) referring to it is collected"""
    import weakref
    L = load_library()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = L.tsar_host_alloc(n)
    if not p:
        raise MemoryError(f"tsar_host_alloc({n}) failed")
    buf = (C.c_char * n).from_address(p)
    weakref.finalize(buf, L.tsar_host_free, p)      # every numpy view keeps `buf` alive through its base chain
    return np.frombuffer(buf, dtype=dt).reshape(shape)

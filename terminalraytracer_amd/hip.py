"""ctypes binding of libtrt_hip.so (C-ABI of include/trt_hip.h).

This is the only compute path of the package: there is no CPU or PyTorch fallback.  If the
HIP library is missing the import of `lib()` raises; if no GPU is present every compute call
fails with TRT_ERR_HIP.  PyTorch is used by callers only for device memory / streams /
torch.distributed; raw device pointers and the stream handle cross this boundary as integers.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
# TRT_HIP_LIB selects another build of the same library (kernel-tuning A/B runs); default is the in-tree one
LIB_PATH = os.environ.get("TRT_HIP_LIB") or os.path.join(_HERE, "libtrt_hip.so")

TRT_OK = 0
ERRORS = {-1: "TRT_ERR_HIP", -2: "TRT_ERR_ARGUMENT", -3: "TRT_ERR_NO_SCENE", -4: "TRT_ERR_CAPACITY",
          -5: "TRT_ERR_NOT_INITIALISED"}


class TrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{ERRORS.get(code, code)}: {message}")
        self.code = code


class RowSet(C.Structure):
    """trt_rowset: interleaved row tiles owned by one renderer (include/trt_hip.h)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("tile_rows", C.c_int), ("tile_first", C.c_int),
                ("tile_step", C.c_int)]

    @staticmethod
    def whole(width, height):
        return RowSet(width, height, height, 0, 1)

    @staticmethod
    def shard(width, height, rank, world, tile_rows=8):
        return RowSet(width, height, tile_rows, rank, world)


# every symbol include/trt_hip.h declares: (restype, argtypes)
_VP, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SYMBOLS = {
    "project_scene": (None, [C.POINTER(L.Scene), C.POINTER(L.Screen)]),
    "trt_render_frame": (_I, [C.POINTER(L.Scene), C.POINTER(L.Screen), _I, _I]),
    "render_frame": (_I, [C.POINTER(L.Scene), C.POINTER(L.Screen), _I, _I]),
    "trt_render_frame_rgb8": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_render_frame_ansi": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_render_frame_ansi_half": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_render_frame_ansi_delta": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_init": (_I, [_I]),
    "trt_shutdown": (_I, []),
    "trt_upload_skybox": (_I, [C.POINTER(L.Skybox)]),
    "trt_invalidate_skybox": (_I, []),
    "trt_rowset_rows": (_I, [C.POINTER(RowSet)]),
    "trt_rowset_frame_row": (_I, [C.POINTER(RowSet), _I]),
    "trt_create": (_I, [_I, C.POINTER(_VP)]),
    "trt_destroy": (_I, [_VP]),
    "trt_set_stream": (_I, [_VP, _VP]),
    "trt_set_scene": (_I, [_VP, C.POINTER(L.Scene)]),
    "trt_render_device": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_device_rgb8": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_quantize_device": (_I, [_VP, _VP, _SZ, _VP]),
    "trt_ansi_bytes": (_SZ, [_I, _I]),
    "trt_render_device_ansi": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_ansi_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP]),
    "trt_ansi_half_bytes": (_SZ, [_I, _I]),
    "trt_render_device_ansi_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_ansi_half_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP]),
    "trt_render_host_ansi_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch_ansi_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch_ansi_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_kitty_bytes": (_SZ, [_I, _I]),
    "trt_render_device_kitty": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_kitty_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP]),
    "trt_render_host_kitty": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch_kitty": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch_kitty": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_frame_kitty": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_ansi256_bytes": (_SZ, [_I, _I]),
    "trt_ansi256_half_bytes": (_SZ, [_I, _I]),
    "trt_render_device_ansi256": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_device_ansi256_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_ansi256_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP]),
    "trt_ansi256_half_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP]),
    "trt_xterm256_from_rgb8_device": (_I, [_VP, _VP, _SZ, _VP]),
    "trt_render_host_ansi256": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_host_ansi256_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch_ansi256": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_device_batch_ansi256_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch_ansi256": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_host_batch_ansi256_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_frame_ansi256": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_render_frame_ansi256_half": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP]),
    "trt_render_frame_ansi_delta_half": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_ansi_delta_half_capacity": (_SZ, [_I, _I]),
    "trt_ansi_delta_half_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi_delta_half_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_render_device_ansi_delta_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_ansi_delta_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_sixel_capacity": (_SZ, [_I, _I]),
    "trt_sixel_from_rgb8_device": (_I, [_VP, _VP, _I, _I, _VP, _SZ, _VP]),
    "trt_render_device_sixel": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_sixel": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_frame_sixel": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_ansi_delta_capacity": (_SZ, [_I, _I]),
    "trt_ansi_delta_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi_delta_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_render_device_ansi_delta": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_ansi_delta": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_ansi_delta_reset": (_I, [_VP]),
    "trt_render_host": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_host_rgb8": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_host_ansi": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch_rgb8": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch_rgb8": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_render_device_batch_ansi": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ]),
    "trt_render_host_batch_ansi": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP]),
    "trt_batch_info": (_I, [_VP, C.POINTER(_I), C.POINTER(_I)]),
    "trt_ansi_delta_chain_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi_delta_half_chain_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi_delta_chain_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_ansi_delta_half_chain_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_render_device_batch_ansi_delta": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_device_batch_ansi_delta_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_batch_ansi_delta": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_host_batch_ansi_delta_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_ansi256_delta_capacity": (_SZ, [_I, _I]),
    "trt_ansi256_delta_half_capacity": (_SZ, [_I, _I]),
    "trt_ansi256_delta_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi256_delta_half_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi256_delta_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_ansi256_delta_half_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_render_device_ansi256_delta": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_device_ansi256_delta_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_ansi256_delta": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_host_ansi256_delta_half": (_I, [_VP, C.POINTER(L.Camera), C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_frame_ansi256_delta": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_frame_ansi256_delta_half": (_I, [C.POINTER(L.Scene), _I, _I, _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_ansi256_delta_chain_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi256_delta_half_chain_from_rgb8_device": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP]),
    "trt_ansi256_delta_chain_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_ansi256_delta_half_chain_kernel_times": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP, C.POINTER(C.c_float)]),
    "trt_render_device_batch_ansi256_delta": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_device_batch_ansi256_delta_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, _VP]),
    "trt_render_host_batch_ansi256_delta": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_render_host_batch_ansi256_delta_half": (_I, [_VP, _VP, _I, C.POINTER(RowSet), _I, _I, _VP, _SZ, C.POINTER(_SZ)]),
    "trt_synchronize": (_I, [_VP]),
    "trt_kernel_times": (_I, [_VP, C.POINTER(C.c_float), _I]),
    "trt_render_kernel_times": (_I, [_VP, C.POINTER(C.c_float), C.POINTER(C.c_float), _I]),
    "trt_enable_counters": (_I, [_VP, _I]),
    "trt_read_counters": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "trt_read_diagnostics": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "trt_set_kernel": (_I, [_VP, _I]),
    "trt_set_light_grids": (_I, [_VP, _I, _I]),
    "trt_set_light_slabs": (_I, [_VP, _I, _I]),
    "trt_share_scene": (_I, [_VP, _VP]),
    "trt_set_scene_policy": (_I, [_I, _I]),
    "trt_scene_is_moving": (_I, []),
    "trt_scene_info": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_I), C.POINTER(C.c_double)]),
    "trt_set_list_pool_words": (_I, [_VP, C.c_size_t]),
    "trt_set_path_grids": (_I, [_VP, _I, _I]),
    "trt_set_path_grids_min_spheres": (_I, [_VP, _I]),
    "trt_set_path_patches": (_I, [_VP, _I]),
    "trt_get_path_patches": (_I, [_VP, C.POINTER(_I), C.POINTER(_I)]),
    "trt_path_family_code": (_I, [_VP, _I, _I, _VP]),
    "trt_set_compaction": (_I, [_VP, _I]),
    "trt_render_variant": (_I, [_VP, C.POINTER(_I), C.POINTER(_I)]),
    "trt_set_scene_image": (_I, [_VP, _I]),
    "trt_render_image": (_I, [_VP, C.POINTER(_I), C.POINTER(C.c_ulonglong)]),
    "trt_set_scratch_fill": (_I, [_VP, _I]),
    "trt_default_context": (_VP, []),
    "trt_build_counts": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "trt_set_path_lean_lists": (_I, [_VP, _I]),
    "trt_get_path_lean_lists": (_I, [_VP, C.POINTER(_I), C.POINTER(C.c_ulonglong)]),
    "trt_read_path_lean_tables": (C.c_long, [_VP, _VP, C.c_size_t]),
    "trt_read_path_tables": (C.c_long, [_VP, C.POINTER(L.Camera), _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(C.c_long)]),
    "trt_read_sweep_fallbacks": (_I, [_VP, C.POINTER(C.c_ulonglong)]),
    "trt_read_shading_passes": (_I, [_VP, C.POINTER(C.c_ulonglong)]),
    "trt_read_loop_diagnostics": (_I, [_VP, C.POINTER(C.c_ulonglong)]),
    "trt_set_refraction": (_I, [_VP, _VP, _I]),
    "trt_set_specular": (_I, [_VP, _I]),
    "trt_get_specular": (_I, [_VP, C.POINTER(_I)]),
    "trt_set_default_specular": (_I, [_I]),
    "trt_set_sky_filter": (_I, [_VP, _I]),
    "trt_get_sky_filter": (_I, [_VP, C.POINTER(_I)]),
    "trt_set_default_sky_filter": (_I, [_I]),
    "trt_reserve_cus": (_I, [_VP, _I]),
    "trt_get_stream": (_I, [_VP, C.POINTER(C.c_void_p)]),
    "trt_selftest_cube": (_I, [_VP, _VP, C.c_size_t, _VP, _VP]),
    "trt_selftest_unit": (_I, [_VP, _VP, C.c_size_t, _VP, _VP]),
    "trt_selftest_sky": (_I, [_VP, _VP, C.c_size_t, _I, _VP, _VP, _VP]),
    "trt_read_light_grid": (C.c_long, [_VP, _I, _I, _VP, C.c_size_t]),
    "trt_read_light_lists": (C.c_long, [_VP, _I, _I, _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(C.c_long)]),
    "trt_kernel_info": (_I, [_VP] + [C.POINTER(_I)] * 5),
    "trt_selftest_div_sqrt": (_I, [_VP, _VP, _VP, _SZ, _VP, _VP]),
    "trt_probe_rays": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "trt_probe_rays_production": (_I, [_VP, C.POINTER(L.Camera), _VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "trt_probe_path_lookups": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "trt_probe_shadow_lookups": (_I, [_VP, _VP, _SZ, _I, _VP, _VP, _VP, _VP, _VP]),
    "trt_selftest_filter": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP]),
    "trt_launch_count": (C.c_long, [_VP]),
    "trt_launch_span_ms": (_I, [_VP, C.c_long, _VP, C.c_long, C.POINTER(C.c_float)]),
    "trt_dist_unique_id": (_I, [_VP]),
    "trt_dist_frame_times": (_I, [_VP, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "trt_dist_allow_rccl_override": (_I, [_I]),
    "trt_dist_rccl_library": (C.c_char_p, []),
    "trt_dist_comm_ranks": (_I, [_VP]),
    "trt_dist_create": (_I, [_I, C.POINTER(L.Scene), _VP, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_VP)]),
    "trt_dist_set_scene": (_I, [_VP, C.POINTER(L.Scene)]),
    "trt_dist_render": (_I, [_VP, C.POINTER(L.Camera), _I, _I, C.POINTER(_VP)]),
    "trt_dist_synchronize": (_I, [_VP]),
    "trt_dist_enable_rgb8": (_I, [_VP]),
    "trt_dist_render_rgb8": (_I, [_VP, C.POINTER(L.Camera), _I, _I, C.POINTER(_VP)]),
    "trt_dist_fetch_rgb8": (_I, [_VP, _VP, _VP]),
    "trt_dist_fetch": (_I, [_VP, _VP, _VP]),
    "trt_dist_source_rows": (_I, [_I, _I, _I, _I, C.POINTER(_I)]),
    "trt_dist_info": (_I, [_VP] + [C.POINTER(_I)] * 5),
    "trt_dist_context": (_VP, [_VP, _I]),
    "trt_dist_destroy": (_I, [_VP]),
    "trt_dist_last_error": (C.c_char_p, []),
    "trt_last_error": (C.c_char_p, []),
    "trt_version": (C.c_char_p, []),
}


@functools.lru_cache(maxsize=None)
def lib():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make lib` (hipcc --offload-arch=gfx950). "
                          "There is no fallback path.")
    # Load order matters when PyTorch shares the process: torch bundles its own libamdhip64/libhsa-runtime64,
    # and a process must initialise only ONE HIP runtime.  Importing torch first (when it is installed) makes
    # libtrt_hip.so's libamdhip64.so dependency resolve to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    dll = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(dll, name)  # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    return dll


def _check(code):
    if code != TRT_OK:
        raise TrtError(code, lib().trt_last_error().decode())


def camera_struct(camera_array):
    cam = L.Camera()
    a = np.ascontiguousarray(camera_array, dtype=np.float64).reshape(15)
    C.memmove(C.byref(cam), a.ctypes.data, 120)
    return cam


class Context:
    """One renderer on one GPU (trt_context)."""

    PRODUCTION, REFERENCE_ORDER = 0, 1

    def __init__(self, device=0, _borrowed=None):
        self._owned = _borrowed is None
        if self._owned:
            self._h = _VP()
            _check(lib().trt_create(device, C.byref(self._h)))
        else:
            self._h = _VP(_borrowed)  # a context owned by someone else (trt_dist_context)
        self.device = device

    def close(self):
        if self._h and self._owned:
            lib().trt_destroy(self._h)
        self._h = _VP()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        _check(lib().trt_set_stream(self._h, _VP(stream_handle or 0)))

    def set_scene(self, scene_data):
        scene = scene_data.as_scene()
        _check(lib().trt_set_scene(self._h, C.byref(scene)))

    def set_kernel(self, which):
        _check(lib().trt_set_kernel(self._h, which))

    def reserve_cus(self, reserved):
        """keep `reserved` compute units free of this context's kernels (trt_reserve_cus)"""
        _check(lib().trt_reserve_cus(self._h, reserved))

    def stream_ptr(self):
        """the HIP stream the context launches on, as an integer (trt_get_stream)"""
        p = C.c_void_p()
        _check(lib().trt_get_stream(self._h, C.byref(p)))
        return p.value or 0

    def set_light_grids(self, directional_cells, point_cells):
        """cells per side of the light-space candidate tables; 0, 0 = off (trt_set_light_grids)"""
        _check(lib().trt_set_light_grids(self._h, directional_cells, point_cells))

    def share_scene(self, source):
        """render `source`'s scene from its tables: one copy of every read-only table per device (trt_share_scene)"""
        _check(lib().trt_share_scene(self._h, source._h))

    def scene_info(self):
        b, n, t = C.c_ulonglong(), _I(), C.c_double()
        _check(lib().trt_scene_info(self._h, C.byref(b), C.byref(n), C.byref(t)))
        return {"table_bytes": b.value, "sharers": n.value, "build_seconds": t.value}

    def set_list_pool_words(self, words):
        """tests: cap the pool of long candidate lists (trt_set_list_pool_words)"""
        _check(lib().trt_set_list_pool_words(self._h, words))

    def set_light_slabs(self, directional_slabs, point_shells):
        """the light tables' depth coordinate: slabs along a directional light, shells about a point light (trt_set_light_slabs)"""
        _check(lib().trt_set_light_slabs(self._h, directional_slabs, point_shells))

    def set_path_grids(self, eye_cells, sphere_cells):
        """cells per cube-map face side of the path rays' family tables; 0, 0 = off (trt_set_path_grids)"""
        _check(lib().trt_set_path_grids(self._h, eye_cells, sphere_cells))

    def set_path_patches(self, m):
        """sub-families of the spheres: 6 m^2 patches per sphere; 0 = one family per sphere, -1 = by the number of spheres (trt_set_path_patches)"""
        _check(lib().trt_set_path_patches(self._h, m))

    def path_patches(self):
        """(m, patches per sphere) of the current scene's tables (trt_get_path_patches)"""
        m, p = _I(), _I()
        _check(lib().trt_get_path_patches(self._h, C.byref(m), C.byref(p)))
        return m.value, p.value

    def family_codes(self, families, rays, num_spheres):
        """The kernel's family codes (trt_path_family_code) for rays stored along chains: families[j] in the numbering 0 eye,
        1 mirror eye, 2 + s starts on sphere s, 2 + N + s reflected by the ground with a parent that started on sphere s --
        that parent is ray j - 1 of the chain, whose origin names the patch."""
        families = np.asarray(families, dtype=np.int32)
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = families.copy()
        n = num_spheres
        for j in np.nonzero(families >= 2 + n)[0]:
            s = int(families[j]) - 2 - n
            assert j > 0 and families[j - 1] == 2 + s, "a mirror ray's parent must precede it"
            parent = np.ascontiguousarray(rays[j - 1, :3])
            out[j] = lib().trt_path_family_code(self._h, 3, s, parent.ctypes.data)
        return out

    def set_path_grids_min_spheres(self, min_spheres):
        """scenes with fewer spheres keep the sweep for their path rays (trt_set_path_grids_min_spheres)"""
        _check(lib().trt_set_path_grids_min_spheres(self._h, min_spheres))

    def set_compaction(self, mode):
        """shading decoupled from the owning lane: -1 when it costs no occupancy (default), 0 never, 1 whenever it fits (trt_set_compaction)"""
        _check(lib().trt_set_compaction(self._h, mode))

    def render_variant(self):
        """{"decoupled": bool, "workgroup_threads": int} of the kernel the next frame of the current scene runs (trt_render_variant)"""
        d, t = _I(), _I()
        _check(lib().trt_render_variant(self._h, C.byref(d), C.byref(t)))
        return {"decoupled": bool(d.value), "workgroup_threads": t.value}

    def set_scene_image(self, mode):
        """where the kernels read the scene from: -1 device memory when the LDS image does not fit (default), 0 LDS only,
        1 device memory always (trt_set_scene_image)"""
        _check(lib().trt_set_scene_image(self._h, mode))

    def render_image(self):
        """{"in_device_memory": bool, "image_bytes": int} of the kernel render_variant() describes (trt_render_image)"""
        d, b = _I(), C.c_ulonglong()
        _check(lib().trt_render_image(self._h, C.byref(d), C.byref(b)))
        return {"in_device_memory": bool(d.value), "image_bytes": b.value}

    def build_counts(self):
        """(table builds, skybox uploads) this context has performed since it was created (trt_build_counts)"""
        b, u = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().trt_build_counts(self._h, C.byref(b), C.byref(u)))
        return b.value, u.value

    def set_scratch_fill(self, on=True):
        """tests: every launch first fills its own range of the sample scratch and its own output range with NaNs, so that a
        work unit or a pixel it does not write shows (trt_set_scratch_fill)"""
        _check(lib().trt_set_scratch_fill(self._h, 1 if on else 0))

    def read_path_tables(self, camera_array):
        """(info dict, list cells uint64[], pool uint64[]) of the path rays' tables as built for this camera's eye"""
        cam = camera_struct(camera_array)
        info = (C.c_long * 8)()
        probe = np.zeros(1, dtype=np.uint64)
        lib().trt_read_path_tables(self._h, C.byref(cam), probe.ctypes.data, 0, probe.ctypes.data, 0, info)  # sizes only
        cells = np.zeros(max(1, info[4]), dtype=np.uint64)
        pool = np.zeros(max(1, info[7]), dtype=np.uint64)
        got = lib().trt_read_path_tables(self._h, C.byref(cam), cells.ctypes.data, cells.size, pool.ctypes.data, pool.size, info)
        if got < 0:
            _check(int(got))
        keys = ("enabled", "eye_cells", "sphere_cells", "spheres", "cells", "pool_used_scene", "pool_used_eye", "pool_capacity")
        return dict(zip(keys, [int(x) for x in info])), cells[:got], pool

    def set_path_lean_lists(self, mode):
        """lean twins of the spheres' own families: 1 on, 0 off (the full tables, as without twins), -1 the default: on within the tables' budget
        (trt_set_path_lean_lists)"""
        _check(lib().trt_set_path_lean_lists(self._h, mode))

    def path_lean_lists(self):
        """{"in_use": bool, "twin_bytes": int} (trt_get_path_lean_lists)"""
        u, b = _I(), C.c_ulonglong()
        _check(lib().trt_get_path_lean_lists(self._h, C.byref(u), C.byref(b)))
        return {"in_use": bool(u.value), "twin_bytes": b.value}

    def read_path_lean_tables(self):
        """the twins' list cells uint64[] (empty: the scene has none); their long lists are in read_path_tables()'s pool"""
        n = self.path_lean_lists()["twin_bytes"] // 8
        cells = np.zeros(max(1, n), dtype=np.uint64)
        got = lib().trt_read_path_lean_tables(self._h, cells.ctypes.data, cells.size)
        if got < 0:
            _check(int(got))
        return cells[:got]

    def set_refraction(self, ior=None):
        """EXTENSION, parity unpinned: per-sphere indices of refraction (0 = opaque); None turns it off (trt_set_refraction)"""
        if ior is None:
            _check(lib().trt_set_refraction(self._h, None, 0))
        else:
            a = np.ascontiguousarray(ior, dtype=np.float64)
            _check(lib().trt_set_refraction(self._h, a.ctypes.data, a.size))

    def set_specular(self, on=True):
        """EXTENSION, parity unpinned: the lights' Blinn-Phong terms from Material.specularity; 0 / False is the reference's path
        (trt_set_specular)"""
        _check(lib().trt_set_specular(self._h, int(on)))

    def specular(self):
        """whether the specular extension is on (trt_get_specular)"""
        v = _I()
        _check(lib().trt_get_specular(self._h, C.byref(v)))
        return bool(v.value)

    def set_sky_filter(self, mode=1):
        """EXTENSION, parity unpinned: SKY_BILINEAR (1) blends the four sky texels around a look-up; SKY_NEAREST (0) is the reference's
        path (trt_set_sky_filter)"""
        _check(lib().trt_set_sky_filter(self._h, int(mode)))

    def sky_filter(self):
        """the context's sky filter, SKY_NEAREST or SKY_BILINEAR (trt_get_sky_filter)"""
        v = _I()
        _check(lib().trt_get_sky_filter(self._h, C.byref(v)))
        return int(v.value)

    def read_sweep_fallbacks(self):
        v = C.c_ulonglong()
        _check(lib().trt_read_sweep_fallbacks(self._h, C.byref(v)))
        return v.value

    def selftest_unit(self, xyzw):
        """(fast, reference): unit(x,y,z) and sqrt(w) by the kernels' lean code and by the compiler's plain expansions"""
        v = np.ascontiguousarray(xyzw, dtype=np.float64).reshape(-1, 4)
        fast, ref = np.zeros_like(v), np.zeros_like(v)
        _check(lib().trt_selftest_unit(self._h, v.ctypes.data, v.shape[0], fast.ctypes.data, ref.ctypes.data))
        return fast, ref

    def selftest_cube(self, xyz):
        """(device, host): {face, sc, tc, 2 * major} of directions by v_cubeid / sc / tc / ma and by their C restatement"""
        v = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        dev, host = np.zeros((v.shape[0], 4), dtype=np.float32), np.zeros((v.shape[0], 4), dtype=np.float32)
        _check(lib().trt_selftest_cube(self._h, v.ctypes.data, v.shape[0], dev.ctypes.data, host.ctypes.data))
        return dev, host

    def selftest_sky(self, dirs, dim):
        """(exact, estimate, ambiguous): texel index of unit directions by the FP64 form of the skybox look-up, by the FP32 estimate,
        and where the estimate does not vouch for itself (trt_selftest_sky)"""
        v = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        exact, est = np.zeros(v.shape[0], dtype=np.int64), np.zeros(v.shape[0], dtype=np.int64)
        amb = np.zeros(v.shape[0], dtype=np.int32)
        _check(lib().trt_selftest_sky(self._h, v.ctypes.data, v.shape[0], int(dim), exact.ctypes.data, est.ctypes.data, amb.ctypes.data))
        return exact, est, amb

    def read_light_grid(self, point_light, index, words):
        """one light's device-built candidate table as uint64 words (trt_read_light_grid)"""
        out = np.zeros(words, dtype=np.uint64)
        got = lib().trt_read_light_grid(self._h, int(point_light), index, out.ctypes.data, words)
        if got < 0:
            _check(int(got))
        return out[:got]

    def read_light_lists(self, point_light, index):
        """(info dict, list cells uint64[], pool uint64[]) of one light's table in the form the kernels read (trt_read_light_lists)"""
        info = (C.c_long * 4)()
        got = lib().trt_read_light_lists(self._h, int(point_light), index, None, 0, None, 0, info)  # sizes only
        if got < 0:
            _check(int(got))
        cells = np.zeros(max(1, info[0]), dtype=np.uint64)
        pool = np.zeros(max(1, info[2]), dtype=np.uint64)
        got = lib().trt_read_light_lists(self._h, int(point_light), index, cells.ctypes.data, cells.size, pool.ctypes.data, pool.size, info)
        if got < 0:
            _check(int(got))
        return dict(zip(("cells", "list_bits", "pool_words", "enabled"), [int(x) for x in info])), cells[:got], pool

    # The entries of a kind whose length the frame's size fixes -- doubles, bytes, the character-cell texts, the kitty image -- have four call
    # shapes and a fifth for the formatting alone: one helper each, which takes the entry's name.  `frame(width, owned rows)`: the shape of one
    # frame of the kind in host memory.

    @staticmethod
    def _camera_batch(cameras):
        cams = np.ascontiguousarray(cameras, dtype=np.float64)
        if cams.ndim != 2 or cams.shape[1] != 15:
            raise ValueError("cameras: float64 [n, 15] (Camera, TRT.c:178-184)")
        return cams

    def _render_device(self, entry, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        cam = camera_struct(camera_array)
        _check(getattr(lib(), entry)(self._h, C.byref(cam), C.byref(rows), bounce_limit, rays_per_pixel, _VP(device_ptr), capacity_bytes))

    def _render_host(self, entry, frame, camera_array, rows, bounce_limit, rays_per_pixel, dtype=np.uint8):
        out = np.zeros(frame(rows.width, lib().trt_rowset_rows(C.byref(rows))), dtype=dtype)
        cam = camera_struct(camera_array)
        _check(getattr(lib(), entry)(self._h, C.byref(cam), C.byref(rows), bounce_limit, rays_per_pixel, out.ctypes.data))
        return out

    def _render_device_batch(self, entry, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        cams = self._camera_batch(cameras)
        _check(getattr(lib(), entry)(self._h, cams.ctypes.data, cams.shape[0], C.byref(rows), bounce_limit, rays_per_pixel, _VP(device_ptr), capacity_bytes))

    def _render_host_batch(self, entry, frame, cameras, rows, bounce_limit, rays_per_pixel, dtype=np.uint8):
        cams = self._camera_batch(cameras)
        out = np.zeros((cams.shape[0], *np.atleast_1d(frame(rows.width, lib().trt_rowset_rows(C.byref(rows))))), dtype=dtype)
        _check(getattr(lib(), entry)(self._h, cams.ctypes.data, cams.shape[0], C.byref(rows), bounce_limit, rays_per_pixel, out.ctypes.data))
        return out

    def _text_from_rgb8(self, entry, rgb_ptr, width, rows, text_ptr):
        _check(getattr(lib(), entry)(self._h, _VP(rgb_ptr), width, rows, _VP(text_ptr)))

    def render_device(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        self._render_device("trt_render_device", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_device_rgb8(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """the frame as the emitter's bytes in device memory, 3 per pixel at any alignment, written by the ordered-mean pass itself
        (trt_render_device_rgb8)"""
        self._render_device("trt_render_device_rgb8", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def quantize_device(self, device_ptr, num_pixels, rgb_ptr):
        _check(lib().trt_quantize_device(self._h, _VP(device_ptr), num_pixels, _VP(rgb_ptr)))

    def render_host(self, camera_array, rows, bounce_limit, rays_per_pixel):
        return self._render_host("trt_render_host", _pixels, camera_array, rows, bounce_limit, rays_per_pixel, dtype=np.float64)

    def render_host_rgb8(self, camera_array, rows, bounce_limit, rays_per_pixel):
        """the frame as the emitter's bytes, (int)(c*255) done on the device: uint8 [rows, width, 3] (trt_render_host_rgb8)"""
        return self._render_host("trt_render_host_rgb8", _pixels, camera_array, rows, bounce_limit, rays_per_pixel)

    def render_device_ansi(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """the frame as the terminal's text in device memory, ansi_bytes(width, owned rows) bytes at any alignment, formatted by the
        ordered-mean pass itself (trt_render_device_ansi)"""
        self._render_device("trt_render_device_ansi", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_ansi(self, camera_array, rows, bounce_limit, rays_per_pixel):
        """the frame as the terminal's text, formatted on the device: uint8 [ansi_bytes(width, owned rows)] (trt_render_host_ansi)"""
        return self._render_host("trt_render_host_ansi", ansi_bytes, camera_array, rows, bounce_limit, rays_per_pixel)

    def ansi_from_rgb8(self, rgb_ptr, width, rows, text_ptr):
        """the text of a width x rows frame of RGB8 bytes in device memory, at text_ptr (trt_ansi_from_rgb8_device)"""
        self._text_from_rgb8("trt_ansi_from_rgb8_device", rgb_ptr, width, rows, text_ptr)

    def render_device_ansi_half(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """the frame as the half-block text in device memory, two owned rows per line of text: ansi_half_bytes(width, owned rows) bytes at
        any alignment, formatted by the ordered-mean pass itself (trt_render_device_ansi_half)"""
        self._render_device("trt_render_device_ansi_half", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_ansi_half(self, camera_array, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [ansi_half_bytes(width, owned rows)] (trt_render_host_ansi_half)"""
        return self._render_host("trt_render_host_ansi_half", ansi_half_bytes, camera_array, rows, bounce_limit, rays_per_pixel)

    def ansi_half_from_rgb8(self, rgb_ptr, width, rows, text_ptr):
        """the half-block text of a width x rows frame of RGB8 bytes in device memory, at text_ptr (trt_ansi_half_from_rgb8_device)"""
        self._text_from_rgb8("trt_ansi_half_from_rgb8_device", rgb_ptr, width, rows, text_ptr)

    def render_device_kitty(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """the frame as a kitty graphics-protocol image in device memory: kitty_bytes(width, owned rows) bytes at any alignment, formatted
        by the ordered-mean pass itself (trt_render_device_kitty)"""
        self._render_device("trt_render_device_kitty", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_kitty(self, camera_array, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [kitty_bytes(width, owned rows)] (trt_render_host_kitty)"""
        return self._render_host("trt_render_host_kitty", kitty_bytes, camera_array, rows, bounce_limit, rays_per_pixel)

    def kitty_from_rgb8(self, rgb_ptr, width, rows, text_ptr):
        """the kitty image of a width x rows frame of RGB8 bytes in device memory, at text_ptr (trt_kitty_from_rgb8_device)"""
        self._text_from_rgb8("trt_kitty_from_rgb8_device", rgb_ptr, width, rows, text_ptr)

    def render_batch_kitty(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """cameras[n, 15] as kitty images in device memory; frame b at device_ptr + b * kitty_bytes(width, owned rows)
        (trt_render_device_batch_kitty)"""
        self._render_device_batch("trt_render_device_batch_kitty", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch_kitty(self, cameras, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [n, kitty_bytes(width, owned rows)] (trt_render_host_batch_kitty)"""
        return self._render_host_batch("trt_render_host_batch_kitty", kitty_bytes, cameras, rows, bounce_limit, rays_per_pixel)

    # the texts in the xterm 256-colour palette come in the same two kinds of cell; `half` chooses the half-block entry of each pair

    def render_device_ansi256(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, half=False):
        """the frame as the 256-colour text in device memory: ansi256_bytes(width, owned rows, half) bytes at any alignment, mapped to the
        palette and formatted by the ordered-mean pass itself (trt_render_device_ansi256, trt_render_device_ansi256_half)"""
        self._render_device("trt_render_device_ansi256" + _half(half), camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_ansi256(self, camera_array, rows, bounce_limit, rays_per_pixel, half=False):
        """the same into host memory: uint8 [ansi256_bytes(width, owned rows, half)] (trt_render_host_ansi256, trt_render_host_ansi256_half)"""
        return self._render_host("trt_render_host_ansi256" + _half(half), functools.partial(ansi256_bytes, half=half), camera_array, rows, bounce_limit, rays_per_pixel)

    def ansi256_from_rgb8(self, rgb_ptr, width, rows, text_ptr, half=False):
        """the 256-colour text of a width x rows frame of RGB8 bytes in device memory, at text_ptr (trt_ansi256_from_rgb8_device,
        trt_ansi256_half_from_rgb8_device)"""
        self._text_from_rgb8("trt_ansi256" + _half(half) + "_from_rgb8_device", rgb_ptr, width, rows, text_ptr)

    def xterm256_from_rgb8(self, rgb_ptr, num_pixels, index_ptr):
        """the palette index 16..255 of each of num_pixels pixels of RGB8 bytes in device memory, a byte each at index_ptr
        (trt_xterm256_from_rgb8_device)"""
        _check(lib().trt_xterm256_from_rgb8_device(self._h, _VP(rgb_ptr), num_pixels, _VP(index_ptr)))

    def render_batch_ansi256(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, half=False):
        """cameras[n, 15] as 256-colour texts in device memory; frame b at device_ptr + b * ansi256_bytes(width, owned rows, half)
        (trt_render_device_batch_ansi256, trt_render_device_batch_ansi256_half)"""
        self._render_device_batch("trt_render_device_batch_ansi256" + _half(half), cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch_ansi256(self, cameras, rows, bounce_limit, rays_per_pixel, half=False):
        """the same into host memory: uint8 [n, ansi256_bytes(width, owned rows, half)] (trt_render_host_batch_ansi256,
        trt_render_host_batch_ansi256_half)"""
        return self._render_host_batch("trt_render_host_batch_ansi256" + _half(half), functools.partial(ansi256_bytes, half=half), cameras, rows, bounce_limit, rays_per_pixel)

    # the delta entries come in two kinds of cell, the full text's and half-block cells: each pair goes through one helper that takes the entry's name

    def _delta_from_rgb8(self, entry, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        _check(getattr(lib(), entry)(self._h, _VP(shown_ptr), _VP(next_ptr), width, rows, _VP(text_ptr), capacity_bytes, _VP(bytes_ptr)))

    def _delta_kernel_times(self, entry, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        ms = (C.c_float * 3)()
        _check(getattr(lib(), entry)(self._h, _VP(shown_ptr), _VP(next_ptr), width, rows, _VP(text_ptr), capacity_bytes, _VP(bytes_ptr), ms))
        return tuple(ms)

    def _render_device_delta(self, entry, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        cam = camera_struct(camera_array)
        _check(getattr(lib(), entry)(self._h, C.byref(cam), C.byref(rows), bounce_limit, rays_per_pixel, _VP(device_ptr), capacity_bytes, _VP(bytes_ptr)))

    def _render_host_delta(self, entry, capacity, camera_array, rows, bounce_limit, rays_per_pixel, out):
        if out is None:
            out = np.empty(capacity(rows.width, lib().trt_rowset_rows(C.byref(rows))), dtype=np.uint8)
        n = _SZ(0)
        cam = camera_struct(camera_array)
        _check(getattr(lib(), entry)(self._h, C.byref(cam), C.byref(rows), bounce_limit, rays_per_pixel, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value]

    def ansi_delta_from_rgb8(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the delta text between two width x rows frames of RGB8 bytes in device memory, at text_ptr, its length (a uint64) at the device
        address bytes_ptr (trt_ansi_delta_from_rgb8_device)"""
        self._delta_from_rgb8("trt_ansi_delta_from_rgb8_device", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi_delta_kernel_times(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the same, synchronous: ms of the (measure, offsets, write) kernels by HIP events (trt_ansi_delta_kernel_times)"""
        return self._delta_kernel_times("trt_ansi_delta_kernel_times", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def render_device_ansi_delta(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        """the frame as the delta text against the context's shown frame (a keyframe when there is none for this rowset) in device memory,
        its length (a uint64) at the device address bytes_ptr (trt_render_device_ansi_delta)"""
        self._render_device_delta("trt_render_device_ansi_delta", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_host_ansi_delta(self, camera_array, rows, bounce_limit, rays_per_pixel, out=None):
        """the same into host memory: the uint8 text, exactly as long as the host is to write it (trt_render_host_ansi_delta); `out`: a
        uint8 buffer of ansi_delta_capacity bytes to reuse"""
        return self._render_host_delta("trt_render_host_ansi_delta", ansi_delta_capacity, camera_array, rows, bounce_limit, rays_per_pixel, out)

    def ansi_delta_reset(self):
        """forget the shown frame: the next delta text, of any of the four kinds, is a keyframe (trt_ansi_delta_reset)"""
        _check(lib().trt_ansi_delta_reset(self._h))

    def ansi_delta_half_from_rgb8(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the delta text in half-block cells between two width x rows frames of RGB8 bytes in device memory, at text_ptr, its length (a
        uint64) at the device address bytes_ptr (trt_ansi_delta_half_from_rgb8_device)"""
        self._delta_from_rgb8("trt_ansi_delta_half_from_rgb8_device", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi_delta_half_kernel_times(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the same, synchronous: ms of the (measure, offsets, write) kernels by HIP events (trt_ansi_delta_half_kernel_times)"""
        return self._delta_kernel_times("trt_ansi_delta_half_kernel_times", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def render_device_ansi_delta_half(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        """the frame as the half-block delta text against the context's shown frame (a keyframe, the half-block text, when there is none
        for this rowset and this kind) in device memory, its length (a uint64) at the device address bytes_ptr
        (trt_render_device_ansi_delta_half)"""
        self._render_device_delta("trt_render_device_ansi_delta_half", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_host_ansi_delta_half(self, camera_array, rows, bounce_limit, rays_per_pixel, out=None):
        """the same into host memory: the uint8 text, exactly as long as the host is to write it (trt_render_host_ansi_delta_half); `out`:
        a uint8 buffer of ansi_delta_half_capacity bytes to reuse"""
        return self._render_host_delta("trt_render_host_ansi_delta_half", ansi_delta_half_capacity, camera_array, rows, bounce_limit, rays_per_pixel, out)

    # the delta entries in the xterm 256-colour palette: the 24-bit ones' helpers, `half` choosing the cells as in the ansi256 entries

    def ansi256_delta_from_rgb8(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr, half=False):
        """ansi_delta_from_rgb8 (half: ansi_delta_half_from_rgb8) in the palette: a cell has a record where its palette index changed
        (trt_ansi256_delta_from_rgb8_device, trt_ansi256_delta_half_from_rgb8_device)"""
        self._delta_from_rgb8("trt_ansi256_delta" + _half(half) + "_from_rgb8_device", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi256_delta_kernel_times(self, shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr, half=False):
        """the same, synchronous: ms of the (measure, offsets, write) kernels by HIP events (trt_ansi256_delta_kernel_times,
        trt_ansi256_delta_half_kernel_times)"""
        return self._delta_kernel_times("trt_ansi256_delta" + _half(half) + "_kernel_times", shown_ptr, next_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def render_device_ansi256_delta(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr, half=False):
        """the frame as the 256-colour delta text against the context's shown frame (a keyframe, the whole 256-colour text, when there is
        none for this rowset and this kind) in device memory, its length (a uint64) at the device address bytes_ptr
        (trt_render_device_ansi256_delta, trt_render_device_ansi256_delta_half)"""
        self._render_device_delta("trt_render_device_ansi256_delta" + _half(half), camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_host_ansi256_delta(self, camera_array, rows, bounce_limit, rays_per_pixel, out=None, half=False):
        """the same into host memory: the uint8 text, exactly as long as the host is to write it (trt_render_host_ansi256_delta,
        trt_render_host_ansi256_delta_half); `out`: a uint8 buffer of ansi256_delta_capacity bytes to reuse"""
        return self._render_host_delta("trt_render_host_ansi256_delta" + _half(half), functools.partial(ansi256_delta_capacity, half=half), camera_array, rows,
                                       bounce_limit, rays_per_pixel, out)

    # the sixel image: a text whose length depends on the picture, reported as the delta entries report theirs

    def sixel_from_rgb8(self, rgb_ptr, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the DEC sixel image of a width x rows frame of RGB8 bytes in device memory, at text_ptr, its length (a uint64) at the device
        address bytes_ptr (trt_sixel_from_rgb8_device)"""
        _check(lib().trt_sixel_from_rgb8_device(self._h, _VP(rgb_ptr), width, rows, _VP(text_ptr), capacity_bytes, _VP(bytes_ptr)))

    def render_device_sixel(self, camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        """the frame as a DEC sixel image in device memory, at any alignment, its length (a uint64) at the device address bytes_ptr
        (trt_render_device_sixel)"""
        self._render_device_delta("trt_render_device_sixel", camera_array, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_host_sixel(self, camera_array, rows, bounce_limit, rays_per_pixel, out=None):
        """the same into host memory: the uint8 image, exactly as long as the host is to write it (trt_render_host_sixel); `out`: a uint8
        buffer of sixel_capacity bytes to reuse"""
        return self._render_host_delta("trt_render_host_sixel", sixel_capacity, camera_array, rows, bounce_limit, rays_per_pixel, out)

    def render_device_batch(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """cameras[n, 15] of the current scene in one call; frame b at device_ptr + b * rows * width * 24 (trt_render_device_batch)"""
        self._render_device_batch("trt_render_device_batch", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch(self, cameras, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: float64 [n, rows, width, 3] (trt_render_host_batch)"""
        return self._render_host_batch("trt_render_host_batch", _pixels, cameras, rows, bounce_limit, rays_per_pixel, dtype=np.float64)

    def render_batch_rgb8(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """cameras[n, 15] as the emitter's bytes in device memory; frame b at device_ptr + b * rows * width * 3 (trt_render_device_batch_rgb8)"""
        self._render_device_batch("trt_render_device_batch_rgb8", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch_rgb8(self, cameras, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [n, rows, width, 3] (trt_render_host_batch_rgb8)"""
        return self._render_host_batch("trt_render_host_batch_rgb8", _pixels, cameras, rows, bounce_limit, rays_per_pixel)

    def render_batch_ansi(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """cameras[n, 15] as the terminal's text in device memory; frame b at device_ptr + b * ansi_bytes(width, owned rows)
        (trt_render_device_batch_ansi)"""
        self._render_device_batch("trt_render_device_batch_ansi", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch_ansi(self, cameras, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [n, ansi_bytes(width, owned rows)] (trt_render_host_batch_ansi)"""
        return self._render_host_batch("trt_render_host_batch_ansi", ansi_bytes, cameras, rows, bounce_limit, rays_per_pixel)

    def render_batch_ansi_half(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes):
        """cameras[n, 15] as the half-block text in device memory; frame b at device_ptr + b * ansi_half_bytes(width, owned rows)
        (trt_render_device_batch_ansi_half)"""
        self._render_device_batch("trt_render_device_batch_ansi_half", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes)

    def render_host_batch_ansi_half(self, cameras, rows, bounce_limit, rays_per_pixel):
        """the same into host memory: uint8 [n, ansi_half_bytes(width, owned rows)] (trt_render_host_batch_ansi_half)"""
        return self._render_host_batch("trt_render_host_batch_ansi_half", ansi_half_bytes, cameras, rows, bounce_limit, rays_per_pixel)

    # the batch forms of the delta entries, of both kinds of cell: n texts back to back, one helper per pair of entries

    def _delta_chain_from_rgb8(self, entry, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        _check(getattr(lib(), entry)(self._h, _VP(shown_ptr), _VP(frames_ptr), n, width, rows, _VP(text_ptr), capacity_bytes, _VP(bytes_ptr)))

    def _delta_chain_kernel_times(self, entry, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        ms = (C.c_float * 3)()
        _check(getattr(lib(), entry)(self._h, _VP(shown_ptr), _VP(frames_ptr), n, width, rows, _VP(text_ptr), capacity_bytes, _VP(bytes_ptr), ms))
        return tuple(ms)

    def _render_device_batch_delta(self, entry, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        cams = self._camera_batch(cameras)
        _check(getattr(lib(), entry)(self._h, cams.ctypes.data, cams.shape[0], C.byref(rows), bounce_limit, rays_per_pixel, _VP(device_ptr), capacity_bytes,
                                     _VP(bytes_ptr)))

    def _render_host_batch_delta(self, entry, capacity, cameras, rows, bounce_limit, rays_per_pixel, out):
        cams = self._camera_batch(cameras)
        if out is None:
            out = np.empty(cams.shape[0] * capacity(rows.width, lib().trt_rowset_rows(C.byref(rows))), dtype=np.uint8)
        lengths = (_SZ * max(cams.shape[0], 1))()
        _check(getattr(lib(), entry)(self._h, cams.ctypes.data, cams.shape[0], C.byref(rows), bounce_limit, rays_per_pixel, out.ctypes.data, out.size, lengths))
        ends = np.cumsum([int(k) for k in lengths])
        return [out[end - int(k):end] for k, end in zip(lengths, ends)]

    def ansi_delta_chain_from_rgb8(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the n delta texts of a chain -- the shown frame at shown_ptr, n frames of RGB8 bytes back to back at frames_ptr, text b between
        frames b - 1 and b -- back to back at text_ptr, their lengths (n uint64) at the device address bytes_ptr
        (trt_ansi_delta_chain_from_rgb8_device)"""
        self._delta_chain_from_rgb8("trt_ansi_delta_chain_from_rgb8_device", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi_delta_half_chain_from_rgb8(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the same in half-block cells (trt_ansi_delta_half_chain_from_rgb8_device)"""
        self._delta_chain_from_rgb8("trt_ansi_delta_half_chain_from_rgb8_device", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi_delta_chain_kernel_times(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """ansi_delta_chain_from_rgb8, synchronous: ms of the (measure, offsets, write) kernels by HIP events (trt_ansi_delta_chain_kernel_times)"""
        return self._delta_chain_kernel_times("trt_ansi_delta_chain_kernel_times", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi_delta_half_chain_kernel_times(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr):
        """the same in half-block cells (trt_ansi_delta_half_chain_kernel_times)"""
        return self._delta_chain_kernel_times("trt_ansi_delta_half_chain_kernel_times", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def render_device_batch_ansi_delta(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        """cameras[n, 15] as n delta texts back to back in device memory: text 0 against the context's shown frame (the keyframe when there
        is none), text b against frame b - 1 of the batch; their lengths (n uint64) at the device address bytes_ptr
        (trt_render_device_batch_ansi_delta)"""
        self._render_device_batch_delta("trt_render_device_batch_ansi_delta", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_device_batch_ansi_delta_half(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr):
        """the same in half-block cells (trt_render_device_batch_ansi_delta_half)"""
        self._render_device_batch_delta("trt_render_device_batch_ansi_delta_half", cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr)

    def render_host_batch_ansi_delta(self, cameras, rows, bounce_limit, rays_per_pixel, out=None):
        """the same into host memory: a list of n uint8 texts, each as long as the host is to write it (trt_render_host_batch_ansi_delta);
        `out`: a uint8 buffer of n * ansi_delta_capacity bytes to reuse, of which the texts are views"""
        return self._render_host_batch_delta("trt_render_host_batch_ansi_delta", ansi_delta_capacity, cameras, rows, bounce_limit, rays_per_pixel, out)

    def render_host_batch_ansi_delta_half(self, cameras, rows, bounce_limit, rays_per_pixel, out=None):
        """the same in half-block cells (trt_render_host_batch_ansi_delta_half); `out`: n * ansi_delta_half_capacity bytes"""
        return self._render_host_batch_delta("trt_render_host_batch_ansi_delta_half", ansi_delta_half_capacity, cameras, rows, bounce_limit, rays_per_pixel, out)

    def ansi256_delta_chain_from_rgb8(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr, half=False):
        """ansi_delta_chain_from_rgb8 in the palette (trt_ansi256_delta_chain_from_rgb8_device, trt_ansi256_delta_half_chain_from_rgb8_device)"""
        self._delta_chain_from_rgb8("trt_ansi256_delta" + _half(half) + "_chain_from_rgb8_device", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr)

    def ansi256_delta_chain_kernel_times(self, shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes, bytes_ptr, half=False):
        """the same, synchronous: ms of the (measure, offsets, write) kernels by HIP events (trt_ansi256_delta_chain_kernel_times,
        trt_ansi256_delta_half_chain_kernel_times)"""
        return self._delta_chain_kernel_times("trt_ansi256_delta" + _half(half) + "_chain_kernel_times", shown_ptr, frames_ptr, n, width, rows, text_ptr, capacity_bytes,
                                              bytes_ptr)

    def render_device_batch_ansi256_delta(self, cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes, bytes_ptr, half=False):
        """render_device_batch_ansi_delta in the palette (trt_render_device_batch_ansi256_delta, trt_render_device_batch_ansi256_delta_half)"""
        self._render_device_batch_delta("trt_render_device_batch_ansi256_delta" + _half(half), cameras, rows, bounce_limit, rays_per_pixel, device_ptr, capacity_bytes,
                                        bytes_ptr)

    def render_host_batch_ansi256_delta(self, cameras, rows, bounce_limit, rays_per_pixel, out=None, half=False):
        """the same into host memory: a list of n uint8 texts (trt_render_host_batch_ansi256_delta, trt_render_host_batch_ansi256_delta_half);
        `out`: n * ansi256_delta_capacity bytes"""
        return self._render_host_batch_delta("trt_render_host_batch_ansi256_delta" + _half(half), functools.partial(ansi256_delta_capacity, half=half), cameras, rows,
                                             bounce_limit, rays_per_pixel, out)

    def batch_info(self):
        """(frames, render-kernel launches) of this context's most recent batch call (trt_batch_info)"""
        n, k = _I(), _I()
        _check(lib().trt_batch_info(self._h, C.byref(n), C.byref(k)))
        return n.value, k.value

    def synchronize(self):
        _check(lib().trt_synchronize(self._h))

    def kernel_times(self, max_count=256):
        buf = (C.c_float * max_count)()
        n = lib().trt_kernel_times(self._h, buf, max_count)
        if n < 0:
            _check(n)
        return [buf[i] for i in range(n)]

    def render_kernel_times(self, max_count=256):
        """(render_ms[], reduce_ms[]) of the most recent launches: the render kernel alone and the ordered mean"""
        a, b = (C.c_float * max_count)(), (C.c_float * max_count)()
        n = lib().trt_render_kernel_times(self._h, a, b, max_count)
        if n < 0:
            _check(n)
        return [a[i] for i in range(n)], [b[i] for i in range(n)]

    def launch_count(self):
        """frames this context has launched so far (trt_launch_count)"""
        return int(lib().trt_launch_count(self._h))

    def launch_span_ms(self, first_launch, last, last_launch):
        """device ms from the start of this context's launch `first_launch` to the end of context `last`'s launch `last_launch` (trt_launch_span_ms)"""
        ms = C.c_float()
        _check(lib().trt_launch_span_ms(self._h, first_launch, last._h, last_launch, C.byref(ms)))
        return float(ms.value)

    def enable_counters(self, on=True):
        _check(lib().trt_enable_counters(self._h, 1 if on else 0))

    def read_counters(self):
        p, s = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().trt_read_counters(self._h, C.byref(p), C.byref(s)))
        return p.value, s.value

    def read_diagnostics(self):
        t, p = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().trt_read_diagnostics(self._h, C.byref(t), C.byref(p)))
        v = C.c_ulonglong()
        _check(lib().trt_read_shading_passes(self._h, C.byref(v)))
        loops = (C.c_ulonglong * 8)()
        _check(lib().trt_read_loop_diagnostics(self._h, loops))
        kinds = ("path", "directional", "point")
        return {"wave_loop_trips": t.value, "phase2_rounds": p.value, "swept_traces": self.read_sweep_fallbacks(), "shading_passes": v.value,
                "exact_loop_iterations": {k: int(loops[i]) for i, k in enumerate(kinds)},
                "exact_loop_lane_activity": {k: round(loops[3 + i] / max(1, 64 * loops[i]), 4) for i, k in enumerate(kinds)},
                "point_light_closest_hit_fallbacks": int(loops[6])}

    def kernel_info(self):
        v = [_I() for _ in range(5)]
        _check(lib().trt_kernel_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("vgprs", "sgprs", "static_lds_bytes", "max_blocks_per_cu", "compute_units"),
                        [x.value for x in v]))

    def selftest_div_sqrt(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        q, r = np.empty_like(a), np.empty_like(a)
        _check(lib().trt_selftest_div_sqrt(self._h, a.ctypes.data, b.ctypes.data, a.size, q.ctypes.data, r.ctypes.data))
        return q, r

    def probe_rays(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        obj = np.zeros(n, dtype=np.int32)
        point, normal, material, lit = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 5)), np.zeros((n, 3))
        _check(lib().trt_probe_rays(self._h, rays.ctypes.data, n, obj.ctypes.data, point.ctypes.data,
                                    normal.ctypes.data, material.ctypes.data, lit.ctypes.data))
        return obj, point, normal, material, lit


    def probe_rays_production(self, camera_array, rays, families=None):
        """trt_probe_rays_production: the probe through the production kernel's stages (tables, sweep, exact tests, lighting)"""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        fam = None if families is None else np.ascontiguousarray(families, dtype=np.int32)
        obj = np.zeros(n, dtype=np.int32)
        point, normal, material, lit = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 5)), np.zeros((n, 3))
        cam = camera_struct(camera_array)
        _check(lib().trt_probe_rays_production(self._h, C.byref(cam), rays.ctypes.data, None if fam is None else fam.ctypes.data, n,
                                               obj.ctypes.data, point.ctypes.data, normal.ctypes.data, material.ctypes.data, lit.ctypes.data))
        return obj, point, normal, material, lit

    def probe_path_lookups(self, cameras, rays, families, frames=None):
        """trt_probe_path_lookups: where the render kernels' own look-up reads a path ray's list cell.  cameras [15] or [n, 15] (2 to 8: the
        batch form, frames[i] the frame of ray i).  Returns a dict of arrays: fallback, word, successor, read_at, region, table, cell."""
        cams = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 15)
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        fam = np.ascontiguousarray(families, dtype=np.int32)
        frm = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        assert fam.shape == (n,) and (frm is None or frm.shape == (n,))
        fallback, successor = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        word, read_at, place = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros((n, 3), dtype=np.int32)
        _check(lib().trt_probe_path_lookups(self._h, cams.ctypes.data, cams.shape[0], rays.ctypes.data, fam.ctypes.data,
                                            None if frm is None else frm.ctypes.data, n, fallback.ctypes.data, word.ctypes.data,
                                            successor.ctypes.data, read_at.ctypes.data, place.ctypes.data))
        return {"fallback": fallback, "word": word, "successor": successor, "read_at": read_at,
                "region": place[:, 0].copy(), "table": place[:, 1].copy(), "cell": place[:, 2].copy()}

    def probe_shadow_lookups(self, origins, light):
        """trt_probe_shadow_lookups: the shading stage's look-up of one light (directional lights first) per origin.  Returns a dict of arrays:
        far, cell, word and, for a point light, lo and hi."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        far, cell, word = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
        lo, hi = np.zeros(n), np.zeros(n)
        _check(lib().trt_probe_shadow_lookups(self._h, o.ctypes.data, n, int(light), far.ctypes.data, cell.ctypes.data, word.ctypes.data,
                                              lo.ctypes.data, hi.ctypes.data))
        return {"far": far, "cell": cell, "word": word, "lo": lo, "hi": hi}

    def selftest_filter(self, rays, num_spheres, fixed_dir=True):
        """trt_selftest_filter: (fields uint32 [n, 9], sign uint32 [spheres, n], sign_fixed uint32 [spheres, n] or None) of the FP32 filter's
        set-up and sign words as the device computes them for the current scene of num_spheres spheres"""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        fields, sign = np.zeros((n, 9), dtype=np.uint32), np.zeros((num_spheres, n), dtype=np.uint32)
        fixed = np.zeros((num_spheres, n), dtype=np.uint32) if fixed_dir else None
        _check(lib().trt_selftest_filter(self._h, rays.ctypes.data, n, fields.ctypes.data, sign.ctypes.data,
                                         None if fixed is None else fixed.ctypes.data))
        return fields, sign, fixed


def default_context():
    """The default context of the drop-in entries as a borrowed Context, None while there is none (trt_default_context); it dangles
    once trt_shutdown has run."""
    h = lib().trt_default_context()
    return Context(0, _borrowed=h) if h else None


def render_frame(scene_data, width, height, bounce_limit=10, rays_per_pixel=10, symbol="trt_render_frame"):
    """Host-in/host-out frame through the extended entry trt_render_frame, or its alias render_frame (default context)."""
    from .scenes import new_screen
    scene = scene_data.as_scene()
    screen, pixels = new_screen(width, height)
    _check(getattr(lib(), symbol)(C.byref(scene), C.byref(screen), bounce_limit, rays_per_pixel))
    return pixels


def render_frame_rgb8(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in, emitter-bytes-out frame: uint8 [height, width, 3] = (int)(c*255) formed on the device (trt_render_frame_rgb8)."""
    scene = scene_data.as_scene()
    out = np.zeros((height, width, 3), dtype=np.uint8)
    _check(lib().trt_render_frame_rgb8(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data))
    return out


def set_default_specular(on=True):
    """EXTENSION, parity unpinned: the specular extension for the default context behind project_scene and the trt_render_frame_*
    entries, until trt_shutdown (trt_set_default_specular)"""
    _check(lib().trt_set_default_specular(int(on)))


SKY_NEAREST, SKY_BILINEAR = 0, 1


def set_default_sky_filter(mode=SKY_BILINEAR):
    """EXTENSION, parity unpinned: the sky filter of the default context behind project_scene and the trt_render_frame_* entries, until
    trt_shutdown (trt_set_default_sky_filter)"""
    _check(lib().trt_set_default_sky_filter(int(mode)))


def ansi_bytes(width, rows):
    """length of the terminal's text of a width x rows screen: 8 + (25 * width + 1) * rows + 1, 0 unless both are positive (trt_ansi_bytes)"""
    return int(lib().trt_ansi_bytes(width, rows))


def ansi_half_bytes(width, rows):
    """length of the half-block text of a width x rows screen: 6 + (39 * width + 5) * ((rows + 1) // 2), 0 unless both are positive
    (trt_ansi_half_bytes)"""
    return int(lib().trt_ansi_half_bytes(width, rows))


def kitty_bytes(width, rows):
    """length of the kitty graphics-protocol image of a width x rows screen: 4 P + 10 ceil(P / 1024) + 46, P = width * rows; 0 unless both
    are positive and at most 99999 (trt_kitty_bytes)"""
    return int(lib().trt_kitty_bytes(width, rows))


def _half(half):
    return "_half" if half else ""


def _pixels(width, rows):
    """the shape of a frame of pixels in host memory, as doubles or as the emitter's bytes"""
    return rows, width, 3


def ansi256_bytes(width, rows, half=False):
    """length of the text of a width x rows screen in the xterm 256-colour palette: 6 + (13 * width + 5) * rows, or for half-block cells
    6 + (23 * width + 5) * ((rows + 1) // 2); 0 unless both are positive (trt_ansi256_bytes, trt_ansi256_half_bytes)"""
    return int(getattr(lib(), "trt_ansi256" + _half(half) + "_bytes")(width, rows))


def _header_constant(header, name):
    """an integer #define of a header under csrc/: the layout headers are what the kernels compile, the binding reads them, it does not restate them"""
    import re
    with open(os.path.join(_HERE, "csrc", header)) as fh:
        return int(re.search(r"^#define\s+" + name + r"\s+(\d+)", fh.read(), re.M).group(1))


# words of the half-block text a wave of the device pass stores (csrc/trt_ansi_half.h): a wave's span is four times as many bytes
ANSI_HALF_WAVE_WORDS = _header_constant("trt_ansi_half.h", "TRT_ANSI_HALF_WAVE_WORDS")


def _delta_capacity(entry, width, rows):
    return int(getattr(lib(), entry)(width, rows))


def _render_frame_delta(entry, capacity, scene_data, width, height, bounce_limit, rays_per_pixel):
    scene = scene_data.as_scene()
    out = np.empty(capacity(width, height), dtype=np.uint8)
    n = _SZ(0)
    _check(getattr(lib(), entry)(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data, out.size, C.byref(n)))
    return out[:n.value]


def ansi_delta_capacity(width, rows):
    """room for any text the delta entries write: max(ansi_bytes, rows * (21 * width + 18)); 0 when a size is not positive or above the
    format's limits (trt_ansi_delta_capacity)"""
    return _delta_capacity("trt_ansi_delta_capacity", width, rows)


def render_frame_ansi_delta(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in frame as the delta text against the frame this entry returned before (a keyframe the first time): the uint8 text, as
    long as the host is to write it (trt_render_frame_ansi_delta)."""
    return _render_frame_delta("trt_render_frame_ansi_delta", ansi_delta_capacity, scene_data, width, height, bounce_limit, rays_per_pixel)


def sixel_capacity(width, rows):
    """room for any DEC sixel image of a width x rows screen: 4352 + L * the sum over the bands of six rows of min(240, the band's pixels),
    L = 4 + width + T; 0 unless both sizes are positive and at most 99999 (trt_sixel_capacity)"""
    return _delta_capacity("trt_sixel_capacity", width, rows)


def render_frame_sixel(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in frame as a DEC sixel image in the 240 fixed colours of the xterm palette, formatted on the device: the uint8 text, as long
    as the host is to write it (trt_render_frame_sixel)."""
    return _render_frame_delta("trt_render_frame_sixel", sixel_capacity, scene_data, width, height, bounce_limit, rays_per_pixel)


def ansi_delta_half_capacity(width, rows):
    """room for any text the half-block delta entries write: max(ansi_half_bytes, ((rows + 1) // 2) * (39 * width + 18)); 0 when a size
    is not positive or above the format's limits (trt_ansi_delta_half_capacity)"""
    return _delta_capacity("trt_ansi_delta_half_capacity", width, rows)


def render_frame_ansi_delta_half(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in frame as the half-block delta text against the frame this entry returned before (a keyframe the first time): the uint8
    text, as long as the host is to write it (trt_render_frame_ansi_delta_half)."""
    return _render_frame_delta("trt_render_frame_ansi_delta_half", ansi_delta_half_capacity, scene_data, width, height, bounce_limit, rays_per_pixel)


def ansi256_delta_capacity(width, rows, half=False):
    """room for any text the 256-colour delta entries write, the whole 256-colour text or the longest delta: rows * (13 * width + 13 +
    5 * ((width + 1) // 2)), half: ((rows + 1) // 2) * (23 * width + 18); 0 when a size is not positive or above the format's limits
    (trt_ansi256_delta_capacity, trt_ansi256_delta_half_capacity)"""
    return _delta_capacity("trt_ansi256_delta" + _half(half) + "_capacity", width, rows)


def render_frame_ansi256_delta(scene_data, width, height, bounce_limit=10, rays_per_pixel=10, half=False):
    """Host-in frame as the 256-colour delta text against the frame this entry returned before (a keyframe the first time, and after a
    delta entry of another kind): the uint8 text, as long as the host is to write it (trt_render_frame_ansi256_delta,
    trt_render_frame_ansi256_delta_half)."""
    return _render_frame_delta("trt_render_frame_ansi256_delta" + _half(half), functools.partial(ansi256_delta_capacity, half=half), scene_data, width, height,
                               bounce_limit, rays_per_pixel)


def render_frame_ansi(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in, terminal-text-out frame: uint8 [ansi_bytes(width, height)], what buffered_draw_screen writes, formatted on the device
    (trt_render_frame_ansi)."""
    scene = scene_data.as_scene()
    out = np.zeros(ansi_bytes(width, height), dtype=np.uint8)
    _check(lib().trt_render_frame_ansi(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data))
    return out


def render_frame_ansi_half(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in, half-block-text-out frame: uint8 [ansi_half_bytes(width, height)], two pixel rows per line of text, formatted on the
    device (trt_render_frame_ansi_half)."""
    scene = scene_data.as_scene()
    out = np.zeros(ansi_half_bytes(width, height), dtype=np.uint8)
    _check(lib().trt_render_frame_ansi_half(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data))
    return out


def render_frame_kitty(scene_data, width, height, bounce_limit=10, rays_per_pixel=10):
    """Host-in, kitty-image-out frame: uint8 [kitty_bytes(width, height)], four bytes of text a pixel, formatted on the device
    (trt_render_frame_kitty)."""
    scene = scene_data.as_scene()
    out = np.zeros(kitty_bytes(width, height), dtype=np.uint8)
    _check(lib().trt_render_frame_kitty(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data))
    return out


def render_frame_ansi256(scene_data, width, height, bounce_limit=10, rays_per_pixel=10, half=False):
    """Host-in, 256-colour-text-out frame: uint8 [ansi256_bytes(width, height, half)], mapped to the xterm palette and formatted on the
    device (trt_render_frame_ansi256, trt_render_frame_ansi256_half)."""
    scene = scene_data.as_scene()
    out = np.zeros(ansi256_bytes(width, height, half), dtype=np.uint8)
    _check(getattr(lib(), "trt_render_frame_ansi256" + _half(half))(C.byref(scene), width, height, bounce_limit, rays_per_pixel, out.ctypes.data))
    return out


def project_scene(scene_data, width, height):
    """The drop-in symbol itself: void project_scene(Scene*, Screen*) at B=10, spp=10 (TRT.c:966)."""
    from .scenes import new_screen
    scene = scene_data.as_scene()
    screen, pixels = new_screen(width, height)
    lib().project_scene(C.byref(scene), C.byref(screen))
    return pixels


def _dist_check(code):
    if code != TRT_OK:
        raise TrtError(code, lib().trt_dist_last_error().decode())


def dist_allow_rccl_override(allow=True):
    """TEST HOOK: let TRT_RCCL_LIB name the library bound in RCCL's place; before the first use of RCCL (trt_dist_allow_rccl_override)"""
    _dist_check(lib().trt_dist_allow_rccl_override(1 if allow else 0))


def dist_rccl_library():
    """which library this process bound for RCCL's entry points ("" before the first use)"""
    return lib().trt_dist_rccl_library().decode()


def dist_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0; trt_dist_unique_id)"""
    buf = C.create_string_buffer(128)
    _dist_check(lib().trt_dist_unique_id(buf))
    return buf.raw


class Dist:
    """trt_dist: this rank's part of one frame sharded over the GPUs of a node (include/trt_hip.h, section 3).
    Row tiles, the RCCL communicator, the gather and the frame pipeline all live in the library."""

    def __init__(self, device, scene_data, unique_id, rank, world, width, height, tile_rows=8, frames_in_flight=2, reserved_cus=0):
        self._h = _VP()
        self._scene = scene_data.as_scene()
        idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _dist_check(lib().trt_dist_create(device, C.byref(self._scene), idbuf, rank, world, width, height, tile_rows, frames_in_flight,
                                          reserved_cus, C.byref(self._h)))
        self.device, self.rank, self.world, self.width, self.height = device, rank, world, width, height
        self.frames_in_flight = frames_in_flight
        v = [_I() for _ in range(5)]
        _dist_check(lib().trt_dist_info(self._h, *[C.byref(x) for x in v]))
        self.local_rows, self.max_rows = v[2].value, v[3].value

    def context(self, slot=0):
        h = lib().trt_dist_context(self._h, slot)
        if not h:
            raise IndexError(slot)
        return Context(self.device, _borrowed=h)

    def render(self, camera_array, bounce_limit, rays_per_pixel):
        """enqueue one frame; returns the device address of the assembled frame on rank 0 (None elsewhere)"""
        cam = camera_struct(camera_array)
        out = _VP()
        _dist_check(lib().trt_dist_render(self._h, C.byref(cam), bounce_limit, rays_per_pixel, C.byref(out)))
        return out.value

    def synchronize(self):
        _dist_check(lib().trt_dist_synchronize(self._h))

    def fetch(self, device_frame):
        out = np.zeros((self.height, self.width, 3), dtype=np.float64)
        _dist_check(lib().trt_dist_fetch(self._h, _VP(device_frame), out.ctypes.data))
        return out

    def set_scene(self, scene_data):
        """another scene for every frame slot: the first slot builds its tables, the others share them (trt_dist_set_scene)"""
        scene = scene_data.as_scene()
        _dist_check(lib().trt_dist_set_scene(self._h, C.byref(scene)))

    def comm_ranks(self):
        """ranks of the communicator as RCCL reports them (ncclCommCount); 0 without a communicator (trt_dist_comm_ranks)"""
        n = lib().trt_dist_comm_ranks(self._h)
        if n < 0:
            _dist_check(n)
        return n

    def frame_times(self):
        """(render_ms, gather_ms) of this rank, averaged over the slots' most recent frames (trt_dist_frame_times)"""
        r, g = C.c_float(), C.c_float()
        _dist_check(lib().trt_dist_frame_times(self._h, C.byref(r), C.byref(g)))
        return float(r.value), float(g.value)

    def enable_rgb8(self):
        """byte buffers for frames gathered as the emitter's (int)(c*255) triplets (trt_dist_enable_rgb8)"""
        _dist_check(lib().trt_dist_enable_rgb8(self._h))

    def render_rgb8(self, camera_array, bounce_limit, rays_per_pixel):
        cam = camera_struct(camera_array)
        out = _VP()
        _dist_check(lib().trt_dist_render_rgb8(self._h, C.byref(cam), bounce_limit, rays_per_pixel, C.byref(out)))
        return out.value

    def fetch_rgb8(self, device_frame):
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        _dist_check(lib().trt_dist_fetch_rgb8(self._h, _VP(device_frame), out.ctypes.data))
        return out

    def close(self):
        if self._h:
            lib().trt_dist_destroy(self._h)
            self._h = _VP()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""mcpt — host-side mirror of the reference's render-path API over the libmcpt C ABI.

The product is ``libmcpt.so`` (HIP kernels for gfx950 + C ABI + C++ scene producer,
``../csrc``).  This module is a thin ctypes binding that mirrors the reference's
host interface for the hot path so a user of ``MontecarloGPU/montecarlo.cpp`` finds
the same objects:

* :class:`Scene`     — ``ScenePrimitives`` + ``BVH_GPU_Scene`` (add_*/finalize/depth/
  nb_prim/nb_emissives; bvh_gpu/gpu_bvh_scene.h:35-121) and the 8 reference scenes
  (montecarlo.cpp:629-795);
* :class:`Renderer`  — the GL program + RGB32F accumulation FBO of ``RTViewer``
  (montecarlo.cpp:384-386, 408-477): upload, passes, read-back, average;
* :func:`camera_canonical` — the default camera (camera.cpp:53-95, montecarlo.cpp:405).

There is no CPU fallback: if ``libmcpt.so`` is missing or the GPU is absent, the
calls raise :class:`MCPTError`.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "MCPTError", "lib", "lib_path", "Scene", "Renderer", "camera_canonical",
    "MONTECARLO", "MAT", "MAT_TR", "EVENT_NAMES", "SCENE_KEYS",
    "TRAVERSAL_AUTO", "TRAVERSAL_LANE", "TRAVERSAL_WAVE", "TRAVERSAL_STREAM",
    "Transfo", "average", "write_pfm", "write_png", "material", "light", "Hit", "HIT_DTYPE",
    "Convergence", "DENOISE_K_COLOR", "ERROR_MU_FLOOR", "DENOISE_K_VARIANCE",
    "TemporalRecord", "TEMPORAL_MAX_HISTORY", "TEMPORAL_PLANE_TOL", "mat4_inverse",
    "AdaptiveTemporal", "TEMPORAL_TARGET",
]

MONTECARLO, MAT, MAT_TR = 0, 1, 2
TRAVERSAL_AUTO, TRAVERSAL_LANE, TRAVERSAL_WAVE, TRAVERSAL_STREAM = 0, 1, 2, 3
# launches of one shape AUTO spends on its timing trials before it settles (up to five candidate
# schedules, each timed twice: mcpt_plan.h kTuneRounds; a trial's time is read when the call
# after the next one starts, so the decision comes two calls after the last trial); callers that
# measure run these first
AUTO_TRIALS = 12
EVENT_NAMES = ("node", "leaf", "prim", "cand", "geom", "colmat", "sample", "trav", "mesh", "tri", "mgeom")
# key bindings of montecarlo.cpp:251-290: scene id -> key
SCENE_KEYS = {1: "Q", 2: "W", 3: "E", 4: "R", 5: "T", 6: "Y", 7: "U", 8: "I"}

_HERE = os.path.dirname(os.path.abspath(__file__))


DEBUG_SLOTS = 64   # MCPT_DEBUG_SLOTS
# the denoiser's default edge-stopping widths (chosen by the sweep of DESIGN.md §3.7)
DENOISE_SIGMA_COLOR = 4.0
DENOISE_SIGMA_PLANE = 1.0
# the noise-guided filter's colour width in standard errors of the pixel (the sweep of DESIGN.md §3.8)
DENOISE_K_COLOR = 64.0
# the variance filter's colour width in standard deviations of the pixel's carried variance (the
# sweep of DESIGN.md §3.8: tools/variance_filter_sweep.py)
DENOISE_K_VARIANCE = 16.0
# the relative error's floor on the mean luminance: pixels darker than this are
# measured against it, so that black pixels do not hold a render back
ERROR_MU_FLOOR = 0.01
NO_GUIDES = -7     # MCPT_ERR_NO_GUIDES
NO_STATS = -8      # MCPT_ERR_NO_STATS
NO_ADAPTIVE = -9   # MCPT_ERR_NO_ADAPTIVE
NO_TEMPORAL = -10  # MCPT_ERR_NO_TEMPORAL
# temporal reprojection's defaults (the sweep of DESIGN.md §3.10: tools/temporal_bench.py): the longest
# history a pixel blends, and the tangent-plane distance, relative to the pixel's distance from the
# camera, within which a history tap shows the same surface point
TEMPORAL_MAX_HISTORY = 8
TEMPORAL_PLANE_TOL = 0.01
# temporal adaptive sampling's default target (tools/temporal_adaptive_bench.py): a
# block stops once the relative error of the blend its accumulate would write now is at most this
TEMPORAL_TARGET = 0.05


class MCPTError(RuntimeError):
    pass


class Convergence(ctypes.Structure):
    """mcpt_convergence_t (include/mcpt.h): the frame record of a convergence query."""
    _fields_ = [("n_px", ctypes.c_longlong), ("n_above", ctypes.c_longlong), ("sum_q", ctypes.c_ulonglong),
                ("max_r", ctypes.c_float), ("mean_r", ctypes.c_double), ("passes", ctypes.c_longlong),
                ("batches", ctypes.c_int)]


class Adaptive(ctypes.Structure):
    """mcpt_adaptive_t (include/mcpt.h): the frame record of an adaptive select."""
    _fields_ = Convergence._fields_ + [("n_active_blocks", ctypes.c_longlong), ("n_blocks", ctypes.c_longlong),
                                       ("samples", ctypes.c_longlong)]


class AdaptiveFiltered(ctypes.Structure):
    """mcpt_adaptive_filtered_t (include/mcpt.h): the raw and the filtered frame record of a select on
    the denoised frame's error."""
    _fields_ = [("raw", Adaptive), ("n_above_f", ctypes.c_longlong), ("sum_qf", ctypes.c_ulonglong),
                ("max_rf", ctypes.c_float), ("mean_rf", ctypes.c_double)]


class AdaptiveRun(ctypes.Structure):
    """mcpt_adaptive_run_t (include/mcpt.h): what a queued adaptive run did."""
    _fields_ = [("rounds_queued", ctypes.c_int), ("rounds_run", ctypes.c_int), ("selects_run", ctypes.c_int),
                ("passes_run", ctypes.c_longlong), ("device_ms", ctypes.c_float)]


ADAPTIVE_RUN_MAX_ROUNDS = 256   # MCPT_ADAPTIVE_RUN_MAX_ROUNDS


class TemporalRecord(ctypes.Structure):
    """mcpt_temporal_t (include/mcpt.h): the frame record of a temporal accumulate."""
    _fields_ = [("n_px", ctypes.c_longlong), ("n_history", ctypes.c_longlong), ("n_new", ctypes.c_longlong),
                ("n_miss", ctypes.c_longlong), ("n_offscreen", ctypes.c_longlong), ("n_rejected", ctypes.c_longlong),
                ("sum_len", ctypes.c_longlong), ("max_len", ctypes.c_int), ("frames", ctypes.c_longlong)]


class AdaptiveTemporal(ctypes.Structure):
    """mcpt_adaptive_temporal_t (include/mcpt.h): the raw frame record and the dry-run record of a select
    on the temporal blend's error."""
    _fields_ = [("raw", Adaptive), ("n_px_t", ctypes.c_longlong), ("n_above_t", ctypes.c_longlong),
                ("sum_qt", ctypes.c_ulonglong), ("max_rt", ctypes.c_float), ("mean_rt", ctypes.c_double),
                ("n_history", ctypes.c_longlong)]


class AdaptiveCheckpoint(ctypes.Structure):
    """mcpt_adaptive_checkpoint_t (include/mcpt.h): the header of an adaptive checkpoint file."""
    _fields_ = [("W", ctypes.c_int), ("rows", ctypes.c_int), ("pass_count", ctypes.c_int), ("next_pass", ctypes.c_int),
                ("H", ctypes.c_int), ("rows_hash", ctypes.c_ulonglong), ("p0", ctypes.c_int),
                ("min_passes", ctypes.c_int), ("stats_passes", ctypes.c_longlong), ("stats_batches", ctypes.c_int),
                ("emap_valid", ctypes.c_int), ("n_blocks", ctypes.c_int), ("blocks_x", ctypes.c_int)]


class Refit(ctypes.Structure):
    """mcpt_refit_t (include/mcpt.h): what a mesh refit wrote, its device time and the new root box."""
    _fields_ = [("triangles", ctypes.c_longlong), ("leaves", ctypes.c_longlong), ("internal_nodes", ctypes.c_longlong),
                ("device_ms", ctypes.c_float), ("has_root", ctypes.c_int), ("root_box", ctypes.c_float * 6)]


class Rebuild(ctypes.Structure):
    """mcpt_rebuild_t (include/mcpt.h): what a mesh rebuild sorted, its device times and the new root box."""
    _fields_ = [("triangles", ctypes.c_longlong), ("rounds", ctypes.c_int), ("sort_passes", ctypes.c_int),
                ("sort_ms", ctypes.c_float), ("refit_ms", ctypes.c_float), ("has_root", ctypes.c_int),
                ("root_box", ctypes.c_float * 6)]


class Hit(ctypes.Structure):
    """mcpt_hit (include/mcpt.h): one ray-query result."""
    _fields_ = [("shape", ctypes.c_int), ("prim", ctypes.c_int), ("dir", ctypes.c_int), ("dist", ctypes.c_float),
                ("pl", ctypes.c_float * 3), ("pg", ctypes.c_float * 3), ("N", ctypes.c_float * 3),
                ("P", ctypes.c_float * 3), ("color", ctypes.c_float * 4), ("material", ctypes.c_float * 4)]


HIT_DTYPE = np.dtype([("shape", "<i4"), ("prim", "<i4"), ("dir", "<i4"), ("dist", "<f4"), ("pl", "<f4", 3),
                      ("pg", "<f4", 3), ("N", "<f4", 3), ("P", "<f4", 3), ("color", "<f4", 4),
                      ("material", "<f4", 4)])


def lib_path() -> str:
    return os.environ.get("MCPT_LIB", os.path.join(_HERE, "libmcpt.so"))


_lib: Optional[ctypes.CDLL] = None
_c_float_p = ctypes.POINTER(ctypes.c_float)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_u64_p = ctypes.POINTER(ctypes.c_ulonglong)
_vp = ctypes.c_void_p


def _declare(L: ctypes.CDLL) -> None:
    i, f, fp, ip = ctypes.c_int, ctypes.c_float, _c_float_p, _c_int_p
    sig = {
        "mcpt_error_string": (ctypes.c_char_p, [i]),
        "mcpt_version": (i, []),
        "mcpt_build_flags": (i, []),
        "mcpt_create": (i, [i, ctypes.POINTER(_vp)]),
        "mcpt_destroy": (i, [_vp]),
        "mcpt_upload_scene": (i, [_vp, fp, i, fp, ip, i, i]),
        "mcpt_set_target": (i, [_vp, i, i, i, i, i]),
        "mcpt_local_rows": (i, [_vp, ip]),
        "mcpt_set_target_rows": (i, [_vp, i, i, ip, i]),
        "mcpt_balanced_rows": (i, [i, i, i, i, ip, ip]),
        "mcpt_local_row_ids": (i, [_vp, ip]),
        "mcpt_render": (i, [_vp, fp, fp, i, i, f, i, f, i]),
        "mcpt_render_counted": (i, [_vp, fp, fp, i, i, f, i, f, i, _c_u64_p]),
        "mcpt_event_bytes": (i, [i]),
        "mcpt_debug_counters": (i, [_vp, _c_u64_p, i, i]),
        "mcpt_read_accum": (i, [_vp, fp, ip]),
        "mcpt_clear_accum": (i, [_vp]),
        "mcpt_accum_device_ptr": (i, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t)]),
        "mcpt_copy_accum_device": (i, [_vp, _vp, ctypes.c_size_t]),
        "mcpt_gather_rows": (i, [_vp, ctypes.POINTER(_vp), i]),
        "mcpt_set_traversal": (i, [_vp, i]),
        "mcpt_trace": (i, [_vp, fp, fp, i, i, i, _vp]),
        "mcpt_sample_hemisphere": (i, [_vp, fp, fp, f, i, i, fp]),
        "mcpt_get_traversal": (i, [_vp, ip]),
        "mcpt_get_schedule": (i, [_vp, ip, ip, ip]),
        "mcpt_set_walk_exit": (i, [_vp, i]),
        "mcpt_get_walk_exit": (i, [_vp, ip]),
        "mcpt_set_leaf_batch": (i, [_vp, i]),
        "mcpt_get_leaf_batch": (i, [_vp, ip]),
        "mcpt_set_partial_budget": (i, [_vp, ctypes.c_size_t]),
        "mcpt_set_render_lanes": (i, [_vp, i]),
        "mcpt_set_stream_pool": (i, [_vp, i, i]),
        "mcpt_stream_iterations": (i, [_vp, ctypes.POINTER(ctypes.c_longlong)]),
        "mcpt_last_launch_count": (i, [_vp, ip]),
        "mcpt_last_pass_split": (i, [_vp, ip]),
        "mcpt_set_stream": (i, [_vp, _vp]),
        "mcpt_synchronize": (i, [_vp]),
        "mcpt_last_render_ms": (i, [_vp, fp]),
        "mcpt_last_kernel_ms": (i, [_vp, fp, fp]),
        "mcpt_kernel_ms_back": (i, [_vp, ctypes.c_int, fp, fp]),
        "mcpt_kernel_span_ms_back": (i, [_vp, ctypes.c_int, fp]),
        "mcpt_scene_create": (i, [ctypes.POINTER(_vp)]),
        "mcpt_scene_destroy": (i, [_vp]),
        "mcpt_scene_clear": (i, [_vp]),
        "mcpt_scene_add_sphere": (i, [_vp, fp, fp]),
        "mcpt_scene_add_cube": (i, [_vp, fp, fp]),
        "mcpt_scene_add_cylinder": (i, [_vp, fp, fp]),
        "mcpt_scene_add_cone": (i, [_vp, fp, fp]),
        "mcpt_scene_add_oriented_quad": (i, [_vp, fp, fp]),
        "mcpt_scene_finalize": (i, [_vp]),
        "mcpt_scene_add_mesh": (i, [_vp, fp, fp, i, ctypes.POINTER(ctypes.c_uint), i, fp, ip]),
        "mcpt_scene_place_mesh": (i, [_vp, i, fp, fp]),
        "mcpt_scene_mesh_sizes": (i, [_vp, ip, ip, ip, ip, ip]),
        "mcpt_scene_get_mesh_buffers": (i, [_vp, ip, fp, ip, ip, fp, fp]),
        "mcpt_upload_meshes": (i, [_vp, i, ip, i, fp, i, ip, i, ip, i, fp, fp]),
        "mcpt_scene_update_mesh": (i, [_vp, i, fp, fp, i]),
        "mcpt_scene_mesh_vertex_range": (i, [_vp, i, ip, ip]),
        "mcpt_update_mesh_vertices": (i, [_vp, i, i, fp, fp]),
        "mcpt_update_mesh_vertices_device": (i, [_vp, i, i, _vp, _vp]),
        "mcpt_refit_mesh": (i, [_vp, i, ctypes.POINTER(Refit)]),
        "mcpt_scene_rebuild_mesh": (i, [_vp, i, ctypes.POINTER(ctypes.c_uint), i]),
        "mcpt_rebuild_mesh": (i, [_vp, i, ip, i, ctypes.POINTER(Rebuild)]),
        "mcpt_set_mesh_vertex_counts": (i, [_vp, i, ip]),
        "mcpt_debug_mesh_record_sizes": (i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
        "mcpt_debug_mesh_records": (i, [_vp, fp, ctypes.c_size_t, fp, ctypes.c_size_t]),
        "mcpt_set_flat_face": (i, [_vp, i]),
        "mcpt_scene_nb_prim": (i, [_vp, ip]),
        "mcpt_scene_depth": (i, [_vp, ip]),
        "mcpt_scene_nb_emissives": (i, [_vp, ip]),
        "mcpt_scene_get_buffers": (i, [_vp, fp, fp, ip]),
        "mcpt_scene_set_material": (i, [_vp, i, fp]),
        "mcpt_scene_build_reference": (i, [_vp, i, f]),
        "mcpt_camera_canonical": (i, [i, i, fp, fp]),
        "mcpt_transfo_translate": (i, [f, f, f, fp]),
        "mcpt_transfo_scale": (i, [f, f, f, fp]),
        "mcpt_transfo_rotate": (i, [i, f, fp]),
        "mcpt_mat4_mul": (i, [fp, fp, fp]),
        "mcpt_average": (i, [fp, ctypes.c_longlong, i, fp]),
        "mcpt_write_pfm": (i, [ctypes.c_char_p, fp, i, i]),
        "mcpt_write_png": (i, [ctypes.c_char_p, fp, i, i]),
        "mcpt_write_accum": (i, [_vp, fp, i]),
        "mcpt_checkpoint_write": (i, [ctypes.c_char_p, fp, i, i, i, i, ctypes.c_char_p]),
        "mcpt_checkpoint_save": (i, [_vp, ctypes.c_char_p, i, ctypes.c_char_p]),
        "mcpt_checkpoint_load": (i, [_vp, ctypes.c_char_p, ctypes.c_char_p, ip]),
        "mcpt_checkpoint_read": (i, [ctypes.c_char_p, fp, ctypes.c_longlong, ip, ip, ip, ip, ctypes.c_char_p]),
        "mcpt_render_guides": (i, [_vp, fp, fp]),
        "mcpt_read_guides": (i, [_vp, fp, fp]),
        "mcpt_denoise": (i, [_vp, i, f, f]),
        "mcpt_read_denoised": (i, [_vp, fp]),
        "mcpt_last_denoise_ms": (i, [_vp, fp, fp]),
        "mcpt_denoise_iteration_ms": (i, [_vp, i, fp]),
        "mcpt_last_denoise_path": (i, [_vp, ip]),
        "mcpt_stats_begin": (i, [_vp]),
        "mcpt_stats_end": (i, [_vp]),
        "mcpt_stats_add_batch": (i, [_vp, i]),
        "mcpt_stats_info": (i, [_vp, ip, ctypes.POINTER(ctypes.c_longlong), ip]),
        "mcpt_convergence": (i, [_vp, f, f, ctypes.POINTER(Convergence)]),
        "mcpt_read_error_map": (i, [_vp, fp]),
        "mcpt_denoise_guided": (i, [_vp, i, f, f]),
        "mcpt_last_stats_ms": (i, [_vp, fp, fp]),
        "mcpt_adaptive_begin": (i, [_vp, i]),
        "mcpt_adaptive_end": (i, [_vp]),
        "mcpt_adaptive_select": (i, [_vp, f, f, ctypes.POINTER(Adaptive)]),
        "mcpt_adaptive_select_filtered": (i, [_vp, f, f, f, i, f, f, ctypes.POINTER(AdaptiveFiltered)]),
        "mcpt_adaptive_run": (i, [_vp, fp, fp, i, i, i, i, f, f, f, i, f, i, ctypes.POINTER(Adaptive), i,
                                  ctypes.POINTER(AdaptiveRun)]),
        "mcpt_adaptive_run_filtered": (i, [_vp, fp, fp, i, i, i, i, f, f, f, i, f, f, f, i, f, i,
                                           ctypes.POINTER(AdaptiveFiltered), i, ctypes.POINTER(AdaptiveRun)]),
        "mcpt_adaptive_until_next": (i, [i, i, i, i, i, i, ip, ip, ip]),
        "mcpt_read_active_blocks": (i, [_vp, ip, i, ip]),
        "mcpt_render_adaptive": (i, [_vp, fp, fp, i, i, f, i, f, i]),
        "mcpt_read_sample_counts": (i, [_vp, ip]),
        "mcpt_read_resolved": (i, [_vp, fp]),
        "mcpt_adaptive_info": (i, [_vp, ip, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),
        "mcpt_last_adaptive_ms": (i, [_vp, fp, fp]),
        "mcpt_denoise_resolved": (i, [_vp, i, f, f]),
        "mcpt_denoise_resolved_guided": (i, [_vp, i, f, f]),
        "mcpt_denoise_variance": (i, [_vp, i, f, f]),
        "mcpt_denoise_resolved_variance": (i, [_vp, i, f, f]),
        "mcpt_read_denoised_variance": (i, [_vp, fp]),
        "mcpt_temporal_begin": (i, [_vp]),
        "mcpt_temporal_end": (i, [_vp]),
        "mcpt_temporal_accumulate": (i, [_vp, fp, i, f, ctypes.POINTER(TemporalRecord)]),
        "mcpt_temporal_accumulate_resolved": (i, [_vp, fp, i, f, ctypes.POINTER(TemporalRecord)]),
        "mcpt_adaptive_select_temporal": (i, [_vp, fp, i, f, f, f, ctypes.POINTER(AdaptiveTemporal)]),
        "mcpt_adaptive_run_temporal": (i, [_vp, fp, fp, i, i, i, i, f, f, fp, i, f, f, i, f, i,
                                           ctypes.POINTER(AdaptiveTemporal), i, ctypes.POINTER(AdaptiveRun)]),
        "mcpt_denoise_temporal": (i, [_vp, i, f, f]),
        "mcpt_read_temporal": (i, [_vp, fp, ip]),
        "mcpt_temporal_info": (i, [_vp, ip, ip, ctypes.POINTER(ctypes.c_longlong)]),
        "mcpt_last_temporal_ms": (i, [_vp, fp, fp]),
        "mcpt_mat4_inverse": (i, [fp, fp]),
        "mcpt_gather_rows_counted": (i, [_vp, ctypes.POINTER(_vp), i]),
        "mcpt_pass_count": (i, [_vp, ip]),
        "mcpt_pack_counted_device": (i, [_vp, _vp, ctypes.c_size_t]),
        "mcpt_load_rows_counted": (i, [_vp, _vp, ctypes.c_longlong, ip, i]),
        "mcpt_gather_error_map": (i, [_vp, ctypes.POINTER(_vp), i]),
        "mcpt_pack_error_map_device": (i, [_vp, _vp, ctypes.c_size_t]),
        "mcpt_load_rows_error_map": (i, [_vp, _vp, ctypes.c_longlong, ip]),
        "mcpt_error_map_record": (i, [_vp, f, ctypes.POINTER(Convergence)]),
        "mcpt_error_map_source": (i, [_vp, ip]),
        "mcpt_adaptive_checkpoint_save": (i, [_vp, ctypes.c_char_p, i, ctypes.c_char_p]),
        "mcpt_adaptive_checkpoint_load": (i, [_vp, ctypes.c_char_p, ctypes.c_char_p, ip]),
        "mcpt_adaptive_checkpoint_write": (i, [ctypes.c_char_p, ctypes.POINTER(AdaptiveCheckpoint), ctypes.c_char_p, ip,
                                               ip, fp, fp, fp]),
        "mcpt_adaptive_checkpoint_read": (i, [ctypes.c_char_p, ctypes.POINTER(AdaptiveCheckpoint), ctypes.c_char_p, ip,
                                              ip, ctypes.c_longlong, fp, fp, fp, ctypes.c_longlong]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args


def lib() -> ctypes.CDLL:
    """Load libmcpt.so (fails loudly: there is no fallback implementation)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise MCPTError(f"libmcpt.so not found at {path}: build it with "
                            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
                            "montecarlo-pathtracing_amd/csrc`")
        L = ctypes.CDLL(path)
        _declare(L)
        _lib = L
    return _lib


BUILD_CHECKED, BUILD_STAMPS, BUILD_LANESTATS, BUILD_BLOCKTIMES, BUILD_DRIVER_MATH = 1, 2, 4, 8, 16


def build_flags() -> int:
    """mcpt_build_flags: which diagnostic build the loaded library is (0: the shipped build)."""
    return int(lib().mcpt_build_flags())


def _check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().mcpt_error_string(status).decode()
        raise MCPTError(f"{what} failed ({status}): {msg}")


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_c_float_p)


def _ip(a: np.ndarray):
    return a.ctypes.data_as(_c_int_p)


def _f32(a, n: int) -> np.ndarray:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if arr.size != n:
        raise ValueError(f"expected {n} floats, got {arr.size}")
    return arr


def material(rgba: Sequence[float], shininess: float = 0.0, roughness: float = 0.0,
             emissivity: float = 0.0) -> np.ndarray:
    """Material (bvh_gpu/scene.h:30-49) packed as the 7 floats the C ABI takes."""
    return np.array(list(rgba) + [shininess, roughness, emissivity], dtype=np.float32)


def light(rgba: Sequence[float], emissivity: float) -> np.ndarray:
    """Material::light (scene.h:48)."""
    return material(rgba, 0.0, 0.0, emissivity)


class Scene:
    """ScenePrimitives + BVH_GPU_Scene (host side, C++ in libmcpt)."""

    def __init__(self) -> None:
        h = _vp()
        _check(lib().mcpt_scene_create(ctypes.byref(h)), "mcpt_scene_create")
        self._h = h

    def __del__(self) -> None:
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.mcpt_scene_destroy(h)
            self._h = None

    @classmethod
    def reference(cls, scene_id: int, light_intensity: float = 1.2) -> "Scene":
        """Build one of the 8 scenes of montecarlo.cpp (keys Q..I → 1..8), finalized."""
        s = cls()
        _check(lib().mcpt_scene_build_reference(s._h, int(scene_id), float(light_intensity)),
               f"mcpt_scene_build_reference({scene_id})")
        return s

    def clear(self) -> None:
        _check(lib().mcpt_scene_clear(self._h), "mcpt_scene_clear")

    def _add(self, fn: str, trf, mat) -> None:
        t = _f32(trf, 16)
        m = _f32(mat, 7)
        _check(getattr(lib(), fn)(self._h, _fp(t), _fp(m)), fn)

    # transforms are 4x4 column-major (GL / Eigen storage); a (4,4) numpy array in
    # row-major math convention is accepted and transposed to column-major storage.
    @staticmethod
    def _colmajor(trf) -> np.ndarray:
        a = np.asarray(trf, dtype=np.float32)
        return a.T.reshape(-1) if a.shape == (4, 4) else a.reshape(-1)

    def add_sphere(self, trf, mat) -> None:
        self._add("mcpt_scene_add_sphere", self._colmajor(trf), mat)

    def add_cube(self, trf, mat) -> None:
        self._add("mcpt_scene_add_cube", self._colmajor(trf), mat)

    def add_cylinder(self, trf, mat) -> None:
        self._add("mcpt_scene_add_cylinder", self._colmajor(trf), mat)

    def add_cone(self, trf, mat) -> None:
        self._add("mcpt_scene_add_cone", self._colmajor(trf), mat)

    def add_oriented_quad(self, trf, mat) -> None:
        self._add("mcpt_scene_add_oriented_quad", self._colmajor(trf), mat)

    add_orientedQuad = add_oriented_quad   # reference spelling (gpu_bvh_scene.h:103)

    def add_mesh(self, vertices, normals, tri_indices, bb=None) -> int:
        """BVH_GPU_Scene::add_mesh: store a mesh (positions, normals, triangle vertex indices)
        and build its BVH; bb = (min.xyz, max.xyz) of Mesh::BB(), default the vertices' box.
        Returns the mesh id for place_mesh."""
        v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
        n = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tri_indices, np.uint32).reshape(-1, 3))
        if n.shape != v.shape:
            raise ValueError("one normal per vertex")
        b = None if bb is None else _f32(bb, 6)
        mid = ctypes.c_int()
        _check(lib().mcpt_scene_add_mesh(self._h, _fp(v), _fp(n), v.shape[0],
                                         t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), t.shape[0],
                                         _fp(b) if b is not None else None, ctypes.byref(mid)), "mcpt_scene_add_mesh")
        return mid.value

    def place_mesh(self, mesh_id: int, trf, mat) -> None:
        """BVH_GPU_Scene::place_mesh: an instance of mesh `mesh_id` (a CODE_MESH primitive)."""
        t = _f32(self._colmajor(trf), 16)
        m = _f32(mat, 7)
        _check(lib().mcpt_scene_place_mesh(self._h, int(mesh_id), _fp(t), _fp(m)), "mcpt_scene_place_mesh")

    def update_mesh(self, mesh_id: int, vertices, normals) -> None:
        """mcpt_scene_update_mesh: new vertices and normals for mesh `mesh_id` (same triangles, depth and
        leaves) and its BVH boxes refitted; every vertex inside the bb the mesh was added with."""
        v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
        n = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        if n.shape != v.shape:
            raise ValueError("one normal per vertex")
        _check(lib().mcpt_scene_update_mesh(self._h, int(mesh_id), _fp(v), _fp(n), v.shape[0]), "mcpt_scene_update_mesh")

    def rebuild_mesh(self, mesh_id: int, tris=None) -> None:
        """mcpt_scene_rebuild_mesh: mesh `mesh_id`'s tree rebuilt from its current vertices by stable median
        splits (same depth and buffer sizes); tris (n x 3 mesh-local vertex indices, the mesh's count)
        replaces its triangles first."""
        if tris is None:
            _check(lib().mcpt_scene_rebuild_mesh(self._h, int(mesh_id), None, 0), "mcpt_scene_rebuild_mesh")
            return
        t = np.ascontiguousarray(np.asarray(tris, np.uint32).reshape(-1, 3))
        _check(lib().mcpt_scene_rebuild_mesh(self._h, int(mesh_id), t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                             t.shape[0]), "mcpt_scene_rebuild_mesh")

    def mesh_vertex_range(self, mesh_id: int) -> Tuple[int, int]:
        """(first vertex, vertex count) of mesh `mesh_id` in mesh_buffers()'s verts / normals."""
        first, n = ctypes.c_int(), ctypes.c_int()
        _check(lib().mcpt_scene_mesh_vertex_range(self._h, int(mesh_id), ctypes.byref(first), ctypes.byref(n)),
               "mcpt_scene_mesh_vertex_range")
        return first.value, n.value

    def mesh_buffers(self):
        """dict of the flat mesh buffers (mcpt_scene_get_mesh_buffers layouts), or None."""
        sz = [ctypes.c_int() for _ in range(5)]
        _check(lib().mcpt_scene_mesh_sizes(self._h, *[ctypes.byref(x) for x in sz]), "mcpt_scene_mesh_sizes")
        nm, nn, nl, nt, nv = (x.value for x in sz)
        if nm == 0:
            return None
        b = {"info": np.zeros((nm, 4), np.int32), "nodes": np.zeros((nn, 6), np.float32),
             "leaves": np.zeros(nl, np.int32), "tris": np.zeros((nt, 3), np.int32),
             "verts": np.zeros((nv, 3), np.float32), "normals": np.zeros((nv, 3), np.float32)}
        _check(lib().mcpt_scene_get_mesh_buffers(self._h, _ip(b["info"]), _fp(b["nodes"]), _ip(b["leaves"]),
                                                 _ip(b["tris"]), _fp(b["verts"]), _fp(b["normals"])),
               "mcpt_scene_get_mesh_buffers")
        return b

    def finalize(self) -> None:
        _check(lib().mcpt_scene_finalize(self._h), "mcpt_scene_finalize")

    def nb_prim(self) -> int:
        n = ctypes.c_int()
        _check(lib().mcpt_scene_nb_prim(self._h, ctypes.byref(n)), "mcpt_scene_nb_prim")
        return n.value

    def depth(self, i: int = 0) -> int:
        d = ctypes.c_int()
        _check(lib().mcpt_scene_depth(self._h, ctypes.byref(d)), "mcpt_scene_depth")
        return d.value

    def nb_emissives(self) -> int:
        n = ctypes.c_int()
        _check(lib().mcpt_scene_nb_emissives(self._h, ctypes.byref(n)), "mcpt_scene_nb_emissives")
        return n.value

    def buffers(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(prims n×64 f32, nodes (2^(d+1)-1)×6 f32, leaves 2^d i32) — texture layouts."""
        n, d = self.nb_prim(), self.depth()
        prims = np.zeros((n, 64), np.float32)
        nodes = np.zeros((2 ** (d + 1) - 1, 6), np.float32)
        leaves = np.zeros(2 ** d, np.int32)
        _check(lib().mcpt_scene_get_buffers(self._h, _fp(prims), _fp(nodes), _ip(leaves)),
               "mcpt_scene_get_buffers")
        return prims, nodes, leaves

    def set_material(self, prim: int, mat) -> None:
        m = _f32(mat, 7)
        _check(lib().mcpt_scene_set_material(self._h, int(prim), _fp(m)), "mcpt_scene_set_material")


def camera_canonical(W: int, H: int) -> Tuple[np.ndarray, np.ndarray]:
    """(invPV, invV) of the default camera at aspect W/H, 16 f32 column-major each."""
    ipv = np.zeros(16, np.float32)
    iv = np.zeros(16, np.float32)
    _check(lib().mcpt_camera_canonical(int(W), int(H), _fp(ipv), _fp(iv)), "mcpt_camera_canonical")
    return ipv, iv


# ---- Transfo (easycppogl/gl_eigen.cpp:29-105) and GLMat4 product, computed by libmcpt
def _m16(fn, *args) -> np.ndarray:
    out = np.zeros(16, np.float32)
    _check(getattr(lib(), fn)(*args, _fp(out)), fn)
    return out


class Transfo:
    """Reference Transfo: 4x4 column-major float matrices (16 floats), angles in degrees."""

    @staticmethod
    def translate(x, y, z) -> np.ndarray:
        return _m16("mcpt_transfo_translate", float(x), float(y), float(z))

    @staticmethod
    def scale(sx, sy=None, sz=None) -> np.ndarray:
        sy = sx if sy is None else sy
        sz = sx if sz is None else sz
        return _m16("mcpt_transfo_scale", float(sx), float(sy), float(sz))

    @staticmethod
    def rotateX(deg) -> np.ndarray:
        return _m16("mcpt_transfo_rotate", 0, float(deg))

    @staticmethod
    def rotateY(deg) -> np.ndarray:
        return _m16("mcpt_transfo_rotate", 1, float(deg))

    @staticmethod
    def rotateZ(deg) -> np.ndarray:
        return _m16("mcpt_transfo_rotate", 2, float(deg))

    @staticmethod
    def mul(*ms) -> np.ndarray:
        """Product a * b * ... in the reference's float arithmetic (left to right)."""
        acc = _f32(ms[0], 16)
        for m in ms[1:]:
            b = _f32(m, 16)
            out = np.zeros(16, np.float32)
            _check(lib().mcpt_mat4_mul(_fp(acc), _fp(b), _fp(out)), "mcpt_mat4_mul")
            acc = out
        return acc


def mat4_inverse(m) -> np.ndarray:
    """mcpt_mat4_inverse: the inverse of 16 f32 (computed in double, rounded once); MCPTError for a
    singular matrix.  mat4_inverse(invPV) is the P·V Renderer.temporal_accumulate takes."""
    a = _f32(m, 16)
    out = np.zeros(16, np.float32)
    _check(lib().mcpt_mat4_inverse(_fp(a), _fp(out)), "mcpt_mat4_inverse")
    return out


# ---- output step
def average(accum: np.ndarray, pass_count: int) -> np.ndarray:
    """fs_frag: accum / nb (montecarlo.cpp:59-70), binary32 per channel."""
    a = np.ascontiguousarray(accum, np.float32)
    out = np.empty_like(a)
    _check(lib().mcpt_average(_fp(a), a.size, int(pass_count), _fp(out)), "mcpt_average")
    return out


def write_pfm(path: str, rgb: np.ndarray) -> None:
    a = np.ascontiguousarray(rgb, np.float32)
    _check(lib().mcpt_write_pfm(str(path).encode(), _fp(a), a.shape[1], a.shape[0]), "mcpt_write_pfm")


def write_png(path: str, rgb: np.ndarray) -> None:
    """8-bit framebuffer view: clamp [0,1], round(255·c), no gamma (GL unorm conversion)."""
    a = np.ascontiguousarray(rgb, np.float32)
    _check(lib().mcpt_write_png(str(path).encode(), _fp(a), a.shape[1], a.shape[0]), "mcpt_write_png")


# ---- checkpoint / resume of a progressive render (mcpt.h: mcpt_checkpoint_write / _read)
CHECKPOINT_TAG_MAX = 1024


def checkpoint_write(path: str, accum: np.ndarray, pass_count: int, next_pass: int, tag: str = "") -> None:
    """accum: rows × W × 3 f32 sums holding `pass_count` passes; `next_pass` = the first pass
    of the render call that continues; `tag` = the render parameters the reader compares."""
    a = np.ascontiguousarray(accum, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise MCPTError("checkpoint_write: accum must be rows x W x 3")
    _check(lib().mcpt_checkpoint_write(str(path).encode(), _fp(a), a.shape[1], a.shape[0], int(pass_count),
                                       int(next_pass), tag.encode()), "mcpt_checkpoint_write")


def checkpoint_read(path: str) -> Tuple[np.ndarray, int, int, str]:
    """(accum rows × W × 3, pass_count, next_pass, tag) of a checkpoint file."""
    w, rows, pc, nxt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tag = ctypes.create_string_buffer(CHECKPOINT_TAG_MAX)
    _check(lib().mcpt_checkpoint_read(str(path).encode(), None, 0, ctypes.byref(w), ctypes.byref(rows), None, None,
                                      None), "mcpt_checkpoint_read")
    out = np.empty((rows.value, w.value, 3), np.float32)
    # the capacity bounds the read if the file was replaced in between; the shape is re-read
    _check(lib().mcpt_checkpoint_read(str(path).encode(), _fp(out), out.size, ctypes.byref(w), ctypes.byref(rows),
                                      ctypes.byref(pc), ctypes.byref(nxt), tag), "mcpt_checkpoint_read")
    if (rows.value, w.value, 3) != out.shape:
        raise MCPTError("checkpoint_read: the file changed while it was read")
    return out, pc.value, nxt.value, tag.value.decode()


# ---- checkpoint / resume of an adaptive render (mcpt.h: mcpt_adaptive_checkpoint_write / _read)
_ADAPTIVE_HEADER_KEYS = ("pass_count", "next_pass", "H", "rows_hash", "p0", "min_passes", "stats_passes",
                         "stats_batches", "emap_valid")


def adaptive_checkpoint_write(path: str, header: dict, block_active, block_passes, accum, stats, emap,
                              tag: str = "") -> None:
    """An "MCPTCKA1" file from plain arrays: accum rows x W x 3, stats rows x W x 4 ({Yacc, S2, Ybase, 0}),
    emap rows x W x 2 ({se, r}), all f32; block_active / block_passes one int32 per 8x8 block of the
    rows x W grid; header = {pass_count, next_pass, H, rows_hash, p0, min_passes, stats_passes,
    stats_batches, emap_valid} (missing keys: 0)."""
    a = np.ascontiguousarray(accum, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise MCPTError("adaptive_checkpoint_write: accum must be rows x W x 3")
    rows, w = a.shape[0], a.shape[1]
    st = np.ascontiguousarray(stats, np.float32)
    em = np.ascontiguousarray(emap, np.float32)
    act = np.ascontiguousarray(block_active, np.int32).reshape(-1)
    pas = np.ascontiguousarray(block_passes, np.int32).reshape(-1)
    bx, by = (w + 7) // 8, (rows + 7) // 8
    if st.shape != (rows, w, 4) or em.shape != (rows, w, 2) or act.size != bx * by or pas.size != bx * by:
        raise MCPTError("adaptive_checkpoint_write: the arrays' shapes do not belong to one rows x W target")
    h = AdaptiveCheckpoint(W=w, rows=rows, n_blocks=bx * by, blocks_x=bx)
    for k in _ADAPTIVE_HEADER_KEYS:
        setattr(h, k, int(header.get(k, 0)))
    _check(lib().mcpt_adaptive_checkpoint_write(str(path).encode(), ctypes.byref(h), tag.encode(), _ip(act), _ip(pas),
                                                _fp(a), _fp(st), _fp(em)), "mcpt_adaptive_checkpoint_write")


def adaptive_checkpoint_read(path: str) -> dict:
    """The header fields of an "MCPTCKA1" file (W, rows, n_blocks, blocks_x and
    adaptive_checkpoint_write's header keys), "tag", and the arrays "block_active", "block_passes",
    "accum", "stats", "emap" in adaptive_checkpoint_write's shapes."""
    h = AdaptiveCheckpoint()
    tag = ctypes.create_string_buffer(CHECKPOINT_TAG_MAX)
    _check(lib().mcpt_adaptive_checkpoint_read(str(path).encode(), ctypes.byref(h), None, None, None, 0, None, None,
                                               None, 0), "mcpt_adaptive_checkpoint_read")
    rows, w, nb = h.rows, h.W, h.n_blocks
    act, pas = np.empty(nb, np.int32), np.empty(nb, np.int32)
    acc, st, em = (np.empty((rows, w, k), np.float32) for k in (3, 4, 2))
    # the capacities bound the read if the file was replaced in between; the shape is re-read
    _check(lib().mcpt_adaptive_checkpoint_read(str(path).encode(), ctypes.byref(h), tag, _ip(act), _ip(pas), nb,
                                               _fp(acc), _fp(st), _fp(em), rows * w), "mcpt_adaptive_checkpoint_read")
    if (h.rows, h.W, h.n_blocks) != (rows, w, nb):
        raise MCPTError("adaptive_checkpoint_read: the file changed while it was read")
    out = {k: getattr(h, k) for k, _ in AdaptiveCheckpoint._fields_}
    out.update(tag=tag.value.decode(), block_active=act, block_passes=pas, accum=acc, stats=st, emap=em)
    return out


def _adaptive_until(render, select, run, first_pass: int, batch: int, max_passes: int, check_every: int = 1,
                    queued_rounds: int = 0, done: int = 0, calls: int = 0) -> Tuple[dict, int, int]:
    """The loop behind every render_adaptive_until: each step is what mcpt_adaptive_until_next (mcpt.h)
    says follows `done` passes in `calls` render calls, issued as render(first, n), select() -> record
    or run(first, rounds) -> adaptive_run()'s dict (None: never queued).  Ends at the cap, on a record
    with no active block or on a run that stopped short; if no select has run, one is made at the end
    (fewer than two batches: MCPT_ERR_NO_STATS).  Returns (the last record, done, calls)."""
    r, n, sel, rec = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), None
    while rec is None or rec["n_active_blocks"] > 0:
        _check(lib().mcpt_adaptive_until_next(done, calls, batch, max_passes, check_every, queued_rounds if run else 0,
                                              ctypes.byref(r), ctypes.byref(n), ctypes.byref(sel)),
               "mcpt_adaptive_until_next")
        if r.value > 0:
            got = run(first_pass + done, r.value)
            done, calls = done + got["rounds_run"] * batch, calls + got["rounds_run"]
            if got["records"]:
                rec = got["records"][-1]
            if got["rounds_run"] < r.value:
                break
        elif n.value > 0:
            render(first_pass + done, n.value)
            done, calls = done + n.value, calls + 1
            if sel.value:
                rec = select()
        else:
            break
    return (select() if rec is None else rec), done, calls


class Renderer:
    """Device context: scene on the GPU, row-band framebuffer, pass accumulation."""

    def __init__(self, device: int = 0) -> None:
        h = _vp()
        _check(lib().mcpt_create(int(device), ctypes.byref(h)), "mcpt_create")
        self._h = h
        self.W = self.H = 0
        self.band_rows, self.world, self.rank = 1, 1, 0
        self.n_local_rows = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().mcpt_destroy(self._h)
            self._h = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene: Optional[Scene] = None, prims=None, nodes=None, leaves=None,
                     depth: Optional[int] = None, nb_emissives: int = 0) -> None:
        if scene is not None:
            prims, nodes, leaves = scene.buffers()
            depth = scene.depth()
            nb_emissives = scene.nb_emissives()
        prims = np.ascontiguousarray(prims, dtype=np.float32)
        nodes = np.ascontiguousarray(nodes, dtype=np.float32)
        leaves = np.ascontiguousarray(leaves, dtype=np.int32)
        n = prims.size // 64
        _check(lib().mcpt_upload_scene(self._h, _fp(prims), int(n), _fp(nodes), _ip(leaves),
                                       int(depth), int(nb_emissives)), "mcpt_upload_scene")
        if scene is not None:
            mb = scene.mesh_buffers()
            if mb is not None:
                self.upload_meshes(mb)
                # (where each mesh's vertices lie: rebuild_mesh with new triangles)
                counts = np.array([scene.mesh_vertex_range(m)[1] for m in range(len(mb["info"]))], np.int32)
                _check(lib().mcpt_set_mesh_vertex_counts(self._h, len(counts), _ip(counts)), "mcpt_set_mesh_vertex_counts")

    def upload_meshes(self, mb) -> None:
        """mcpt_upload_meshes from a Scene.mesh_buffers() dict (None/empty: no meshes)."""
        if not mb:
            _check(lib().mcpt_upload_meshes(self._h, 0, None, 0, None, 0, None, 0, None, 0, None, None),
                   "mcpt_upload_meshes")
            return
        info = np.ascontiguousarray(mb["info"], np.int32)
        nodes = np.ascontiguousarray(mb["nodes"], np.float32)
        leaves = np.ascontiguousarray(mb["leaves"], np.int32)
        tris = np.ascontiguousarray(mb["tris"], np.int32)
        verts = np.ascontiguousarray(mb["verts"], np.float32)
        norms = np.ascontiguousarray(mb["normals"], np.float32)
        _check(lib().mcpt_upload_meshes(self._h, info.shape[0], _ip(info), nodes.shape[0], _fp(nodes), leaves.size,
                                        _ip(leaves), tris.shape[0], _ip(tris), verts.shape[0], _fp(verts),
                                        _fp(norms)), "mcpt_upload_meshes")

    def update_mesh_vertices(self, first: int, verts, normals) -> None:
        """New positions and normals (n x 3 f32 each) over the uploaded vertices first .. first + n
        (Scene.mesh_vertex_range): numpy arrays (mcpt_update_mesh_vertices), or two torch tensors on
        this renderer's device (mcpt_update_mesh_vertices_device; the torch stream that wrote them is
        waited for here).  Follow it with refit_mesh."""
        if hasattr(verts, "data_ptr") and hasattr(normals, "data_ptr"):
            import torch
            if not (verts.is_cuda and normals.is_cuda) or verts.dtype != torch.float32 or normals.dtype != torch.float32:
                raise ValueError("update_mesh_vertices: float32 tensors on the device, or numpy arrays")
            v, n = verts.reshape(-1, 3).contiguous(), normals.reshape(-1, 3).contiguous()
            if n.shape != v.shape:
                raise ValueError("one normal per vertex")
            torch.cuda.current_stream(v.device).synchronize()
            self._vertex_src = (v, n)   # (kept until the next update: the queued kernel still reads them)
            _check(lib().mcpt_update_mesh_vertices_device(self._h, int(first), v.shape[0], _vp(v.data_ptr()),
                                                          _vp(n.data_ptr())), "mcpt_update_mesh_vertices_device")
            return
        v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
        n = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        if n.shape != v.shape:
            raise ValueError("one normal per vertex")
        _check(lib().mcpt_update_mesh_vertices(self._h, int(first), v.shape[0], _fp(v), _fp(n)),
               "mcpt_update_mesh_vertices")

    def refit_mesh(self, mesh_id: int = -1, record: bool = True) -> Optional[dict]:
        """mcpt_refit_mesh: the BVH records of mesh `mesh_id` (-1: every mesh) rewritten on the device from
        the current vertices.  record=True waits and returns {triangles, leaves, internal_nodes,
        device_ms, root_box (a single mesh of depth >= 1, else None)}; record=False queues it only."""
        if not record:
            _check(lib().mcpt_refit_mesh(self._h, int(mesh_id), None), "mcpt_refit_mesh")
            return None
        rec = Refit()
        _check(lib().mcpt_refit_mesh(self._h, int(mesh_id), ctypes.byref(rec)), "mcpt_refit_mesh")
        return {"triangles": rec.triangles, "leaves": rec.leaves, "internal_nodes": rec.internal_nodes,
                "device_ms": rec.device_ms,
                "root_box": np.array(rec.root_box[:], np.float32) if rec.has_root else None}

    def rebuild_mesh(self, mesh_id: int = -1, tris=None, record: bool = True) -> Optional[dict]:
        """mcpt_rebuild_mesh: the BVH of mesh `mesh_id` (-1: every mesh, without tris) rebuilt on the device
        from the current vertices — a new leaf order by stable median splits, then the refit; tris (n x 3
        mesh-local vertex indices, the mesh's count) replaces its triangles first.  record=True waits and
        returns {triangles, rounds, sort_passes, sort_ms, refit_ms, device_ms, root_box (a single mesh of
        depth >= 1, else None)}; record=False queues it only."""
        t, tp, nt = None, None, 0
        if tris is not None:
            t = np.ascontiguousarray(np.asarray(tris, np.int32).reshape(-1, 3))
            tp, nt = _ip(t), t.shape[0]
        if not record:
            _check(lib().mcpt_rebuild_mesh(self._h, int(mesh_id), tp, nt, None), "mcpt_rebuild_mesh")
            return None
        rec = Rebuild()
        _check(lib().mcpt_rebuild_mesh(self._h, int(mesh_id), tp, nt, ctypes.byref(rec)), "mcpt_rebuild_mesh")
        return {"triangles": rec.triangles, "rounds": rec.rounds, "sort_passes": rec.sort_passes,
                "sort_ms": rec.sort_ms, "refit_ms": rec.refit_ms, "device_ms": rec.sort_ms + rec.refit_ms,
                "root_box": np.array(rec.root_box[:], np.float32) if rec.has_root else None}

    def mesh_records(self) -> dict:
        """mcpt_debug_mesh_records: {"pairs": (slots, 4, 4) f32, "leaves": (leaves, 4, 4) f32}, the device's
        child-pair slots and leaf triangle records as they stand (diagnostics; synchronizes)."""
        np_, nl = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().mcpt_debug_mesh_record_sizes(self._h, ctypes.byref(np_), ctypes.byref(nl)),
               "mcpt_debug_mesh_record_sizes")
        pairs, leaves = np.zeros(np_.value, np.float32), np.zeros(nl.value, np.float32)
        _check(lib().mcpt_debug_mesh_records(self._h, _fp(pairs), pairs.size, _fp(leaves), leaves.size),
               "mcpt_debug_mesh_records")
        return {"pairs": pairs.reshape(-1, 4, 4), "leaves": leaves.reshape(-1, 4, 4)}

    def set_flat_face(self, flat: bool) -> None:
        _check(lib().mcpt_set_flat_face(self._h, int(bool(flat))), "mcpt_set_flat_face")

    def set_target(self, W: int, H: int, band_rows: int = 8, world: int = 1, rank: int = 0) -> None:
        _check(lib().mcpt_set_target(self._h, int(W), int(H), int(band_rows), int(world), int(rank)),
               "mcpt_set_target")
        self.W, self.H = int(W), int(H)
        self.band_rows, self.world, self.rank = int(band_rows), int(world), int(rank)
        n = ctypes.c_int()
        _check(lib().mcpt_local_rows(self._h, ctypes.byref(n)), "mcpt_local_rows")
        self.n_local_rows = n.value

    def set_target_rows(self, W: int, H: int, rows) -> None:
        """Explicit shard (mcpt_set_target_rows): local row i renders global row rows[i]."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        _check(lib().mcpt_set_target_rows(self._h, int(W), int(H), _ip(r), int(r.size)), "mcpt_set_target_rows")
        self.W, self.H = int(W), int(H)
        self.band_rows, self.world, self.rank = 0, 0, 0
        self.n_local_rows = int(r.size)

    def local_row_ids(self) -> np.ndarray:
        out = np.zeros(self.n_local_rows, np.int32)
        if self.n_local_rows:
            _check(lib().mcpt_local_row_ids(self._h, _ip(out)), "mcpt_local_row_ids")
        return out.astype(np.int64)

    def render(self, invPV, invV, first_pass: int, n_passes: int, date: float = 0.0,
               bounces: int = 3, refract_ind: float = 1.0, variant: int = MONTECARLO) -> None:
        a, b = _f32(invPV, 16), _f32(invV, 16)
        _check(lib().mcpt_render(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes), float(date),
                                 int(bounces), float(refract_ind), int(variant)), "mcpt_render")

    def render_counted(self, invPV, invV, first_pass: int, n_passes: int, date: float = 0.0,
                       bounces: int = 3, refract_ind: float = 1.0, variant: int = MONTECARLO) -> np.ndarray:
        a, b = _f32(invPV, 16), _f32(invV, 16)
        ev = np.zeros(len(EVENT_NAMES), np.uint64)
        _check(lib().mcpt_render_counted(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes),
                                         float(date), int(bounces), float(refract_ind), int(variant),
                                         ev.ctypes.data_as(_c_u64_p)), "mcpt_render_counted")
        return ev

    def debug_counters(self, reset: bool = True) -> np.ndarray:
        """The context's MCPT_DEBUG_SLOTS device counter slots (diagnostic builds write there)."""
        out = np.zeros(DEBUG_SLOTS, np.uint64)
        _check(lib().mcpt_debug_counters(self._h, out.ctypes.data_as(_c_u64_p), out.size, int(reset)),
               "mcpt_debug_counters")
        return out

    @staticmethod
    def event_bytes() -> np.ndarray:
        return np.array([lib().mcpt_event_bytes(e) for e in range(len(EVENT_NAMES))], np.int64)

    def read_accum(self) -> Tuple[np.ndarray, int]:
        """(local rows × W × 3 f32 sums, pass count)."""
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        pc = ctypes.c_int()
        _check(lib().mcpt_read_accum(self._h, _fp(out), ctypes.byref(pc)), "mcpt_read_accum")
        return out, pc.value

    def read_image(self) -> np.ndarray:
        """Averaged image (fs_frag: accum / nb, montecarlo.cpp:59-70); single-shard only."""
        acc, n = self.read_accum()
        full = self.n_local_rows == self.H and (self.world != 0 or
                                                np.array_equal(self.local_row_ids(), np.arange(self.H)))
        if not full:
            raise MCPTError("read_image needs the full frame in row order; gather shards with mcpt.dist")
        return acc / max(n, 1)

    def clear_accum(self) -> None:
        _check(lib().mcpt_clear_accum(self._h), "mcpt_clear_accum")

    def write_accum(self, accum: np.ndarray, pass_count: int) -> None:
        """mcpt_write_accum: load local rows × W × 3 sums holding `pass_count` passes."""
        a = np.ascontiguousarray(accum, np.float32)
        if a.shape != (self.n_local_rows, self.W, 3):
            raise MCPTError(f"write_accum: expected {(self.n_local_rows, self.W, 3)}, got {a.shape}")
        _check(lib().mcpt_write_accum(self._h, _fp(a), int(pass_count)), "mcpt_write_accum")

    def save_checkpoint(self, path: str, next_pass: int, tag: str = "") -> None:
        """mcpt_checkpoint_save: this context's accumulator, its pass count, `next_pass`, `tag` and
        the target's identity (H, row ids) to `path`."""
        _check(lib().mcpt_checkpoint_save(self._h, str(path).encode(), int(next_pass), tag.encode()),
               "mcpt_checkpoint_save")

    def load_checkpoint(self, path: str, tag: Optional[str] = None) -> int:
        """mcpt_checkpoint_load: resume from `path` — it must have been saved for this target
        (W, H, row ids) and, if `tag` is given, with that tag; loads the sums and pass count and
        returns the first pass of the next render call."""
        nxt = ctypes.c_int()
        _check(lib().mcpt_checkpoint_load(self._h, str(path).encode(), None if tag is None else tag.encode(),
                                          ctypes.byref(nxt)), "mcpt_checkpoint_load")
        return nxt.value

    def accum_device_ptr(self) -> Tuple[int, int]:
        p = _vp()
        n = ctypes.c_size_t()
        _check(lib().mcpt_accum_device_ptr(self._h, ctypes.byref(p), ctypes.byref(n)), "mcpt_accum_device_ptr")
        return int(p.value or 0), int(n.value)

    def copy_accum_device(self, dst_ptr: int, nbytes: int) -> None:
        """D2D copy of the local accumulator into a device buffer (ordered on our stream)."""
        _check(lib().mcpt_copy_accum_device(self._h, _vp(dst_ptr), ctypes.c_size_t(nbytes)),
               "mcpt_copy_accum_device")

    def gather_rows(self, shards) -> None:
        """This full-frame renderer's accumulator <- the shard renderers' rows (mcpt_gather_rows:
        device-to-device peer copies inside one process, ordered after the shards' renders)."""
        hs = (_vp * max(len(shards), 1))(*[s._h for s in shards])
        _check(lib().mcpt_gather_rows(self._h, hs, len(shards)), "mcpt_gather_rows")

    # ---- guide buffers and the a-trous denoiser (mcpt.h)
    def render_guides(self, invPV, invV) -> None:
        """mcpt_render_guides: the primary hit of every local pixel's camera ray (asynchronous)."""
        a, b = _f32(invPV, 16), _f32(invV, 16)
        _check(lib().mcpt_render_guides(self._h, _fp(a), _fp(b)), "mcpt_render_guides")

    def read_guides(self) -> dict:
        """The guide buffers as local rows x W arrays: normal (.., 3), key (int32: shape << 28 |
        primitive index, -1 = miss), position (.., 3), dist, albedo (.., 4 rgba)."""
        g = np.zeros((self.n_local_rows, self.W, 8), np.float32)
        al = np.zeros((self.n_local_rows, self.W, 4), np.float32)
        _check(lib().mcpt_read_guides(self._h, _fp(g), _fp(al)), "mcpt_read_guides")
        return {"normal": np.ascontiguousarray(g[..., 0:3]), "key": np.ascontiguousarray(g[..., 3]).view(np.int32),
                "position": np.ascontiguousarray(g[..., 4:7]), "dist": np.ascontiguousarray(g[..., 7]),
                "albedo": al}

    def denoise(self, iterations: int = 5, sigma_color: float = DENOISE_SIGMA_COLOR,
                sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise + mcpt_read_denoised: the H x W x 3 image after `iterations` a-trous passes
        over accum / pass_count (the accumulator stays as it is).  Needs render_guides first."""
        _check(lib().mcpt_denoise(self._h, int(iterations), float(sigma_color), float(sigma_plane)), "mcpt_denoise")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def last_denoise_ms(self) -> Tuple[float, float]:
        """(guides kernel ms, filter ms) of the last render_guides / denoise."""
        g, fl = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_last_denoise_ms(self._h, ctypes.byref(g), ctypes.byref(fl)), "mcpt_last_denoise_ms")
        return g.value, fl.value

    def denoise_iteration_ms(self, iteration: int) -> float:
        """Device ms of one iteration of the last denoise (-1: its averaging step)."""
        ms = ctypes.c_float()
        _check(lib().mcpt_denoise_iteration_ms(self._h, int(iteration), ctypes.byref(ms)), "mcpt_denoise_iteration_ms")
        return ms.value

    def last_denoise_path(self) -> int:
        """Bit s set: iteration s of the last denoise staged its taps in LDS (clear: global taps)."""
        m = ctypes.c_int()
        _check(lib().mcpt_last_denoise_path(self._h, ctypes.byref(m)), "mcpt_last_denoise_path")
        return m.value

    # ---- noise statistics, convergence and the noise-guided filter (mcpt.h)
    def stats_begin(self) -> None:
        """mcpt_stats_begin: start a statistics window at the accumulator as it is (asynchronous);
        from now on every render call is one batch."""
        _check(lib().mcpt_stats_begin(self._h), "mcpt_stats_begin")

    def stats_end(self) -> None:
        """mcpt_stats_end: statistics off, their buffers freed."""
        _check(lib().mcpt_stats_end(self._h), "mcpt_stats_end")

    def stats_add_batch(self, n: int) -> None:
        """mcpt_stats_add_batch: the accumulator holds n more passes than at the previous batch
        (after write_accum / load_checkpoint / gather_rows; render calls declare theirs)."""
        _check(lib().mcpt_stats_add_batch(self._h, int(n)), "mcpt_stats_add_batch")

    def stats_info(self) -> dict:
        """{"on", "passes", "batches"} of the statistics window."""
        on, b, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        _check(lib().mcpt_stats_info(self._h, ctypes.byref(on), ctypes.byref(n), ctypes.byref(b)), "mcpt_stats_info")
        return {"on": bool(on.value), "passes": n.value, "batches": b.value}

    def convergence(self, threshold: float, mu_floor: float = ERROR_MU_FLOOR) -> dict:
        """mcpt_convergence: the frame record {n_px, n_above (r > threshold), sum_q, max_r, mean_r,
        passes, batches} of the local pixels' relative errors; writes the error map.  Synchronizes."""
        rec = Convergence()
        _check(lib().mcpt_convergence(self._h, float(threshold), float(mu_floor), ctypes.byref(rec)), "mcpt_convergence")
        return {k: getattr(rec, k) for k, _ in Convergence._fields_}

    def read_error_map(self) -> np.ndarray:
        """(local rows, W, 2) f32: {standard error of the mean luminance, relative error r} of the
        last convergence() / adaptive_select(); on a frame with a gathered error map
        (gather_error_map, load_rows_error_map) that map, (H, W, 2)."""
        out = np.zeros((self.n_local_rows, self.W, 2), np.float32)
        _check(lib().mcpt_read_error_map(self._h, _fp(out)), "mcpt_read_error_map")
        return out

    def denoise_guided(self, iterations: int = 5, k_color: float = DENOISE_K_COLOR,
                       sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_guided + mcpt_read_denoised: denoise() with the colour width per pixel,
        k_color standard errors of that pixel (needs render_guides and a convergence() first)."""
        _check(lib().mcpt_denoise_guided(self._h, int(iterations), float(k_color), float(sigma_plane)),
               "mcpt_denoise_guided")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def denoise_variance(self, iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                         sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_variance + mcpt_read_denoised: the variance-propagating filter (the error
        map's se^2 prefiltered 3x3, carried and filtered through the iterations; the colour width
        is k_color standard deviations of the variance the iteration's input has).  Needs what
        denoise_guided needs; read_denoised_variance() returns the filtered variance."""
        _check(lib().mcpt_denoise_variance(self._h, int(iterations), float(k_color), float(sigma_plane)),
               "mcpt_denoise_variance")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def read_denoised_variance(self) -> np.ndarray:
        """mcpt_read_denoised_variance: (local rows, W) f32, the variance the last denoise_variance /
        denoise_resolved_variance carried to its result."""
        out = np.zeros((self.n_local_rows, self.W), np.float32)
        _check(lib().mcpt_read_denoised_variance(self._h, _fp(out)), "mcpt_read_denoised_variance")
        return out

    def last_stats_ms(self) -> Tuple[float, float]:
        """(batch update ms, error kernel ms) of the last of each (0: none yet)."""
        u, e = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_last_stats_ms(self._h, ctypes.byref(u), ctypes.byref(e)), "mcpt_last_stats_ms")
        return u.value, e.value

    def render_until(self, invPV, invV, target_error: float, batch: int = 32, max_passes: int = 4096,
                     check_every: int = 4, first_pass: int = 1, date: float = 0.0, bounces: int = 3,
                     refract_ind: float = 1.0, variant: int = MONTECARLO, threshold: Optional[float] = None,
                     mu_floor: float = ERROR_MU_FLOOR) -> dict:
        """Render passes first_pass, first_pass + 1, ... in calls of `batch` passes until the mean
        relative error is at most `target_error` or `max_passes` passes are rendered.  The
        convergence is queried after every `check_every` calls (and at the cap), the calls in
        between are queued without a wait, so that render lanes keep overlapping.  Begins a
        statistics window unless one is on (then its batches count too).  Returns the last
        convergence record plus "rendered" (this call's passes) and "converged"; `threshold`
        (n_above's bound) defaults to target_error."""
        if batch <= 0 or check_every <= 0 or max_passes <= 0 or not target_error > 0:
            raise MCPTError("render_until: batch, check_every, max_passes and target_error must be positive")
        if not self.stats_info()["on"]:
            self.stats_begin()
        thr = target_error if threshold is None else threshold
        done, calls, rec = 0, 0, None
        while done < max_passes:
            n = min(batch, max_passes - done)
            self.render(invPV, invV, first_pass + done, n, date, bounces, refract_ind, variant)
            done += n
            calls += 1
            if (calls % check_every == 0 or done >= max_passes) and self.stats_info()["batches"] >= 2:
                rec = self.convergence(thr, mu_floor)
                if rec["mean_r"] <= target_error:
                    break
        if rec is None:
            rec = self.convergence(thr, mu_floor)     # (fewer than two batches: MCPT_ERR_NO_STATS)
        rec["rendered"] = done
        rec["converged"] = rec["mean_r"] <= target_error
        return rec

    # ---- adaptive sampling of 8x8 blocks (mcpt.h)
    def adaptive_begin(self, min_passes: int = 0) -> None:
        """mcpt_adaptive_begin: every 8x8 block active with zero passes (needs statistics on)."""
        _check(lib().mcpt_adaptive_begin(self._h, int(min_passes)), "mcpt_adaptive_begin")

    def adaptive_end(self) -> None:
        """mcpt_adaptive_end: adaptive mode off, its state freed."""
        _check(lib().mcpt_adaptive_end(self._h), "mcpt_adaptive_end")

    def adaptive_select(self, threshold: float, mu_floor: float = ERROR_MU_FLOOR) -> dict:
        """mcpt_adaptive_select: retire the active blocks whose largest r <= threshold (and that hold
        min_passes); convergence()'s record over all local pixels plus n_active_blocks, n_blocks and
        samples.  Synchronizes."""
        rec = Adaptive()
        _check(lib().mcpt_adaptive_select(self._h, float(threshold), float(mu_floor), ctypes.byref(rec)),
               "mcpt_adaptive_select")
        return {k: getattr(rec, k) for k, _ in Adaptive._fields_}

    def adaptive_select_filtered(self, threshold: float, raw_cap: float = 64.0, mu_floor: float = ERROR_MU_FLOOR,
                                 iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                                 sigma_plane: float = DENOISE_SIGMA_PLANE) -> dict:
        """mcpt_adaptive_select_filtered: the select on the denoised frame's error.  Writes the error
        map, runs denoise_resolved_variance(iterations, k_color, sigma_plane) on it and retires the
        active blocks whose largest filtered error rf <= threshold and largest raw r <= raw_cap (and
        that hold min_passes).  adaptive_select()'s keys (n_active_blocks: what this rule keeps) plus
        n_above_f, sum_qf, max_rf, mean_rf of rf over all local pixels.  read_denoised() /
        read_denoised_variance() then return the filter's image.  Needs render_guides.  Synchronizes."""
        rec = AdaptiveFiltered()
        _check(lib().mcpt_adaptive_select_filtered(self._h, float(threshold), float(raw_cap), float(mu_floor),
                                                   int(iterations), float(k_color), float(sigma_plane),
                                                   ctypes.byref(rec)), "mcpt_adaptive_select_filtered")
        return self._filtered_dict(rec)

    def read_denoised(self) -> np.ndarray:
        """mcpt_read_denoised: (local rows, W, 3) f32, the last filter run's image."""
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def adaptive_info(self) -> dict:
        """{"on", "n_active", "n_blocks"} of the adaptive mode."""
        on, a, b = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        _check(lib().mcpt_adaptive_info(self._h, ctypes.byref(on), ctypes.byref(a), ctypes.byref(b)), "mcpt_adaptive_info")
        return {"on": bool(on.value), "n_active": a.value, "n_blocks": b.value}

    def read_active_blocks(self) -> np.ndarray:
        """The active block ids (by * ceil(W / 8) + bx over the local grid), ascending."""
        out = np.zeros(max(self.adaptive_info()["n_blocks"], 1), np.int32)
        n = ctypes.c_int()
        _check(lib().mcpt_read_active_blocks(self._h, _ip(out), int(out.size), ctypes.byref(n)), "mcpt_read_active_blocks")
        return out[:n.value].copy()

    def render_adaptive(self, invPV, invV, first_pass: int, n_passes: int, date: float = 0.0,
                        bounces: int = 3, refract_ind: float = 1.0, variant: int = MONTECARLO) -> None:
        """mcpt_render_adaptive: render() for the active blocks only."""
        a, b = _f32(invPV, 16), _f32(invV, 16)
        _check(lib().mcpt_render_adaptive(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes), float(date),
                                          int(bounces), float(refract_ind), int(variant)), "mcpt_render_adaptive")

    def read_sample_counts(self) -> np.ndarray:
        """(local rows, W) i32: every pixel's sample count."""
        out = np.zeros((self.n_local_rows, self.W), np.int32)
        _check(lib().mcpt_read_sample_counts(self._h, _ip(out)), "mcpt_read_sample_counts")
        return out

    def read_resolved(self) -> np.ndarray:
        """(local rows, W, 3) f32: accum / (float)count with every pixel's own sample count."""
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_resolved(self._h, _fp(out)), "mcpt_read_resolved")
        return out

    def last_adaptive_ms(self) -> Tuple[float, float]:
        """(select ms, adaptive render ms) of the last of each (0: none yet)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_last_adaptive_ms(self._h, ctypes.byref(a), ctypes.byref(b)), "mcpt_last_adaptive_ms")
        return a.value, b.value

    @staticmethod
    def _filtered_dict(rec: AdaptiveFiltered) -> dict:
        out = {k: getattr(rec.raw, k) for k, _ in Adaptive._fields_}
        out.update({k: getattr(rec, k) for k in ("n_above_f", "sum_qf", "max_rf", "mean_rf")})
        return out

    def adaptive_run(self, invPV, invV, first_pass: int, n_passes: int, rounds: int, threshold: float,
                     check_every: int = 1, mu_floor: float = ERROR_MU_FLOOR, date: float = 0.0, bounces: int = 3,
                     refract_ind: float = 1.0, variant: int = MONTECARLO) -> dict:
        """mcpt_adaptive_run: `rounds` rounds of {render_adaptive(first_pass + i * n_passes, n_passes),
        on the schedule's rounds adaptive_select(threshold, mu_floor)} queued on the device, the same
        bits as that loop, one wait at the end.  {"rounds_queued", "rounds_run", "selects_run",
        "passes_run", "device_ms", "records": adaptive_select()'s dicts in order}."""
        a, b = _f32(invPV, 16), _f32(invV, 16)
        cap = max(int(rounds), 1)
        recs, run = (Adaptive * cap)(), AdaptiveRun()
        _check(lib().mcpt_adaptive_run(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes), int(rounds),
                                       int(check_every), float(threshold), float(mu_floor), float(date), int(bounces),
                                       float(refract_ind), int(variant), recs, cap, ctypes.byref(run)),
               "mcpt_adaptive_run")
        out = {k: getattr(run, k) for k, _ in AdaptiveRun._fields_}
        out["records"] = [{k: getattr(recs[j], k) for k, _ in Adaptive._fields_} for j in range(run.selects_run)]
        return out

    def adaptive_run_filtered(self, invPV, invV, first_pass: int, n_passes: int, rounds: int, threshold: float,
                              check_every: int = 1, raw_cap: float = 64.0, mu_floor: float = ERROR_MU_FLOOR,
                              iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                              sigma_plane: float = DENOISE_SIGMA_PLANE, date: float = 0.0, bounces: int = 3,
                              refract_ind: float = 1.0, variant: int = MONTECARLO) -> dict:
        """mcpt_adaptive_run_filtered: adaptive_run() whose selects are adaptive_select_filtered(threshold,
        raw_cap, mu_floor, iterations, k_color, sigma_plane); the records are that call's dicts."""
        a, b = _f32(invPV, 16), _f32(invV, 16)
        cap = max(int(rounds), 1)
        recs, run = (AdaptiveFiltered * cap)(), AdaptiveRun()
        _check(lib().mcpt_adaptive_run_filtered(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes), int(rounds),
                                                int(check_every), float(threshold), float(raw_cap), float(mu_floor),
                                                int(iterations), float(k_color), float(sigma_plane), float(date),
                                                int(bounces), float(refract_ind), int(variant), recs, cap,
                                                ctypes.byref(run)), "mcpt_adaptive_run_filtered")
        out = {k: getattr(run, k) for k, _ in AdaptiveRun._fields_}
        out["records"] = [self._filtered_dict(recs[j]) for j in range(run.selects_run)]
        return out

    def render_adaptive_until(self, invPV, invV, threshold: float, batch: int = 32, max_passes: int = 4096,
                              min_passes: int = 0, check_every: int = 1, first_pass: int = 1, date: float = 0.0,
                              bounces: int = 3, refract_ind: float = 1.0, variant: int = MONTECARLO,
                              mu_floor: float = ERROR_MU_FLOOR, filtered: bool = False, raw_cap: float = 64.0,
                              iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                              sigma_plane: float = DENOISE_SIGMA_PLANE, queued_rounds: int = 0) -> dict:
        """Begin a statistics window and the adaptive mode, then render passes first_pass,
        first_pass + 1, ... in calls of `batch` passes for the active blocks only, selecting after
        every `check_every` calls (from the second batch on, and at the cap), until no block is
        active or `max_passes` passes are rendered.  Returns the last select's record plus
        "rendered" (the passes the longest-lived blocks received); the mode stays on, so that
        read_resolved() and read_sample_counts() serve the result.  filtered: the selects are
        adaptive_select_filtered(threshold, raw_cap, mu_floor, iterations, k_color, sigma_plane), the
        guides are rendered first unless they are current, and read_denoised() serves the last
        select's image.  queued_rounds K > 0: the calls go out as queued runs of up to K rounds
        (adaptive_run / adaptive_run_filtered: one host wait per run instead of one per select);
        the same record and the same "rendered" come back."""
        if batch <= 0 or check_every <= 0 or max_passes <= 0 or not threshold > 0 or queued_rounds < 0:
            raise MCPTError("render_adaptive_until: batch, check_every, max_passes and threshold must be positive")
        if filtered:
            select = lambda: self.adaptive_select_filtered(threshold, raw_cap, mu_floor, iterations, k_color, sigma_plane)
            run = lambda p, r: self.adaptive_run_filtered(invPV, invV, p, batch, r, threshold, check_every, raw_cap,
                                                          mu_floor, iterations, k_color, sigma_plane, date, bounces,
                                                          refract_ind, variant)
            if lib().mcpt_read_guides(self._h, None, None) == NO_GUIDES:      # (copies nothing: the guides' state alone)
                self.render_guides(invPV, invV)
        else:
            select = lambda: self.adaptive_select(threshold, mu_floor)
            run = lambda p, r: self.adaptive_run(invPV, invV, p, batch, r, threshold, check_every, mu_floor, date,
                                                 bounces, refract_ind, variant)
        self.stats_begin()
        self.adaptive_begin(min_passes)
        render = lambda p, n: self.render_adaptive(invPV, invV, p, n, date, bounces, refract_ind, variant)
        rec, done, _ = _adaptive_until(render, select, run, first_pass, batch, max_passes, check_every, queued_rounds)
        rec["rendered"] = done
        return rec

    # ---- temporal reprojection across camera moves (mcpt.h)
    def temporal_begin(self) -> None:
        """mcpt_temporal_begin: temporal mode on, the history allocated and empty (asynchronous)."""
        _check(lib().mcpt_temporal_begin(self._h), "mcpt_temporal_begin")

    def temporal_end(self) -> None:
        """mcpt_temporal_end: temporal mode off, the history freed."""
        _check(lib().mcpt_temporal_end(self._h), "mcpt_temporal_end")

    def temporal_info(self) -> dict:
        """{"on", "history_valid", "frames"} of the temporal mode."""
        on, v, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        _check(lib().mcpt_temporal_info(self._h, ctypes.byref(on), ctypes.byref(v), ctypes.byref(n)), "mcpt_temporal_info")
        return {"on": bool(on.value), "history_valid": bool(v.value), "frames": n.value}

    def temporal_accumulate(self, prevPV=None, max_history: int = TEMPORAL_MAX_HISTORY,
                            plane_tol: float = TEMPORAL_PLANE_TOL) -> dict:
        """mcpt_temporal_accumulate: reproject the history through prevPV (the P·V of the camera it was
        made with, 16 f32 column-major; None only while the history is empty) and blend the current
        frame in; the record {n_px, n_history, n_new, n_miss, n_offscreen, n_rejected, sum_len, max_len,
        frames}.  Needs a convergence() and render_guides() of the current frame.  Synchronizes."""
        rec = TemporalRecord()
        m = None if prevPV is None else _f32(prevPV, 16)
        _check(lib().mcpt_temporal_accumulate(self._h, None if m is None else _fp(m), int(max_history), float(plane_tol),
                                              ctypes.byref(rec)), "mcpt_temporal_accumulate")
        return {k: getattr(rec, k) for k, _ in TemporalRecord._fields_}

    def read_temporal(self) -> Tuple[np.ndarray, np.ndarray]:
        """mcpt_read_temporal: ((local rows, W, 4) f32 {rgb, variance of the mean}, (local rows, W) i32
        history lengths) of the history."""
        c = np.zeros((self.n_local_rows, self.W, 4), np.float32)
        n = np.zeros((self.n_local_rows, self.W), np.int32)
        _check(lib().mcpt_read_temporal(self._h, _fp(c), _ip(n)), "mcpt_read_temporal")
        return c, n

    def denoise_temporal(self, iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                         sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_temporal + mcpt_read_denoised: the variance filter from the temporal image;
        read_denoised_variance() returns the filtered variance."""
        _check(lib().mcpt_denoise_temporal(self._h, int(iterations), float(k_color), float(sigma_plane)),
               "mcpt_denoise_temporal")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def last_temporal_ms(self) -> Tuple[float, float]:
        """(accumulate kernel ms, guides copy ms) of the last temporal_accumulate."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_last_temporal_ms(self._h, ctypes.byref(a), ctypes.byref(b)), "mcpt_last_temporal_ms")
        return a.value, b.value

    def render_frame_temporal(self, invPV, invV, prevPV, first_pass: int, spp: int = 4, batches: int = 2,
                              date: float = 0.0, bounces: int = 3, refract_ind: float = 1.0,
                              variant: int = MONTECARLO, max_history: int = TEMPORAL_MAX_HISTORY,
                              plane_tol: float = TEMPORAL_PLANE_TOL, iterations: int = 5,
                              k_color: float = DENOISE_K_VARIANCE, sigma_plane: float = DENOISE_SIGMA_PLANE,
                              threshold: float = 0.05, mu_floor: float = ERROR_MU_FLOOR) -> Tuple[np.ndarray, dict]:
        """One frame of a moving-camera render: clear the accumulator, `spp` passes from `first_pass` on
        in `batches` render calls (two or more: the error map needs them) under a fresh statistics
        window, the error map, the guides of this camera, temporal_accumulate(prevPV) and
        denoise_temporal.  Begins the temporal mode unless it is on.  Returns (the filtered H x W x 3
        image, the accumulate's record); the next frame's first_pass is first_pass + spp and its
        prevPV is mat4_inverse(invPV) of this one."""
        if batches < 2 or spp < batches:
            raise MCPTError("render_frame_temporal: two batches or more, one pass or more each")
        if not self.temporal_info()["on"]:
            self.temporal_begin()
        self.clear_accum()
        self.stats_begin()
        done = 0
        for b in range(batches):
            n = spp // batches + (1 if b < spp % batches else 0)
            self.render(invPV, invV, first_pass + done, n, date, bounces, refract_ind, variant)
            done += n
        self.convergence(threshold, mu_floor)
        self.render_guides(invPV, invV)
        rec = self.temporal_accumulate(prevPV, max_history, plane_tol)
        return self.denoise_temporal(iterations, k_color, sigma_plane), rec

    # ---- temporal adaptive sampling: render only the blocks the history cannot carry (mcpt.h;
    # DESIGN.md §3.10.1)
    def temporal_accumulate_resolved(self, prevPV=None, max_history: int = TEMPORAL_MAX_HISTORY,
                                     plane_tol: float = TEMPORAL_PLANE_TOL) -> dict:
        """mcpt_temporal_accumulate_resolved: temporal_accumulate() whose current colour is accum /
        (float)count with every pixel's own sample count (the adaptive mode must be on; retired blocks
        are allowed and keep the error map entries they retired with).  The same record."""
        rec = TemporalRecord()
        m = None if prevPV is None else _f32(prevPV, 16)
        _check(lib().mcpt_temporal_accumulate_resolved(self._h, None if m is None else _fp(m), int(max_history),
                                                       float(plane_tol), ctypes.byref(rec)),
               "mcpt_temporal_accumulate_resolved")
        return {k: getattr(rec, k) for k, _ in TemporalRecord._fields_}

    @staticmethod
    def _temporal_dict(rec: AdaptiveTemporal) -> dict:
        out = {k: getattr(rec.raw, k) for k, _ in Adaptive._fields_}
        out.update({k: getattr(rec, k) for k, _ in AdaptiveTemporal._fields_[1:]})
        return out

    def adaptive_select_temporal(self, prevPV=None, threshold: float = TEMPORAL_TARGET,
                                 max_history: int = TEMPORAL_MAX_HISTORY, plane_tol: float = TEMPORAL_PLANE_TOL,
                                 mu_floor: float = ERROR_MU_FLOOR) -> dict:
        """mcpt_adaptive_select_temporal: the select on the error of the blend that
        temporal_accumulate_resolved(prevPV, max_history, plane_tol) would write now.  Writes the error
        map as adaptive_select() does, reads the history and leaves it alone, and retires the active
        blocks whose largest rt <= threshold (and that hold min_passes).  adaptive_select()'s keys
        (n_active_blocks: what this rule keeps) plus n_px_t, n_above_t, sum_qt, max_rt, mean_rt and
        n_history over the pixels of the blocks active on entry.  Needs render_guides() of the camera
        being rendered."""
        rec = AdaptiveTemporal()
        m = None if prevPV is None else _f32(prevPV, 16)
        _check(lib().mcpt_adaptive_select_temporal(self._h, None if m is None else _fp(m), int(max_history),
                                                   float(plane_tol), float(threshold), float(mu_floor),
                                                   ctypes.byref(rec)), "mcpt_adaptive_select_temporal")
        return self._temporal_dict(rec)

    def adaptive_run_temporal(self, invPV, invV, first_pass: int, n_passes: int, rounds: int, prevPV=None,
                              threshold: float = TEMPORAL_TARGET, check_every: int = 1,
                              max_history: int = TEMPORAL_MAX_HISTORY, plane_tol: float = TEMPORAL_PLANE_TOL,
                              mu_floor: float = ERROR_MU_FLOOR, date: float = 0.0, bounces: int = 3,
                              refract_ind: float = 1.0, variant: int = MONTECARLO) -> dict:
        """mcpt_adaptive_run_temporal: adaptive_run() whose selects are adaptive_select_temporal(prevPV,
        threshold, max_history, plane_tol, mu_floor); the records are that call's dicts."""
        a, b = _f32(invPV, 16), _f32(invV, 16)
        m = None if prevPV is None else _f32(prevPV, 16)
        cap = max(int(rounds), 1)
        recs, run = (AdaptiveTemporal * cap)(), AdaptiveRun()
        _check(lib().mcpt_adaptive_run_temporal(self._h, _fp(a), _fp(b), int(first_pass), int(n_passes), int(rounds),
                                                int(check_every), float(threshold), float(mu_floor),
                                                None if m is None else _fp(m), int(max_history), float(plane_tol),
                                                float(date), int(bounces), float(refract_ind), int(variant), recs, cap,
                                                ctypes.byref(run)), "mcpt_adaptive_run_temporal")
        out = {k: getattr(run, k) for k, _ in AdaptiveRun._fields_}
        out["records"] = [self._temporal_dict(recs[j]) for j in range(run.selects_run)]
        return out

    def render_frame_temporal_adaptive(self, invPV, invV, prevPV, first_pass: int, cap_spp: int = 16,
                                       n_passes: int = 2, threshold: float = TEMPORAL_TARGET, date: float = 0.0,
                                       bounces: int = 3, refract_ind: float = 1.0, variant: int = MONTECARLO,
                                       max_history: int = TEMPORAL_MAX_HISTORY, plane_tol: float = TEMPORAL_PLANE_TOL,
                                       iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                                       sigma_plane: float = DENOISE_SIGMA_PLANE, mu_floor: float = ERROR_MU_FLOOR,
                                       min_passes: int = 0, queued: bool = True) -> Tuple[np.ndarray, dict, dict]:
        """One frame of a moving-camera render that spends samples only where the history cannot carry
        the pixel: clear the accumulator, a fresh statistics window and adaptive state, the guides of
        this camera, then rounds of `n_passes` passes for the active blocks, up to cap_spp // n_passes
        rounds, with adaptive_select_temporal(prevPV, threshold) after every round from the second on
        (queued: as one adaptive_run_temporal, one host wait; else the host loop, the same bits), then
        temporal_accumulate_resolved(prevPV) and denoise_temporal.  Begins the temporal mode unless it
        is on.  Returns (the filtered H x W x 3 image, the accumulate's record, the last select's record
        with "rendered": the passes the longest-lived blocks received).  The next frame's first_pass is
        first_pass + cap_spp (pass ids never repeat whatever a frame rendered) and its prevPV is
        mat4_inverse(invPV) of this one."""
        if n_passes <= 0 or cap_spp < 2 * n_passes or not threshold > 0:
            raise MCPTError("render_frame_temporal_adaptive: positive n_passes and threshold, cap_spp of two "
                            "rounds or more")
        rounds = min(cap_spp // n_passes, ADAPTIVE_RUN_MAX_ROUNDS)
        if not self.temporal_info()["on"]:
            self.temporal_begin()
        self.clear_accum()
        self.stats_begin()
        self.adaptive_begin(min_passes)
        self.render_guides(invPV, invV)
        if queued:
            got = self.adaptive_run_temporal(invPV, invV, first_pass, n_passes, rounds, prevPV, threshold, 1,
                                             max_history, plane_tol, mu_floor, date, bounces, refract_ind, variant)
            sel, done = got["records"][-1], got["rounds_run"] * n_passes
        else:
            render = lambda p, n: self.render_adaptive(invPV, invV, p, n, date, bounces, refract_ind, variant)
            select = lambda: self.adaptive_select_temporal(prevPV, threshold, max_history, plane_tol, mu_floor)
            sel, done, _ = _adaptive_until(render, select, None, first_pass, n_passes, rounds * n_passes)
        sel["rendered"] = done
        rec = self.temporal_accumulate_resolved(prevPV, max_history, plane_tol)
        return self.denoise_temporal(iterations, k_color, sigma_plane), rec, sel

    # ---- frames with per-pixel sample counts: filter, checkpoint, gather (mcpt.h)
    def denoise_resolved(self, iterations: int = 5, sigma_color: float = DENOISE_SIGMA_COLOR,
                         sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_resolved + mcpt_read_denoised: denoise() over accum / (float)count with every
        pixel's own sample count (adaptive mode on, or after gather_rows_counted)."""
        _check(lib().mcpt_denoise_resolved(self._h, int(iterations), float(sigma_color), float(sigma_plane)),
               "mcpt_denoise_resolved")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def denoise_resolved_guided(self, iterations: int = 5, k_color: float = DENOISE_K_COLOR,
                                sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_resolved_guided + mcpt_read_denoised: denoise_guided() over the resolved
        colour, with the error map of the last adaptive_select()."""
        _check(lib().mcpt_denoise_resolved_guided(self._h, int(iterations), float(k_color), float(sigma_plane)),
               "mcpt_denoise_resolved_guided")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def denoise_resolved_variance(self, iterations: int = 5, k_color: float = DENOISE_K_VARIANCE,
                                  sigma_plane: float = DENOISE_SIGMA_PLANE) -> np.ndarray:
        """mcpt_denoise_resolved_variance + mcpt_read_denoised: denoise_variance() over the resolved
        colour (adaptive mode on, or a counted gather with its gathered error map)."""
        _check(lib().mcpt_denoise_resolved_variance(self._h, int(iterations), float(k_color), float(sigma_plane)),
               "mcpt_denoise_resolved_variance")
        out = np.zeros((self.n_local_rows, self.W, 3), np.float32)
        _check(lib().mcpt_read_denoised(self._h, _fp(out)), "mcpt_read_denoised")
        return out

    def save_adaptive_checkpoint(self, path: str, next_pass: int, tag: str = "") -> None:
        """mcpt_adaptive_checkpoint_save: the accumulator, the statistics window, the error map and
        the blocks' state of an adaptive render (the mode must be on) to `path`."""
        _check(lib().mcpt_adaptive_checkpoint_save(self._h, str(path).encode(), int(next_pass), tag.encode()),
               "mcpt_adaptive_checkpoint_save")

    def load_adaptive_checkpoint(self, path: str, tag: Optional[str] = None) -> int:
        """mcpt_adaptive_checkpoint_load: resume an adaptive render saved for this target (and, if
        given, with this tag): statistics and the adaptive mode come on in the saved state; returns
        the first pass of the next render call."""
        nxt = ctypes.c_int()
        _check(lib().mcpt_adaptive_checkpoint_load(self._h, str(path).encode(),
                                                   None if tag is None else tag.encode(), ctypes.byref(nxt)),
               "mcpt_adaptive_checkpoint_load")
        return nxt.value

    def gather_rows_counted(self, shards) -> None:
        """mcpt_gather_rows_counted: gather_rows() for shards with per-pixel counts or different pass
        counts; their counts fill this full-frame renderer's count plane (read_sample_counts,
        read_resolved, denoise_resolved).  Every frame row must come from exactly one shard."""
        hs = (_vp * max(len(shards), 1))(*[s._h for s in shards])
        _check(lib().mcpt_gather_rows_counted(self._h, hs, len(shards)), "mcpt_gather_rows_counted")

    # ---- the counted gather across processes (mcpt.h; mcpt.dist.ShardedRenderer)
    def pass_count(self) -> int:
        """mcpt_pass_count: read_accum()'s pass count without the copy or a wait."""
        n = ctypes.c_int()
        _check(lib().mcpt_pass_count(self._h, ctypes.byref(n)), "mcpt_pass_count")
        return n.value

    def pack_counted_device(self, dst_ptr: int, nbytes: int) -> None:
        """mcpt_pack_counted_device: 16-byte records {r, g, b bits, int32 sample count} of the local
        pixels into a device buffer (an int32 torch tensor), on our stream after the queued renders."""
        _check(lib().mcpt_pack_counted_device(self._h, _vp(dst_ptr), ctypes.c_size_t(nbytes)),
               "mcpt_pack_counted_device")

    def load_rows_counted(self, src_ptr: int, src_rows: int, src_row, pass_count: int) -> None:
        """mcpt_load_rows_counted: this full-frame renderer's accumulator and count plane <- packed
        rows on its device, frame row y from packed row src_row[y] (H ints, each < src_rows); leaves
        the state of gather_rows_counted with `pass_count` as the pass count.  Asynchronous."""
        idx = np.ascontiguousarray(src_row, dtype=np.int32)
        if idx.shape != (self.H,):
            raise MCPTError(f"load_rows_counted: expected {self.H} source rows, got {idx.shape}")
        _check(lib().mcpt_load_rows_counted(self._h, _vp(src_ptr), int(src_rows), _ip(idx), int(pass_count)),
               "mcpt_load_rows_counted")

    # ---- the gathered error map: the guided filters on sharded renders (mcpt.h)
    def gather_error_map(self, shards) -> None:
        """mcpt_gather_error_map: this full-frame renderer's gathered error map <- the shard
        renderers' maps (their last convergence() / adaptive_select()), after gather_rows() or
        gather_rows_counted(); denoise_guided / denoise_resolved_guided, read_error_map and
        error_map_record then serve the frame.  Every frame row must come from exactly one shard."""
        hs = (_vp * max(len(shards), 1))(*[s._h for s in shards])
        _check(lib().mcpt_gather_error_map(self._h, hs, len(shards)), "mcpt_gather_error_map")

    def pack_error_map_device(self, dst_ptr: int, nbytes: int) -> None:
        """mcpt_pack_error_map_device: the local pixels' 8-byte {se, r} records into a device buffer
        (an int32 torch tensor: the words travel as bits), on our stream after the queued work."""
        _check(lib().mcpt_pack_error_map_device(self._h, _vp(dst_ptr), ctypes.c_size_t(nbytes)),
               "mcpt_pack_error_map_device")

    def load_rows_error_map(self, src_ptr: int, src_rows: int, src_row) -> None:
        """mcpt_load_rows_error_map: this full-frame renderer's gathered error map <- packed map rows
        on its device, frame row y from packed row src_row[y] (load_rows_counted's index; after the
        load of the rows themselves).  Asynchronous."""
        idx = np.ascontiguousarray(src_row, dtype=np.int32)
        if idx.shape != (self.H,):
            raise MCPTError(f"load_rows_error_map: expected {self.H} source rows, got {idx.shape}")
        _check(lib().mcpt_load_rows_error_map(self._h, _vp(src_ptr), int(src_rows), _ip(idx)),
               "mcpt_load_rows_error_map")

    def error_map_record(self, threshold: float) -> dict:
        """mcpt_error_map_record: convergence()'s record reduced from the stored r values of the map
        this renderer holds (the gathered map, else its own window's).  Synchronizes."""
        rec = Convergence()
        _check(lib().mcpt_error_map_record(self._h, float(threshold), ctypes.byref(rec)), "mcpt_error_map_record")
        return {k: getattr(rec, k) for k, _ in Convergence._fields_}

    def error_map_source(self) -> int:
        """mcpt_error_map_source: 0 no error map, 1 the own window's, 2 the gathered map."""
        s = ctypes.c_int()
        _check(lib().mcpt_error_map_source(self._h, ctypes.byref(s)), "mcpt_error_map_source")
        return s.value

    def trace(self, origins, dirs, any_hit: bool = False, prim: int = -1) -> np.ndarray:
        """Ray queries (traverse_all_bvh / just_hit_bvh, or one primitive) + intersection_info.
        Returns a structured array of HIT_DTYPE records (shape -1 = miss)."""
        o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        if o.shape != d.shape:
            raise ValueError("origins and dirs must have the same shape")
        out = np.zeros(o.shape[0], HIT_DTYPE)
        assert HIT_DTYPE.itemsize == ctypes.sizeof(Hit)
        _check(lib().mcpt_trace(self._h, _fp(o), _fp(d), o.shape[0], int(bool(any_hit)), int(prim),
                                out.ctypes.data_as(_vp)), "mcpt_trace")
        return out

    def sample_hemisphere(self, normal, fseed, n: int, roughness: float = 1.0, nb_used: int = 3) -> np.ndarray:
        """DrawSampling point cloud: n directions random_ray(normalize(normal), roughness)."""
        nrm = _f32(normal, 3)
        sd = _f32(fseed, 3)
        out = np.zeros((int(n), 3), np.float32)
        _check(lib().mcpt_sample_hemisphere(self._h, _fp(nrm), _fp(sd), float(roughness), int(nb_used), int(n),
                                            _fp(out)), "mcpt_sample_hemisphere")
        return out

    def set_traversal(self, mode: int) -> None:
        """BVH traversal strategy: TRAVERSAL_AUTO / _LANE / _WAVE / _STREAM (same results)."""
        _check(lib().mcpt_set_traversal(self._h, int(mode)), "mcpt_set_traversal")

    def set_walk_exit(self, lanes: int) -> None:
        """mcpt_set_walk_exit: suspend per-lane walks at <= lanes walking lanes (-1: default)."""
        _check(lib().mcpt_set_walk_exit(self._h, int(lanes)), "mcpt_set_walk_exit")

    def walk_exit(self) -> int:
        n = ctypes.c_int()
        _check(lib().mcpt_get_walk_exit(self._h, ctypes.byref(n)), "mcpt_get_walk_exit")
        return n.value

    def set_leaf_batch(self, lanes: int) -> None:
        """mcpt_set_leaf_batch: primitive-test block once >= lanes lanes wait on a leaf (-1: default)."""
        _check(lib().mcpt_set_leaf_batch(self._h, int(lanes)), "mcpt_set_leaf_batch")

    def leaf_batch(self) -> int:
        n = ctypes.c_int()
        _check(lib().mcpt_get_leaf_batch(self._h, ctypes.byref(n)), "mcpt_get_leaf_batch")
        return n.value

    def set_stream_pool(self, slots: int = 0, refill: int = -1) -> None:
        """Stream schedule knobs (mcpt_set_stream_pool): path slots (0 = default) and the trace
        kernel's refill threshold (-1 = default).  Same results for every value."""
        _check(lib().mcpt_set_stream_pool(self._h, int(slots), int(refill)), "mcpt_set_stream_pool")

    def stream_iterations(self) -> int:
        """Iterations (trace + shade kernel pairs) of the last stream-schedule launch."""
        n = ctypes.c_longlong()
        _check(lib().mcpt_stream_iterations(self._h, ctypes.byref(n)), "mcpt_stream_iterations")
        return n.value

    def set_partial_budget(self, nbytes: int) -> None:
        """mcpt_set_partial_budget: bound of one launch's segment-sum buffer (calls spanning more
        32-pass chunks are split into launches at chunk boundaries; same bits)."""
        _check(lib().mcpt_set_partial_budget(self._h, int(nbytes)), "mcpt_set_partial_budget")

    def set_render_lanes(self, on: bool) -> None:
        """mcpt_set_render_lanes: consecutive launches on two alternating lanes (overlapping each
        other's tails; the default) or every launch in order on the context's stream."""
        _check(lib().mcpt_set_render_lanes(self._h, int(bool(on))), "mcpt_set_render_lanes")

    def last_launch_count(self) -> int:
        """Sub-launches the last render call was split into."""
        n = ctypes.c_int()
        _check(lib().mcpt_last_launch_count(self._h, ctypes.byref(n)), "mcpt_last_launch_count")
        return n.value

    def last_pass_split(self) -> bool:
        """mcpt_last_pass_split: the last render call ran one segment per pass (small launches;
        same bits)."""
        n = ctypes.c_int()
        _check(lib().mcpt_last_pass_split(self._h, ctypes.byref(n)), "mcpt_last_pass_split")
        return bool(n.value)

    def traversal(self) -> int:
        """The strategy AUTO resolves to for the uploaded scene."""
        m = ctypes.c_int()
        _check(lib().mcpt_get_traversal(self._h, ctypes.byref(m)), "mcpt_get_traversal")
        return m.value

    def schedule(self) -> dict:
        """The schedule of the next launch of the last launch shape (mcpt_get_schedule):
        traversal ("lane"/"wave"/"stream"), pass segments per work item, AUTO settled or not."""
        t, k, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().mcpt_get_schedule(self._h, ctypes.byref(t), ctypes.byref(k), ctypes.byref(s)),
               "mcpt_get_schedule")
        return {"traversal": {1: "lane", 2: "wave", 3: "stream"}.get(t.value, str(t.value)), "seg_per_item": k.value,
                "settled": bool(s.value)}

    def set_stream(self, hip_stream_ptr: int) -> None:
        _check(lib().mcpt_set_stream(self._h, _vp(hip_stream_ptr)), "mcpt_set_stream")

    def synchronize(self) -> None:
        _check(lib().mcpt_synchronize(self._h), "mcpt_synchronize")

    def last_render_ms(self) -> float:
        ms = ctypes.c_float()
        _check(lib().mcpt_last_render_ms(self._h, ctypes.byref(ms)), "mcpt_last_render_ms")
        return ms.value

    def last_kernel_ms(self) -> Tuple[float, float]:
        """(path-tracing kernel ms, chunk-combine kernel ms) of the last render."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)), "mcpt_last_kernel_ms")
        return a.value, b.value

    # render calls whose kernel times a context keeps (mcpt_kernel_ms_back)
    TIMING_RING = 64

    def kernel_span_ms_back(self, back: int) -> float:
        """mcpt_kernel_span_ms_back: the path-tracing kernel's whole span (own start -> end) of the
        call `back` calls before the last; with render lanes the launches overlap, and
        kernel_ms_back charges each its period instead."""
        a = ctypes.c_float()
        _check(lib().mcpt_kernel_span_ms_back(self._h, int(back), ctypes.byref(a)), "mcpt_kernel_span_ms_back")
        return a.value

    def kernel_ms_back(self, back: int) -> Tuple[float, float]:
        """mcpt_kernel_ms_back: (path-tracing ms, combine ms) of the render call `back` calls
        before the last (0: the last; < TIMING_RING); waits for that call only."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().mcpt_kernel_ms_back(self._h, int(back), ctypes.byref(a), ctypes.byref(b)), "mcpt_kernel_ms_back")
        return a.value, b.value

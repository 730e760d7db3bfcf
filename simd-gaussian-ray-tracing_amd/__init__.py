"""MI355X-native volumetric Gaussian ray tracer: Python (ctypes) face of libvrt_hip.so.

The product is the C-ABI shared library built from csrc/ (include/vrt_hip.h); this module is
only the thin binding the tests, bench.py and the smoke entry use.  It mirrors the reference's
operator set for the hot path -- render_image / simd_render_image, radiance, transmittance,
tile_gaussians (reference src/vrt/rt.h, rt.cpp) -- and fails loudly when the HIP library or a
GPU is missing: there is no CPU fallback.

The directory name contains '-', so import it through `load()` in tests/conftest.py /
__graft_entry__.py (importlib by path) under the module name `sgrt_amd`.
"""
import ctypes as C
import mmap
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VRT_HIP_LIB") or os.path.join(_HERE, "lib", "libvrt_hip.so")   # override: A/B builds
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

EXP_LIBM, EXP_VCL, EXP_FAST, EXP_SPLINE = 0, 1, 2, 3
ERF_LIBM, ERF_AS, ERF_SPLINE, ERF_SPLINE_MIRROR, ERF_TAYLOR = 0, 1, 2, 3, 4
GRAD_STRIDE = 12            # VRT_HIP_GRAD_STRIDE: floats per row of a gradient bundle's table
RAY_GRAD_STRIDE = 8         # VRT_HIP_RAY_GRAD_STRIDE: floats per ray row of a gradient bundle's ray output
TGRAD_T, TGRAD_DEPTH = 0, 1 # VRT_HIP_TGRAD_*: what a transmittance gradient bundle's grad_T is the derivative with respect to
TABLE_STEP_DEFAULT = 0.05   # vrt_hip_set_table_step: the library's default (0 = exact kernels only)
PACK_TRUNC, PACK_ROUND, ALPHA_OPAQUE, ALPHA_COMPUTED = 0, 1, 0, 2

_lib = None


class VrtHipError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("tiling_ms", C.c_double), ("rays", C.c_uint64), ("blocks", C.c_uint64),
                ("list_entries", C.c_uint64), ("tile_entries", C.c_uint64), ("overflow_blocks", C.c_uint64),
                ("lane_entries", C.c_uint64), ("lane_max_entries", C.c_uint64), ("shaded_blocks", C.c_uint64), ("dense_blocks", C.c_uint64),
                ("dense_busy_frac", C.c_double), ("table_blocks", C.c_uint64),
                ("lane_pairs", C.c_uint64), ("dense_visits_full", C.c_uint64), ("dense_visits_zero", C.c_uint64),
                ("dense_visits_common", C.c_uint64), ("table_nodes", C.c_uint64), ("table_retries", C.c_uint64),
                ("table_skips", C.c_uint64), ("table_declined", C.c_uint64), ("table_coarser", C.c_uint64), ("table_empty", C.c_uint64), ("table_phase_ticks", C.c_uint64 * 8), ("dense_launch_skips", C.c_uint64)]


class RayStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("rays", "short_rays", "long_rays", "lane_entries", "lane_pairs", "chunks_tested",
                                          "chunks_kept", "members_tested", "scratch_rays")]


class RayIndexStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("indexed", "groups", "leaves", "groups_tested", "groups_kept", "leaves_tested", "leaves_kept",
                                          "members_tested")]


class RaySortStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("sorted", "rays", "rays_without_sphere")]


class GradOrderedStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "gaussians", "longest", "mismatches")]


class RayPlanInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("rays", "entries", "short_rays", "long_rays", "longest", "scratch_rays", "bytes", "sorted", "indexed",
                                          "scene_n", "cull_generation")]


PLAN_KEEP_LISTS = 1         # VRT_HIP_PLAN_KEEP_LISTS: a bound ray plan's lists stay in force across scene updates that keep N
GRAD_RECORD_COLS = 9        # floats per record of an ordered gradient table: the table's columns 0..8


def build(verbose=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-j4", "-C", os.path.join(_HERE, "csrc")], stdout=out)   # the kernel translation units side by side
    return LIB_PATH


# every symbol include/vrt_hip.h declares: (restype, argtypes)
_f32p, _u32p, _vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
SYMBOLS = {
    "vrt_hip_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "vrt_hip_destroy": (None, [_vp]),
    "vrt_hip_last_error": (C.c_char_p, [_vp]),
    "vrt_hip_version": (C.c_char_p, []),
    "vrt_hip_set_gaussians": (C.c_int, [_vp, C.c_size_t] + [_f32p] * 9),
    "vrt_hip_set_gaussians_aos": (C.c_int, [_vp, C.c_size_t, _vp]),
    "vrt_hip_set_gaussians_device": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "vrt_hip_tile_gaussians": (C.c_int, [_vp, C.c_float, C.c_float, _f32p]),
    "vrt_hip_tile_gaussians_device": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _vp]),
    "vrt_hip_set_tiles": (C.c_int, [_vp, C.c_float, C.c_float, C.c_uint64, C.c_uint64, _u32p, _u32p]),
    "vrt_hip_clear_tiles": (C.c_int, [_vp]),
    "vrt_hip_get_tile_counts": (C.c_int, [_vp, _u32p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vrt_hip_get_tile_indices": (C.c_int, [_vp, C.c_uint64, _u32p, C.c_size_t, _u32p]),
    "vrt_hip_set_plane": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p]),
    "vrt_hip_set_camera": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, _f32p, C.c_float]),
    "vrt_hip_set_options": (C.c_int, [_vp, C.c_int, C.c_int, C.c_float]),
    "vrt_hip_render": (C.c_int, [_vp, _f32p, C.c_int, _u32p, _f32p]),
    "vrt_hip_render_device": (C.c_int, [_vp, _f32p, C.c_int, _vp, _vp, _vp]),
    "vrt_hip_frame_device": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp, C.c_int, _vp]),
    "vrt_hip_frame_retained_device": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp, _vp]),
    "vrt_hip_set_shard": (C.c_int, [_vp, C.c_int, C.c_int]),
    "vrt_hip_shard_pixels": (C.c_size_t, [_vp]),
    "vrt_hip_render_shard_device": (C.c_int, [_vp, _f32p, C.c_int, _vp, _vp]),
    "vrt_hip_set_table_step": (C.c_int, [_vp, C.c_float]),
    "vrt_hip_set_table_budget": (C.c_int, [_vp, C.c_float]),
    "vrt_hip_set_cull_prune": (C.c_int, [_vp, C.c_float]),
    "vrt_hip_set_camera_view": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _f32p]),
    "vrt_hip_frame": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp, C.c_int]),
    "vrt_hip_sync": (C.c_int, [_vp]),
    "vrt_hip_host_register": (C.c_int, [_vp, _vp, C.c_size_t]),
    "vrt_hip_host_unregister": (C.c_int, [_vp, _vp]),
    "vrt_hip_frame_host": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp]),
    "vrt_hip_assemble_shards_device": (C.c_int, [_vp, _vp, _vp, _vp]),
    "vrt_hip_assemble_shards_strided_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "vrt_hip_image_pixels": (C.c_size_t, [_vp]),
    "vrt_hip_sparse_shard_words": (C.c_size_t, [_vp]),
    "vrt_hip_frame_sparse_device": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp, _vp]),
    "vrt_hip_frame_batch_device": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _vp, C.c_int, _vp]),
    "vrt_hip_scatter_sparse_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int, _vp, _vp]),
    "vrt_hip_scatter_sparse_retained_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int, _vp, _vp]),
    "vrt_hip_scatter_sparse_batch_device": (C.c_int, [_vp, _vp, C.c_int, C.c_size_t, C.c_int, C.c_int, _vp, C.c_int, _vp]),
    "vrt_hip_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_vp)]),
    "vrt_hip_group_destroy": (None, [_vp]),
    "vrt_hip_group_size": (C.c_int, [_vp]),
    "vrt_hip_group_ctx": (_vp, [_vp, C.c_int]),
    "vrt_hip_group_last_error": (C.c_char_p, [_vp]),
    "vrt_hip_group_frame": (C.c_int, [_vp, C.c_float, C.c_float, _f32p, _f32p, C.c_int, _u32p, C.c_int]),
    "vrt_hip_group_image_device": (_vp, [_vp]),
    "vrt_hip_group_sync": (C.c_int, [_vp]),
    "vrt_hip_group_frame_batch": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, _f32p, _f32p, C.c_int, C.POINTER(C.c_void_p), C.c_int]),
    "vrt_hip_group_batch_image_device": (_vp, [_vp, C.c_int]),
    "vrt_hip_copy_state": (C.c_int, [_vp, _vp]),
    "vrt_hip_state_generation": (C.c_uint64, [_vp]),
    "vrt_hip_get_image_size": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vrt_hip_transmittance": (C.c_int, [_vp, _f32p, _f32p, _f32p, C.c_size_t, _f32p]),
    "vrt_hip_transmittance_rays": (C.c_int, [_vp, C.c_size_t, _f32p, _f32p, _f32p, _f32p]),
    "vrt_hip_radiance": (C.c_int, [_vp, C.c_size_t, _f32p, _f32p, _f32p]),
    "vrt_hip_radiance_rays_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp]),
    "vrt_hip_radiance_rays": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, _u32p, C.c_int]),
    "vrt_hip_transmittance_bundle_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int, _vp, _vp]),
    "vrt_hip_transmittance_bundle": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, C.c_size_t, C.c_int, _f32p]),
    "vrt_hip_depth_bundle_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int, _vp, _vp]),
    "vrt_hip_depth_bundle": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, C.c_size_t, C.c_int, _f32p]),
    "vrt_hip_radiance_rays_grad_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "vrt_hip_radiance_rays_grad": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, _f32p]),
    "vrt_hip_transmittance_bundle_grad_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "vrt_hip_transmittance_bundle_grad": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, C.c_size_t, C.c_int, _f32p, C.c_int, _f32p, _f32p]),
    "vrt_hip_radiance_rays_grad_rays_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "vrt_hip_radiance_rays_grad_rays": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    "vrt_hip_radiance_rays_gn_diag_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "vrt_hip_radiance_rays_gn_diag": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, _f32p]),
    "vrt_hip_radiance_rays_tangent_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "vrt_hip_radiance_rays_tangent": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    "vrt_hip_transmittance_bundle_grad_rays_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int, _vp, _vp, _vp,
                                                                _vp]),
    "vrt_hip_transmittance_bundle_grad_rays": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, C.c_size_t, C.c_int, _f32p, C.c_int, _f32p, _f32p,
                                                         _f32p]),
    "vrt_hip_transmittance_bundle_tangent_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int,
                                                              _vp, _vp]),
    "vrt_hip_transmittance_bundle_tangent": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, _f32p, C.c_size_t, C.c_int, C.c_int, _f32p, _f32p, _f32p,
                                                       C.c_int, _f32p]),
    "vrt_hip_get_ray_stats": (C.c_int, [_vp, C.POINTER(RayStats)]),
    "vrt_hip_set_ray_index": (C.c_int, [_vp, C.c_int]),
    "vrt_hip_get_ray_index_stats": (C.c_int, [_vp, C.POINTER(RayIndexStats)]),
    "vrt_hip_get_ray_index_perm": (C.c_int, [_vp, _u32p, C.c_size_t]),
    "vrt_hip_set_ray_sort": (C.c_int, [_vp, C.c_int]),
    "vrt_hip_get_ray_sort_stats": (C.c_int, [_vp, C.POINTER(RaySortStats)]),
    "vrt_hip_get_ray_order": (C.c_int, [_vp, _u32p, _u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vrt_hip_ray_plan_create_device": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.POINTER(_vp)]),
    "vrt_hip_ray_plan_create": (C.c_int, [_vp, C.c_size_t, _f32p, C.c_int, _f32p, C.POINTER(_vp)]),
    "vrt_hip_ray_plan_destroy": (C.c_int, [_vp, _vp]),
    "vrt_hip_set_ray_plan": (C.c_int, [_vp, _vp, C.c_int]),
    "vrt_hip_get_ray_plan_info": (C.c_int, [_vp, _vp, C.POINTER(RayPlanInfo)]),
    "vrt_hip_get_ray_plan_lists": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), _u32p]),
    "vrt_hip_set_grad_ordered": (C.c_int, [_vp, C.c_int]),
    "vrt_hip_get_grad_records": (C.c_int, [_vp, _u32p, _u32p, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vrt_hip_get_grad_ordered_stats": (C.c_int, [_vp, C.POINTER(GradOrderedStats)]),
    "vrt_hip_transmittance_step": (C.c_int, [_vp, _f32p, _f32p, _f32p, C.c_size_t, C.c_float, _f32p]),
    "vrt_hip_density": (C.c_int, [_vp, C.c_size_t, _f32p, _f32p]),
    "vrt_hip_eval_erf": (C.c_int, [_vp, C.c_int, _f32p, C.c_size_t, _f32p]),
    "vrt_hip_eval_exp": (C.c_int, [_vp, C.c_int, _f32p, C.c_size_t, _f32p]),
    "vrt_hip_camera_init": (None, [_vp, _f32p, _f32p, _f32p, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_float]),
    "vrt_hip_camera_turn": (None, [_vp, C.c_float, C.c_float, C.c_int]),
    "vrt_hip_camera_refresh": (None, [_vp]),
    "vrt_hip_camera_plane": (None, [_vp, _f32p, _f32p, _f32p]),
    "vrt_hip_camera_orbit": (None, [_vp, C.c_float]),
    "vrt_hip_mat4_inverse": (None, [_f32p, _f32p]),
    "vrt_hip_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "vrt_hip_enable_stats": (C.c_int, [_vp, C.c_int]),
    "vrt_hip_enable_kernel_timing": (C.c_int, [_vp, C.c_int]),
    "vrt_hip_get_kernel_timing": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_uint64)]),
}


def lib():
    """dlopen libvrt_hip.so; raises if it has not been built (never falls back to anything)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VrtHipError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950)")
        try:
            # PyTorch ships its own libamdhip64; load it first so the process has ONE HIP runtime
            # (torch is the plumbing for device buffers / streams / RCCL in tests and bench.py)
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(_f32p)


def host_frame(w, h):
    """A host frame buffer for Renderer.register_host: uint32 [h, w] in anonymous memory of its own whole pages (page
    aligned, so two registrations never share a page).  The array keeps its memory alive."""
    mm = mmap.mmap(-1, max(1, int(w) * int(h)) * 4)
    return np.frombuffer(mm, np.uint32, count=int(w) * int(h)).reshape(int(h), int(w))


def _f3(v):
    return np.ascontiguousarray(np.asarray(v, np.float32)[:3])


def _rays(origins, dirs):
    """The rays of a bundle as the library takes them: origins f32 [3] (one for the bundle) or [nrays, 3], dirs f32 [nrays, 3], and
    whether there is an origin per ray."""
    origins = np.ascontiguousarray(origins, np.float32)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    per_ray = origins.size != 3
    if per_ray:
        assert origins.size == dirs.size
    return origins, dirs, per_ray


def _table(v, nrays, per_ray):
    """A bundle's table of values, [n] for every ray or [nrays, n] per ray (per_ray says which when the shape does not): the array
    f32, the values per ray, and whether they are per ray."""
    v = np.ascontiguousarray(v, np.float32)
    if per_ray is None:
        per_ray = v.ndim == 2
    n = v.size // nrays if per_ray and nrays else v.size
    if per_ray:
        assert v.size == nrays * n
    return v, n, bool(per_ray)


def grad_columns(table):
    """The columns of a gradient bundle's table [N, GRAD_STRIDE] (numpy array or torch tensor) by name: views, not copies."""
    return {"albedo": table[:, 0:4], "mu": table[:, 4:7], "sigma": table[:, 7], "magnitude": table[:, 8]}


def ray_grad_columns(rows):
    """The columns of a gradient bundle's ray rows [nrays, RAY_GRAD_STRIDE] (numpy array or torch tensor) by name: views, not copies.
    "origin": d(loss) / d(origin) per ray (a bundle with one origin: sum them over the rays); "dir": the tangential d(loss) / d(dir)."""
    return {"origin": rows[:, 0:3], "dir": rows[:, 4:7]}


def _pack_tangent(tangent, n):
    """A tangent bundle's direction in the Gaussians as the library takes it, f32 [n, GRAD_STRIDE]: from the dict grad_columns makes (a
    missing key: zeros) or from a packed array."""
    if not isinstance(tangent, dict):
        t = np.ascontiguousarray(tangent, np.float32)
        assert t.shape == (n, GRAD_STRIDE), t.shape
        return t
    t = np.zeros((n, GRAD_STRIDE), np.float32)
    cols = grad_columns(t)
    for k, v in tangent.items():
        cols[k][...] = np.asarray(v, np.float32).reshape(cols[k].shape)
    return t


def _pack_ray_tangent(ray_tangent, nrays):
    """... and in the rays, f32 [nrays, RAY_GRAD_STRIDE]: from the dict ray_grad_columns makes (a missing key: zeros; an "origin" of
    [3] moves every ray's origin alike) or from a packed array."""
    if not isinstance(ray_tangent, dict):
        t = np.ascontiguousarray(ray_tangent, np.float32)
        assert t.shape == (nrays, RAY_GRAD_STRIDE), t.shape
        return t
    t = np.zeros((nrays, RAY_GRAD_STRIDE), np.float32)
    cols = ray_grad_columns(t)
    for k, v in ray_tangent.items():
        v = np.asarray(v, np.float32)
        cols[k][...] = v.reshape(1, 3) if v.size == 3 else v.reshape(nrays, 3)
    return t


class RayPlan:
    """A ray plan (Renderer.ray_plan / ray_plan_device): the kept lists of one bundle, culled once and held in device memory.  Bind it
    with Renderer.set_ray_plan or `with renderer.using(plan):` and every bundle call takes its lists from it: see "Ray plans" in
    include/vrt_hip.h.  Belongs to its renderer; close() (or the renderer's) frees it."""

    def __init__(self, renderer, handle):
        self._r, self._p = renderer, handle

    def info(self):
        """rays, entries, short_rays, long_rays, longest, scratch_rays, bytes, sorted, indexed, scene_n, cull_generation: see
        vrt_hip_ray_plan_info in include/vrt_hip.h."""
        s = RayPlanInfo()
        self._r._chk(self._r._L.vrt_hip_get_ray_plan_info(self._r._h, self._p, C.byref(s)), "get_ray_plan_info")
        return {k: getattr(s, k) for k, _ in RayPlanInfo._fields_}

    def lists(self):
        """(offsets u64 [nrays + 1], entries u32 [info()["entries"]]): ray r, at the caller's index, keeps entries[offsets[r]:offsets[r + 1]],
        scene indices in ascending order."""
        i = self.info()
        offsets, entries = np.zeros(i["rays"] + 1, np.uint64), np.zeros(max(i["entries"], 1), np.uint32)
        self._r._chk(self._r._L.vrt_hip_get_ray_plan_lists(self._r._h, self._p, offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                           entries.ctypes.data_as(_u32p)), "get_ray_plan_lists")
        return offsets, entries[:i["entries"]]

    def close(self):
        """Frees the plan; the bound plan is unbound first.  Waits for bundles in flight."""
        if getattr(self, "_p", None) and getattr(self._r, "_h", None):
            self._r._L.vrt_hip_ray_plan_destroy(self._r._h, self._p)
            if self._r._plan[0] is self:
                self._r._plan = (None, False)
        self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _UsingPlan:
    """`with renderer.using(plan):` -- binds the plan, and puts the binding that was there back on the way out."""

    def __init__(self, renderer, plan, keep_lists):
        self._r, self._new = renderer, (plan, keep_lists)

    def __enter__(self):
        self._old = self._r._plan
        self._r.set_ray_plan(*self._new)
        return self._new[0]

    def __exit__(self, *exc):
        old, keep = self._old
        if old is not None and old._p is None:   # closed meanwhile
            old = None
        self._r.set_ray_plan(old, keep)
        return False


class Renderer:
    """One context = one GPU.  Mirrors the reference call set (main.cpp:257-296)."""

    def __init__(self, device=0, _handle=None):
        self._L = lib()
        self._owned = _handle is None
        if _handle is None:
            h = _vp()
            rc = self._L.vrt_hip_create(device, C.byref(h))
            if rc != 0:
                raise VrtHipError(f"vrt_hip_create({device}) failed ({rc}): {self._L.vrt_hip_last_error(None).decode()}")
            _handle = h
        self._h = _handle
        self.device = device if self._owned else None   # the HIP device of a context made here (a group's members: not known)
        self._host = {}   # registered host buffers by address: kept alive while the GPU may write them
        self._plan = (None, False)   # the bound RayPlan and its keep_lists
        self.n = 0
        self.w = self.h = 0
        self.table_step = float(os.environ.get("VRT_HIP_TABLE_STEP", TABLE_STEP_DEFAULT))

    def close(self):
        if getattr(self, "_h", None):
            for addr in list(self._host):   # each waits for the frames in flight, then unregisters (destroy would too)
                self._L.vrt_hip_host_unregister(self._h, addr)
            if self._owned:
                self._L.vrt_hip_destroy(self._h)
            self._h = None
            self._host.clear()              # no frame of this context can write the arrays any more

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise VrtHipError(f"{what} failed ({rc}): {self._L.vrt_hip_last_error(self._h).decode()}")

    def _device(self, what, nrays, d_origins, origin_per_ray, d_dirs, *rest):
        """vrt_hip_<what>, the device form of a ray bundle: the rays, then the kind's own arguments as ctypes takes them, the stream last."""
        rc = getattr(self._L, "vrt_hip_" + what)(self._h, int(nrays), d_origins or None, int(bool(origin_per_ray)), d_dirs or None, *rest)
        if rc != 0:
            self._chk(rc, what)

    # ---- scene ----
    def set_gaussians(self, g):
        """g: structured array with fields albedo[4], mu[4], sigma, magnitude (gaussian_t, types.h:195-200)."""
        g = np.ascontiguousarray(g)
        assert g.dtype.itemsize == 40
        self.n = len(g)
        self._chk(self._L.vrt_hip_set_gaussians_aos(self._h, len(g), g.ctypes.data), "set_gaussians_aos")

    def set_gaussians_soa(self, mu, albedo, sigma, magnitude, alpha=None):
        mu = np.asarray(mu, np.float32)
        albedo = np.asarray(albedo, np.float32)
        cols = [np.ascontiguousarray(mu[:, i]) for i in range(3)] + [np.ascontiguousarray(albedo[:, i]) for i in range(3)]
        a = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
        s = np.ascontiguousarray(sigma, np.float32)
        m = np.ascontiguousarray(magnitude, np.float32)
        self.n = len(s)
        self._chk(self._L.vrt_hip_set_gaussians(self._h, len(s), *[_fp(c) for c in cols], None if a is None else _fp(a),
                                                _fp(s), _fp(m)), "set_gaussians")

    def set_gaussians_device(self, n, d_mu, d_albedo, d_sigma, d_magnitude, stream=0):
        """vrt_hip_set_gaussians_device: the scene from device pointers (mu [n, 3], albedo [n, 4] with alpha in column 3, sigma [n],
        magnitude [n], float32, packed), everything enqueued on `stream` and nothing waited for: the same scene, bit for bit, as
        set_gaussians_soa(..., alpha=...) of the same values."""
        self._chk(self._L.vrt_hip_set_gaussians_device(self._h, int(n), d_mu or None, d_albedo or None, d_sigma or None, d_magnitude or None,
                                                       stream or None), "set_gaussians_device")
        self.n = int(n)

    # ---- tiles ----
    def tile_gaussians(self, tw, th, view):
        v = np.ascontiguousarray(view, np.float32).ravel()
        assert v.size == 16
        self._chk(self._L.vrt_hip_tile_gaussians(self._h, tw, th, _fp(v)), "tile_gaussians")

    def tile_gaussians_device(self, tw, th, view, stream=0):
        v = np.ascontiguousarray(view, np.float32).ravel()
        self._chk(self._L.vrt_hip_tile_gaussians_device(self._h, tw, th, _fp(v), stream or None), "tile_gaussians_device")

    def set_tiles(self, tiles):
        off = np.ascontiguousarray(tiles["offsets"], np.uint32)
        idx = np.ascontiguousarray(tiles["indices"], np.uint32)
        self._chk(self._L.vrt_hip_set_tiles(self._h, float(tiles["tw"]), float(tiles["th"]), int(tiles["w"]),
                                            int(tiles["h"]), off.ctypes.data_as(_u32p),
                                            idx.ctypes.data_as(_u32p) if idx.size else None), "set_tiles")

    def clear_tiles(self):
        self._chk(self._L.vrt_hip_clear_tiles(self._h), "clear_tiles")

    def tile_counts(self):
        tw, th = C.c_uint64(), C.c_uint64()
        self._chk(self._L.vrt_hip_get_tile_counts(self._h, None, 0, C.byref(tw), C.byref(th)), "get_tile_counts")
        counts = np.zeros(tw.value * th.value, np.uint32)
        self._chk(self._L.vrt_hip_get_tile_counts(self._h, counts.ctypes.data_as(_u32p), counts.size, None, None),
                  "get_tile_counts")
        return counts.reshape(th.value, tw.value)

    def tile_indices(self, t):
        cnt = C.c_uint32()
        self._chk(self._L.vrt_hip_get_tile_indices(self._h, t, None, 0, C.byref(cnt)), "get_tile_indices")
        out = np.zeros(max(cnt.value, 1), np.uint32)
        self._chk(self._L.vrt_hip_get_tile_indices(self._h, t, out.ctypes.data_as(_u32p), out.size, C.byref(cnt)),
                  "get_tile_indices")
        return out[:cnt.value]

    # ---- rays ----
    def set_plane(self, w, h, xs, ys, zs):
        xs, ys, zs = (np.ascontiguousarray(a, np.float32) for a in (xs, ys, zs))
        assert xs.size == ys.size == zs.size == w * h
        self.w, self.h = w, h
        self._chk(self._L.vrt_hip_set_plane(self._h, w, h, _fp(xs), _fp(ys), _fp(zs)), "set_plane")

    def set_camera(self, w, h, pos, right, up, front, focal=1.0):
        self.w, self.h = w, h
        self._chk(self._L.vrt_hip_set_camera(self._h, w, h, _fp(_f3(pos)), _fp(_f3(right)), _fp(_f3(up)),
                                             _fp(_f3(front)), focal), "set_camera")

    def set_camera_view(self, w, h, view):
        """In-kernel rays that are bit for bit the reference's: plane point = inverse(view) * (x, y, 0, 1)."""
        self.w, self.h = w, h
        v = np.ascontiguousarray(np.asarray(view, np.float32).reshape(16))
        self._chk(self._L.vrt_hip_set_camera_view(self._h, w, h, _fp(v)), "set_camera_view")

    def set_options(self, exp_kind=EXP_VCL, erf_kind=ERF_AS, cull_eps=1e-9):
        self._chk(self._L.vrt_hip_set_options(self._h, exp_kind, erf_kind, cull_eps), "set_options")

    # ---- render ----
    def render(self, origin, pack=PACK_ROUND | ALPHA_COMPUTED, want_radiance=True):
        """Returns (image u32 [h,w], radiance f32 [h,w,4] or None)."""
        img = np.zeros(self.w * self.h, np.uint32)
        rad = np.zeros((self.w * self.h, 4), np.float32) if want_radiance else None
        self._chk(self._L.vrt_hip_render(self._h, _fp(_f3(origin)), pack, img.ctypes.data_as(_u32p),
                                         _fp(rad) if rad is not None else None), "render")
        return img.reshape(self.h, self.w), (rad.reshape(self.h, self.w, 4) if rad is not None else None)

    def render_device(self, origin, pack, d_image, d_radiance=0, stream=0):
        self._chk(self._L.vrt_hip_render_device(self._h, _fp(_f3(origin)), pack, d_image, d_radiance or None,
                                                stream or None), "render_device")

    def frame_call(self, tw, th, view, origin, pack, shard=False, retained=False):
        """Pre-marshalled per-frame call (tile_gaussians + render in ONE C call): returns f(d_out, stream).
        The argument arrays are converted once, so an animation loop pays ~1 us of Python per frame.
        retained: vrt_hip_frame_retained_device -- the caller promises that d_out still holds this context's previous frame."""
        v = np.ascontiguousarray(view, np.float32).ravel().copy()
        o = _f3(origin).copy()
        fn, h, vp, op = self._L.vrt_hip_frame_device, self._h, _fp(v), _fp(o)
        tw, th, pack, shard = float(tw), float(th), int(pack), int(bool(shard))
        if retained:
            fnr = self._L.vrt_hip_frame_retained_device

            def call_retained(d_out, stream=0, _keep=(v, o)):
                rc = fnr(h, tw, th, vp, op, pack, d_out, stream or None)
                if rc != 0:
                    self._chk(rc, "frame_retained_device")
            return call_retained

        def call(d_out, stream=0, _keep=(v, o)):
            rc = fn(h, tw, th, vp, op, pack, d_out, shard, stream or None)
            if rc != 0:
                self._chk(rc, "frame_device")
        return call

    def frame_view_call(self, tw, th, view, origin, pack):
        """Like frame_call for a frame loop whose camera MOVES: sets the in-kernel rays of `view` (vrt_hip_set_camera_view)
        and renders the frame, two C calls behind one pre-marshalled Python call: returns f(d_out, stream)."""
        v = np.ascontiguousarray(view, np.float32).ravel().copy()
        o = _f3(origin).copy()
        setv, fn, h, vp, op = self._L.vrt_hip_set_camera_view, self._L.vrt_hip_frame_device, self._h, _fp(v), _fp(o)
        tw, th, pack, w_, h_ = float(tw), float(th), int(pack), int(self.w), int(self.h)

        def call(d_out, stream=0, _keep=(v, o)):
            rc = setv(h, w_, h_, vp)
            if rc == 0:
                rc = fn(h, tw, th, vp, op, pack, d_out, 0, stream or None)
            if rc != 0:
                self._chk(rc, "frame_device")
        return call

    def frame(self, tw, th, view, origin, pack, want_image=True, wait=True):
        """vrt_hip_frame: tile_gaussians + render on the context's own stream and buffer (what the CLI calls)."""
        v = np.ascontiguousarray(view, np.float32).ravel()
        img = np.zeros(self.w * self.h, np.uint32) if want_image else None
        self._chk(self._L.vrt_hip_frame(self._h, float(tw), float(th), _fp(v), _fp(_f3(origin)), int(pack),
                                        img.ctypes.data if want_image else None, int(wait)), "frame")
        return img.reshape(self.h, self.w) if want_image else None

    def sync(self):
        self._chk(self._L.vrt_hip_sync(self._h), "sync")

    # ---- host frames (a frame buffer in host memory, registered once) ----
    def register_host(self, arr):
        """vrt_hip_host_register: `arr` (uint32, C-contiguous; host_frame() makes one) becomes a delivery target of this
        context.  The Renderer holds a reference to it until unregister_host / close."""
        if not isinstance(arr, np.ndarray) or arr.dtype != np.uint32 or not arr.flags.c_contiguous:
            raise VrtHipError("register_host: a C-contiguous uint32 array is required")
        addr = arr.ctypes.data
        self._chk(self._L.vrt_hip_host_register(self._h, addr, arr.size), "host_register")
        self._host[addr] = arr

    def unregister_host(self, arr):
        """vrt_hip_host_unregister: returns once every frame in flight has landed."""
        addr = arr.ctypes.data
        self._chk(self._L.vrt_hip_host_unregister(self._h, addr), "host_unregister")
        self._host.pop(addr, None)

    def frame_host(self, tw, th, view, origin, pack, arr):
        """vrt_hip_frame_host: the frame of frame() delivered into the registered array `arr`; enqueues only, sync() waits.
        Afterwards arr.reshape(-1)[:w*h] holds the frame."""
        v = np.ascontiguousarray(view, np.float32).ravel()
        self._chk(self._L.vrt_hip_frame_host(self._h, float(tw), float(th), _fp(v), _fp(_f3(origin)), int(pack), arr.ctypes.data),
                  "frame_host")

    def set_shard(self, rank, world):
        self._chk(self._L.vrt_hip_set_shard(self._h, rank, world), "set_shard")

    def shard_pixels(self):
        return self._L.vrt_hip_shard_pixels(self._h)

    def render_shard_device(self, origin, pack, d_shard, stream=0):
        self._chk(self._L.vrt_hip_render_shard_device(self._h, _fp(_f3(origin)), pack, d_shard, stream or None),
                  "render_shard_device")

    # ---- sparse shards (only the non-empty 32x32 cells travel) ----
    def sparse_shard_words(self):
        return self._L.vrt_hip_sparse_shard_words(self._h)

    def frame_sparse_call(self, tw, th, view, origin, pack):
        """Pre-marshalled vrt_hip_frame_sparse_device: returns f(d_sparse, stream)."""
        v = np.ascontiguousarray(view, np.float32).ravel().copy()
        o = _f3(origin).copy()
        fn, h, vp, op = self._L.vrt_hip_frame_sparse_device, self._h, _fp(v), _fp(o)
        tw, th, pack = float(tw), float(th), int(pack)

        def call(d_sparse, stream=0, _keep=(v, o)):
            rc = fn(h, tw, th, vp, op, pack, d_sparse, stream or None)
            if rc != 0:
                self._chk(rc, "frame_sparse_device")
        return call

    def frame_batch_call(self, others, tw, th, views, origins, pack, out_kind=0):
        """Pre-marshalled vrt_hip_frame_batch_device: frame i of a batch is rendered by (self, *others)[i] with views[i],
        origins[i]; returns f(out_ptrs, stream, n=None) -- the first n frames into the device pointers out_ptrs[i]
        (out_kind 0: raster frames, 1: compact shards, 2: sparse shards), every kernel launched once for all of them."""
        ctxs = [self, *others]
        v = np.ascontiguousarray(views, np.float32).reshape(len(ctxs), 16).copy()
        o = np.ascontiguousarray(origins, np.float32).reshape(len(ctxs), 3).copy()
        harr = (_vp * len(ctxs))(*[c_._h.value for c_ in ctxs])
        fn, vp, op = self._L.vrt_hip_frame_batch_device, _fp(v), _fp(o)
        tw, th, pack, out_kind = float(tw), float(th), int(pack), int(out_kind)

        def call(out_ptrs, stream=0, n=None, _keep=(v, o, ctxs)):
            n = len(ctxs) if n is None else int(n)
            outs = (_vp * n)(*[int(p_) for p_ in out_ptrs[:n]])
            rc = fn(harr, n, tw, th, vp, op, pack, outs, out_kind, stream or None)
            if rc != 0:
                self._chk(rc, "frame_batch_device")
        return call

    def scatter_sparse_device(self, shard_ptrs, pack, d_image, stream=0, retained=False):
        """Background + every stored cell of every shard (device pointers readable from this context's GPU).  retained:
        d_image still holds this context's previous retained assembly -- only cells that went dark are reset."""
        arr = (_vp * len(shard_ptrs))(*[int(p) for p in shard_ptrs])
        fn = self._L.vrt_hip_scatter_sparse_retained_device if retained else self._L.vrt_hip_scatter_sparse_device
        self._chk(fn(self._h, arr, len(shard_ptrs), int(pack), d_image, stream or None), "scatter_sparse_device")

    def scatter_sparse_batch_device(self, shard_ptrs, frame_stride_words, nframes, pack, image_ptrs, stream=0, retained=False):
        """vrt_hip_scatter_sparse_batch_device: frame f from shard s at shard_ptrs[s] + 4 * f * frame_stride_words bytes into
        image_ptrs[f], all frames in one launch."""
        arr = (_vp * len(shard_ptrs))(*[int(p) for p in shard_ptrs])
        imgs = (_vp * nframes)(*[int(p) for p in image_ptrs[:nframes]])
        self._chk(self._L.vrt_hip_scatter_sparse_batch_device(self._h, arr, len(shard_ptrs), int(frame_stride_words), int(nframes), int(pack),
                                                              imgs, int(bool(retained)), stream or None), "scatter_sparse_batch_device")

    def assemble_shards_device(self, d_gathered, d_image, stream=0, rank_stride_px=None):
        """Scatter a rank-major gather result into raster order; rank_stride_px > shard_pixels() when the gather
        carried several frames per rank (d_gathered then points at the frame's slice of rank 0)."""
        if rank_stride_px is None:
            rc = self._L.vrt_hip_assemble_shards_device(self._h, d_gathered, d_image, stream or None)
        else:
            rc = self._L.vrt_hip_assemble_shards_strided_device(self._h, d_gathered, rank_stride_px, d_image, stream or None)
        self._chk(rc, "assemble_shards_device")

    # ---- point queries ----
    def transmittance(self, o, n, s):
        s = np.ascontiguousarray(np.atleast_1d(s), np.float32)
        out = np.zeros_like(s)
        self._chk(self._L.vrt_hip_transmittance(self._h, _fp(_f3(o)), _fp(_f3(n)), _fp(s), s.size, _fp(out)),
                  "transmittance")
        return out

    def transmittance_rays(self, origins, dirs, s):
        """broadcast_transmittance (rt.h:102-127): one sample point per ray."""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(s, np.float32).ravel()
        assert len(origins) == len(dirs) == s.size
        out = np.zeros_like(s)
        self._chk(self._L.vrt_hip_transmittance_rays(self._h, s.size, _fp(origins), _fp(dirs), _fp(s), _fp(out)),
                  "transmittance_rays")
        return out

    def transmittance_step(self, o, n, s, delta):
        s = np.ascontiguousarray(np.atleast_1d(s), np.float32)
        out = np.zeros_like(s)
        self._chk(self._L.vrt_hip_transmittance_step(self._h, _fp(_f3(o)), _fp(_f3(n)), _fp(s), s.size, delta,
                                                     _fp(out)), "transmittance_step")
        return out

    def density(self, pts):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        out = np.zeros(len(pts), np.float32)
        self._chk(self._L.vrt_hip_density(self._h, len(pts), _fp(pts), _fp(out)), "density")
        return out

    def radiance(self, origins, dirs):
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((len(dirs), 4), np.float32)
        self._chk(self._L.vrt_hip_radiance(self._h, len(dirs), _fp(origins), _fp(dirs), _fp(out)), "radiance")
        return out

    # ---- ray bundles (any rays, culled per ray) ----
    def radiance_rays(self, origins, dirs, want_image=False, pack=PACK_ROUND | ALPHA_COMPUTED):
        """vrt_hip_radiance_rays: origins [3] (one for the bundle) or [nrays, 3], dirs [nrays, 3] unit length.  Returns the
        radiance f32 [nrays, 4], or (radiance, packed pixels u32 [nrays]) with want_image."""
        origins, dirs, per_ray = _rays(origins, dirs)
        rad = np.zeros((len(dirs), 4), np.float32)
        img = np.zeros(len(dirs), np.uint32) if want_image else None
        self._chk(self._L.vrt_hip_radiance_rays(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), _fp(rad),
                                                img.ctypes.data_as(_u32p) if want_image else None, int(pack)), "radiance_rays")
        return (rad, img) if want_image else rad

    def radiance_rays_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_radiance=0, d_image=0, pack=PACK_ROUND | ALPHA_COMPUTED,
                             stream=0):
        """vrt_hip_radiance_rays_device: device pointers, everything enqueued on `stream`."""
        self._device("radiance_rays_device", nrays, d_origins, origin_per_ray, d_dirs, d_radiance or None, d_image or None, int(pack),
                     stream or None)

    def _profile(self, what, origins, dirs, table, table_per_ray):
        """vrt_hip_<what>: a table of values, shared or per ray, in; a result f32 [nrays, values per ray] out."""
        origins, dirs, per_ray = _rays(origins, dirs)
        table, n, table_per_ray = _table(table, len(dirs), table_per_ray)
        out = np.zeros((len(dirs), n), np.float32)
        self._chk(getattr(self._L, "vrt_hip_" + what)(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), _fp(table), n, int(table_per_ray),
                                                      _fp(out)), what)
        return out

    def transmittance_bundle(self, origins, dirs, s, s_per_ray=None):
        """vrt_hip_transmittance_bundle: T at sample distances along the rays, culled per ray like radiance_rays.  origins [3] (one for
        the bundle) or [nrays, 3], dirs [nrays, 3] unit length; s [ns] (the same samples for every ray) or [nrays, ns] (per ray;
        s_per_ray says which when the shape does not).  Returns T f32 [nrays, ns]."""
        return self._profile("transmittance_bundle", origins, dirs, s, s_per_ray)

    def transmittance_bundle_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_s, ns, s_per_ray, d_T, stream=0):
        """vrt_hip_transmittance_bundle_device: device pointers, everything enqueued on `stream`."""
        self._device("transmittance_bundle_device", nrays, d_origins, origin_per_ray, d_dirs, d_s or None, int(ns), int(bool(s_per_ray)),
                     d_T or None, stream or None)

    def depth_bundle(self, origins, dirs, tau, tau_per_ray=None):
        """vrt_hip_depth_bundle: the distance along each ray at which its transmittance falls to the levels tau -- 0 where it starts at
        or below a level, +inf where it never gets there (include/vrt_hip.h has the contract).  origins [3] (one for the bundle) or
        [nrays, 3], dirs [nrays, 3] unit length; tau [nt] (the same levels for every ray) or [nrays, nt] (per ray; tau_per_ray says
        which when the shape does not).  Returns the depths f32 [nrays, nt]."""
        return self._profile("depth_bundle", origins, dirs, tau, tau_per_ray)

    def depth_bundle_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_tau, nt, tau_per_ray, d_depth, stream=0):
        """vrt_hip_depth_bundle_device: device pointers, everything enqueued on `stream`."""
        self._device("depth_bundle_device", nrays, d_origins, origin_per_ray, d_dirs, d_tau or None, int(nt), int(bool(tau_per_ray)),
                     d_depth or None, stream or None)

    def radiance_rays_grad(self, origins, dirs, grad_radiance, want_table=True, want_rays=False):
        """vrt_hip_radiance_rays_grad_rays: the derivative of a loss with respect to the Gaussians and, with want_rays, to the rays,
        given its derivative grad_radiance [nrays, 4] with respect to what radiance_rays returns for the same rays (each ray's kept
        list is held fixed).
        Returns {"albedo": [N, 4], "mu": [N, 3], "sigma": [N], "magnitude": [N]}, float32.  The sums are float atomics on the device:
        not bitwise reproducible, unless set_grad_ordered is on.  With want_rays: (that dict, or None without want_table, {"origin": [nrays, 3], "dir": [nrays, 3]})
        -- per ray d(loss) / d(origin) and the tangential d(loss) / d(dir), bitwise reproducible; without the table no atomic add is
        issued at all."""
        origins, dirs, per_ray = _rays(origins, dirs)
        g = np.ascontiguousarray(grad_radiance, np.float32).reshape(-1, 4)
        assert len(g) == len(dirs)
        out = np.zeros((self.n, GRAD_STRIDE), np.float32) if want_table else None
        rows = np.zeros((len(dirs), RAY_GRAD_STRIDE), np.float32) if want_rays else None
        self._chk(self._L.vrt_hip_radiance_rays_grad_rays(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), _fp(g),
                                                          _fp(out) if want_table else None, _fp(rows) if want_rays else None),
                  "radiance_rays_grad")
        table = grad_columns(out) if want_table else None
        return (table, ray_grad_columns(rows)) if want_rays else table

    def radiance_rays_grad_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_grad_radiance, d_grad, stream=0):
        """vrt_hip_radiance_rays_grad_device: device pointers, everything enqueued on `stream`; ADDS into d_grad ([N, GRAD_STRIDE]
        float32: grad_columns names its columns)."""
        self._device("radiance_rays_grad_device", nrays, d_origins, origin_per_ray, d_dirs, d_grad_radiance or None, d_grad or None,
                     stream or None)

    def radiance_rays_grad_rays_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_grad_radiance, d_grad=0, d_grad_rays=0, stream=0):
        """vrt_hip_radiance_rays_grad_rays_device: as radiance_rays_grad_device, and STORES d_grad_rays ([nrays, RAY_GRAD_STRIDE]
        float32, 16-byte aligned: ray_grad_columns names its columns); either may be 0, not both."""
        self._device("radiance_rays_grad_rays_device", nrays, d_origins, origin_per_ray, d_dirs, d_grad_radiance or None, d_grad or None,
                     d_grad_rays or None, stream or None)

    def radiance_rays_tangent(self, origins, dirs, tangent=None, ray_tangent=None):
        """vrt_hip_radiance_rays_tangent: forward mode, J . v -- how what radiance_rays returns for the same rays moves along a direction
        in parameter space (each ray's kept list is held fixed).  tangent: the direction's part in the Gaussians, the dict grad_columns
        makes ({"albedo": [N, 4], "mu": [N, 3], "sigma": [N], "magnitude": [N]}, a missing key: zeros) or a packed [N, GRAD_STRIDE] array
        (columns 9..11 are never read); ray_tangent: its part in the rays, the dict ray_grad_columns makes ({"origin": [nrays, 3] or [3]
        for every ray, "dir": [nrays, 3]}, a missing key: zeros) or a packed [nrays, RAY_GRAD_STRIDE] array; of "dir" only the part
        perpendicular to the ray's direction counts.  Either may be None (zero), not both.  Returns float32 [nrays, 4], stored without
        atomic adds: bitwise reproducible."""
        origins, dirs, per_ray = _rays(origins, dirs)
        t = None if tangent is None else _pack_tangent(tangent, self.n)
        rt = None if ray_tangent is None else _pack_ray_tangent(ray_tangent, len(dirs))
        out = np.zeros((len(dirs), 4), np.float32)
        self._chk(self._L.vrt_hip_radiance_rays_tangent(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), None if t is None else _fp(t),
                                                        None if rt is None else _fp(rt), _fp(out)), "radiance_rays_tangent")
        return out

    def radiance_rays_tangent_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_tangent=0, d_ray_tangent=0, d_out=0, stream=0):
        """vrt_hip_radiance_rays_tangent_device: device pointers, everything enqueued on `stream`; reads d_tangent ([N, GRAD_STRIDE]
        float32) and d_ray_tangent ([nrays, RAY_GRAD_STRIDE] float32), either may be 0, not both, and STORES d_out ([nrays, 4] float32);
        all three 16-byte aligned."""
        self._device("radiance_rays_tangent_device", nrays, d_origins, origin_per_ray, d_dirs, d_tangent or None, d_ray_tangent or None,
                     d_out or None, stream or None)

    def radiance_rays_gn_diag(self, origins, dirs, weights=None):
        """vrt_hip_radiance_rays_gn_diag: the diagonal of the Gauss-Newton matrix J^T W J of what radiance_rays returns for the same
        rays (each ray's kept list is held fixed): per parameter the sum over rays and channels of weights[r, c] times the squared
        derivative of channel c of ray r.  weights [nrays, 4] or None (all 1).  Returns float32 [N, GRAD_STRIDE] in the gradient table's
        layout (grad_columns splits it); float atomics on the device, bitwise reproducible with set_grad_ordered on."""
        origins, dirs, per_ray = _rays(origins, dirs)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
        assert w is None or len(w) == len(dirs)
        out = np.zeros((self.n, GRAD_STRIDE), np.float32)
        self._chk(self._L.vrt_hip_radiance_rays_gn_diag(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), None if w is None else _fp(w),
                                                        _fp(out)), "radiance_rays_gn_diag")
        return out

    def radiance_rays_gn_diag_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_weights=0, d_diag=0, stream=0):
        """vrt_hip_radiance_rays_gn_diag_device: device pointers, everything enqueued on `stream`; reads d_weights ([nrays, 4] float32,
        16-byte aligned, or 0: all 1) and ADDS into d_diag ([N, GRAD_STRIDE] float32: grad_columns names its columns)."""
        self._device("radiance_rays_gn_diag_device", nrays, d_origins, origin_per_ray, d_dirs, d_weights or None, d_diag or None, stream or None)

    def transmittance_bundle_grad(self, origins, dirs, s, grad_T, wrt=TGRAD_T, s_per_ray=None, want_table=True, want_grad_s=True, want_rays=False):
        """vrt_hip_transmittance_bundle_grad_rays: the derivative of a loss with respect to the Gaussians and the samples, given its
        derivative grad_T [nrays, ns] with respect to what transmittance_bundle returns for the same rays and samples s (wrt = TGRAD_T)
        -- or, with wrt = TGRAD_DEPTH, s [nrays, ns] the depths depth_bundle returned and grad_T the derivative with respect to them:
        the derivative with respect to the Gaussians and the levels tau (of the ideal crossing; a depth of +inf, 0 or NaN contributes
        nothing).  A sample with grad_T == 0 is skipped exactly.  Each ray's kept list is held fixed.
        Returns ({"albedo": zeros [N, 4], "mu": [N, 3], "sigma": [N], "magnitude": [N]} or None, grad_s [nrays, ns] or None), float32.
        The table's sums are float atomics on the device: not bitwise reproducible, unless set_grad_ordered is on.  With want_rays a third value follows:
        {"origin": [nrays, 3], "dir": [nrays, 3]}, per ray d(loss) / d(origin) and the tangential d(loss) / d(dir), bitwise reproducible."""
        origins, dirs, per_ray = _rays(origins, dirs)
        s, ns, s_per_ray = _table(s, len(dirs), s_per_ray)
        g = np.ascontiguousarray(grad_T, np.float32)
        assert g.size == len(dirs) * ns
        out = np.zeros((self.n, GRAD_STRIDE), np.float32) if want_table else None
        gs = np.zeros((len(dirs), ns), np.float32) if want_grad_s else None
        rows = np.zeros((len(dirs), RAY_GRAD_STRIDE), np.float32) if want_rays else None
        self._chk(self._L.vrt_hip_transmittance_bundle_grad_rays(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), _fp(s), ns, int(s_per_ray),
                                                                 _fp(g), int(wrt), _fp(out) if want_table else None,
                                                                 _fp(gs) if want_grad_s else None, _fp(rows) if want_rays else None),
                  "transmittance_bundle_grad")
        res = ((grad_columns(out) if want_table else None), gs)
        return res + (ray_grad_columns(rows),) if want_rays else res

    def transmittance_bundle_grad_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_s, ns, s_per_ray, d_grad_T, wrt, d_grad=0, d_grad_s=0,
                                         stream=0):
        """vrt_hip_transmittance_bundle_grad_device: device pointers, everything enqueued on `stream`; ADDS into columns 4..8 of d_grad
        ([N, GRAD_STRIDE] float32: grad_columns names its columns) and STORES d_grad_s ([nrays, ns]); either may be 0, not both."""
        self._device("transmittance_bundle_grad_device", nrays, d_origins, origin_per_ray, d_dirs, d_s or None, int(ns), int(bool(s_per_ray)),
                     d_grad_T or None, int(wrt), d_grad or None, d_grad_s or None, stream or None)

    def transmittance_bundle_grad_rays_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_s, ns, s_per_ray, d_grad_T, wrt, d_grad=0, d_grad_s=0,
                                              d_grad_rays=0, stream=0):
        """vrt_hip_transmittance_bundle_grad_rays_device: as transmittance_bundle_grad_device, and STORES d_grad_rays ([nrays,
        RAY_GRAD_STRIDE] float32, 16-byte aligned); any of the three outputs may be 0, not all."""
        self._device("transmittance_bundle_grad_rays_device", nrays, d_origins, origin_per_ray, d_dirs, d_s or None, int(ns), int(bool(s_per_ray)),
                     d_grad_T or None, int(wrt), d_grad or None, d_grad_s or None, d_grad_rays or None, stream or None)

    def transmittance_bundle_tangent(self, origins, dirs, s, tangent=None, ray_tangent=None, s_tangent=None, wrt=TGRAD_T, s_per_ray=None):
        """vrt_hip_transmittance_bundle_tangent: forward mode, J . v -- how what transmittance_bundle returns for the same rays and samples
        s moves along a direction (wrt = TGRAD_T), or, with wrt = TGRAD_DEPTH and s [nrays, ns] the depths depth_bundle returned, how those
        depths move (the derivative of the ideal crossing; a depth of +inf, 0 or NaN gets exactly 0).  Each ray's kept list is held
        fixed.  tangent and ray_tangent: as radiance_rays_tangent takes them, dicts or packed arrays ("albedo" is never read: T does not
        depend on it); s_tangent: the direction's part in the samples (TGRAD_T) or in the levels (TGRAD_DEPTH), [ns] shared by the rays
        or [nrays, ns].  Each may be None (zero), not all three.  Returns float32 [nrays, ns], stored without atomic adds: bitwise
        reproducible."""
        origins, dirs, per_ray = _rays(origins, dirs)
        s, ns, s_per_ray = _table(s, len(dirs), s_per_ray)
        t = None if tangent is None else _pack_tangent(tangent, self.n)
        rt = None if ray_tangent is None else _pack_ray_tangent(ray_tangent, len(dirs))
        st, st_per_ray = None, False
        if s_tangent is not None:
            st = np.ascontiguousarray(s_tangent, np.float32)
            st_per_ray = st.ndim == 2
            assert st.size == (len(dirs) if st_per_ray else 1) * ns, st.shape
        out = np.zeros((len(dirs), ns), np.float32)
        self._chk(self._L.vrt_hip_transmittance_bundle_tangent(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), _fp(s), ns, int(s_per_ray),
                                                               int(wrt), None if t is None else _fp(t), None if rt is None else _fp(rt),
                                                               None if st is None else _fp(st), int(st_per_ray), _fp(out)),
                  "transmittance_bundle_tangent")
        return out

    def transmittance_bundle_tangent_device(self, nrays, d_origins, origin_per_ray, d_dirs, d_s, ns, s_per_ray, wrt, d_tangent=0, d_ray_tangent=0,
                                            d_s_tangent=0, s_tangent_per_ray=True, d_out=0, stream=0):
        """vrt_hip_transmittance_bundle_tangent_device: device pointers, everything enqueued on `stream`; reads d_tangent ([N, GRAD_STRIDE]
        float32), d_ray_tangent ([nrays, RAY_GRAD_STRIDE] float32), both 16-byte aligned, and d_s_tangent ([nrays, ns], or [ns] with
        s_tangent_per_ray false); each may be 0, not all three; STORES d_out ([nrays, ns] float32)."""
        self._device("transmittance_bundle_tangent_device", nrays, d_origins, origin_per_ray, d_dirs, d_s or None, int(ns), int(bool(s_per_ray)),
                     int(wrt), d_tangent or None, d_ray_tangent or None, d_s_tangent or None, int(bool(s_tangent_per_ray)), d_out or None,
                     stream or None)

    # ---- ray plans (cull once, reuse the kept lists in every bundle call) ----
    def ray_plan(self, origins, dirs):
        """vrt_hip_ray_plan_create: culls the bundle once, as every bundle call would (through the index and in the sorted order when
        those switches are on), and keeps every ray's list.  origins [3] (one for the bundle) or [nrays, 3], dirs [nrays, 3].  Returns a
        RayPlan; bind it with set_ray_plan or `with renderer.using(plan):`."""
        origins, dirs, per_ray = _rays(origins, dirs)
        h = _vp()
        self._chk(self._L.vrt_hip_ray_plan_create(self._h, len(dirs), _fp(origins), int(per_ray), _fp(dirs), C.byref(h)), "ray_plan_create")
        return RayPlan(self, h)

    def ray_plan_device(self, nrays, d_origins, origin_per_ray, d_dirs, stream=0):
        """vrt_hip_ray_plan_create_device: the same from device pointers, enqueued on `stream` and waited for: the plan is complete when
        this returns and may be used on any stream."""
        h = _vp()
        self._chk(self._L.vrt_hip_ray_plan_create_device(self._h, int(nrays), d_origins or None, int(bool(origin_per_ray)), d_dirs or None,
                                                         stream or None, C.byref(h)), "ray_plan_create_device")
        return RayPlan(self, h)

    def set_ray_plan(self, plan, keep_lists=False):
        """vrt_hip_set_ray_plan: while a plan is bound (None: none) every bundle call of nrays = the plan's takes its lists from it -- the
        same bits, no cull.  Strict by default: a call after the scene or the cull options were set again raises; with keep_lists the
        lists stay in force across scene updates that keep N (the function the gradient and tangent bundles differentiate)."""
        if plan is not None and (plan._p is None or plan._r is not self):
            raise VrtHipError("set_ray_plan: the plan is closed, or belongs to another renderer")
        self._chk(self._L.vrt_hip_set_ray_plan(self._h, plan._p if plan is not None else None, PLAN_KEEP_LISTS if (plan is not None and keep_lists) else 0),
                  "set_ray_plan")
        self._plan = (plan, bool(keep_lists) if plan is not None else False)

    def using(self, plan, keep_lists=False):
        """Context manager: `with renderer.using(plan, keep_lists=False):` binds the plan for the block and restores the binding that
        was there before."""
        return _UsingPlan(self, plan, keep_lists)

    def ray_stats(self):
        """Counts of the last bundle (enable_stats first): see vrt_hip_ray_stats in include/vrt_hip.h."""
        s = RayStats()
        self._chk(self._L.vrt_hip_get_ray_stats(self._h, C.byref(s)), "get_ray_stats")
        return {k: getattr(s, k) for k, _ in RayStats._fields_}

    def set_ray_index(self, on):
        """Ray bundles cull through the Morton index of the scene (off by default; the same bits either way): see
        vrt_hip_set_ray_index in include/vrt_hip.h."""
        self._chk(self._L.vrt_hip_set_ray_index(self._h, int(bool(on))), "set_ray_index")

    def ray_index_stats(self):
        """The index's counts of the last bundle (enable_stats first): see vrt_hip_ray_index_stats in include/vrt_hip.h."""
        s = RayIndexStats()
        self._chk(self._L.vrt_hip_get_ray_index_stats(self._h, C.byref(s)), "get_ray_index_stats")
        return {k: getattr(s, k) for k, _ in RayIndexStats._fields_}

    def ray_index_perm(self):
        """Diagnostic: the Morton index as perm[Morton position] = scene index, u32 [N] (waits; raises while the index is off or not
        built): see vrt_hip_get_ray_index_perm in include/vrt_hip.h."""
        out = np.zeros(max(self.n, 1), np.uint32)
        self._chk(self._L.vrt_hip_get_ray_index_perm(self._h, out.ctypes.data_as(_u32p), out.size), "get_ray_index_perm")
        return out[:self.n]

    def set_ray_sort(self, on):
        """Ray bundles of more than 64 rays are shaded in an order that puts rays which keep the same bounding spheres into the same wave
        (off by default; every output stays at the caller's ray index, the same bits either way): see vrt_hip_set_ray_sort in
        include/vrt_hip.h."""
        self._chk(self._L.vrt_hip_set_ray_sort(self._h, int(bool(on))), "set_ray_sort")

    def ray_sort_stats(self):
        """Whether the last bundle was sorted, its rays and those that keep no sphere: see vrt_hip_ray_sort_stats in include/vrt_hip.h."""
        s = RaySortStats()
        self._chk(self._L.vrt_hip_get_ray_sort_stats(self._h, C.byref(s)), "get_ray_sort_stats")
        return {k: getattr(s, k) for k, _ in RaySortStats._fields_}

    def ray_order(self):
        """Diagnostic: (order u32 [nrays], keys u32 [nrays]) of the last sorted bundle -- order[slot] = ray id, keys[ray id] (waits; raises
        while the sort is off or the last bundle was not sorted): see vrt_hip_get_ray_order in include/vrt_hip.h."""
        n = self.ray_sort_stats()["rays"]
        order, keys, count = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), C.c_size_t()
        self._chk(self._L.vrt_hip_get_ray_order(self._h, order.ctypes.data_as(_u32p), keys.ctypes.data_as(_u32p), order.size, C.byref(count)),
                  "get_ray_order")
        return order[:count.value], keys[:count.value]

    def set_grad_ordered(self, on):
        """Gradient bundles build their table without float atomics, bit for bit reproducible and summed in a documented order (off by
        default; an ordered call waits once for its stream): see vrt_hip_set_grad_ordered in include/vrt_hip.h."""
        self._chk(self._L.vrt_hip_set_grad_ordered(self._h, int(bool(on))), "set_grad_ordered")

    def grad_records(self):
        """The records the last ordered gradient bundle reduced its table from, in consumed order (Gaussian, ray, place in the ray):
        (gauss u32 [m], ray u32 [m], rows f32 [m, 9] = the table's columns 0..8).  Waits; m = 0 before any ordered call.  See
        vrt_hip_get_grad_records in include/vrt_hip.h."""
        n = C.c_size_t()
        rc = self._L.vrt_hip_get_grad_records(self._h, None, None, None, 0, C.byref(n))
        m = n.value
        gauss, ray, rows = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, GRAD_RECORD_COLS), np.float32)
        if m == 0:
            self._chk(rc, "get_grad_records")
            return gauss, ray, rows
        self._chk(self._L.vrt_hip_get_grad_records(self._h, gauss.ctypes.data_as(_u32p), ray.ctypes.data_as(_u32p), _fp(rows), m, C.byref(n)),
                  "get_grad_records")
        return gauss, ray, rows

    def grad_ordered_stats(self):
        """Counts of the last ordered gradient bundle (records, Gaussians with records, longest segment, mismatches): see
        vrt_hip_grad_ordered_stats in include/vrt_hip.h."""
        s = GradOrderedStats()
        self._chk(self._L.vrt_hip_get_grad_ordered_stats(self._h, C.byref(s)), "get_grad_ordered_stats")
        return {k: getattr(s, k) for k, _ in GradOrderedStats._fields_}

    def eval_erf(self, kind, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x)
        self._chk(self._L.vrt_hip_eval_erf(self._h, kind, _fp(x), x.size, _fp(y)), "eval_erf")
        return y

    def eval_exp(self, kind, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x)
        self._chk(self._L.vrt_hip_eval_exp(self._h, kind, _fp(x), x.size, _fp(y)), "eval_exp")
        return y

    def enable_stats(self, on=True):
        self._chk(self._L.vrt_hip_enable_stats(self._h, int(on)), "enable_stats")

    def set_table_step(self, step):
        """Table mode for dense blocks (default 0.05; 0 = exact kernels only): see vrt_hip_set_table_step in include/vrt_hip.h."""
        self._chk(self._L.vrt_hip_set_table_step(self._h, float(step)), "set_table_step")
        self.table_step = float(step)

    def set_cull_prune(self, kappa):
        """Budget factor of the block kernel's ray-level prune (default 6; 0 = off): see vrt_hip_set_cull_prune in include/vrt_hip.h."""
        self._chk(self._L.vrt_hip_set_cull_prune(self._h, float(kappa)), "set_cull_prune")

    def set_table_budget(self, budget):
        """Largest worst-case change of a ray's radiance the table kernel may cause (default 2.5e-5)."""
        self._chk(self._L.vrt_hip_set_table_budget(self._h, float(budget)), "set_table_budget")

    def enable_kernel_timing(self, on=True):
        self._chk(self._L.vrt_hip_enable_kernel_timing(self._h, int(on)), "enable_kernel_timing")

    def kernel_timing(self):
        """Mean HIP-event durations (ms) of the render kernel, the dense kernel and the list kernels."""
        r, d, l, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        self._chk(self._L.vrt_hip_get_kernel_timing(self._h, C.byref(r), C.byref(d), C.byref(l), C.byref(n)),
                  "get_kernel_timing")
        return dict(render_ms=r.value, dense_ms=d.value, lists_ms=l.value, launches=n.value)

    def stats(self):
        s = Stats()
        self._chk(self._L.vrt_hip_get_stats(self._h, C.byref(s)), "get_stats")
        return {k: (list(getattr(s, k)) if k == "table_phase_ticks" else getattr(s, k)) for k, _ in Stats._fields_}


class Group:
    """Several GPUs from one process (vrt_hip_group_*): one member context per entry of `devices`; a device listed twice
    gives two members on it (protocol tests on a one-GPU box)."""

    def __init__(self, devices):
        self._L = lib()
        d = (C.c_int * len(devices))(*devices)
        h = _vp()
        rc = self._L.vrt_hip_group_create(d, len(devices), C.byref(h))
        if rc != 0:
            raise VrtHipError(f"vrt_hip_group_create failed ({rc}): {self._L.vrt_hip_group_last_error(None).decode()}")
        self._g = h
        self.members = [Renderer(_handle=_vp(self._L.vrt_hip_group_ctx(h, i))) for i in range(len(devices))]

    def frame(self, tw, th, view, origin, pack, want_image=True, wait=True):
        w, h = self.members[0].w, self.members[0].h
        img = np.zeros(w * h, np.uint32) if want_image else None
        v = np.ascontiguousarray(view, np.float32).ravel()
        rc = self._L.vrt_hip_group_frame(self._g, float(tw), float(th), _fp(v), _fp(_f3(origin)), int(pack),
                                         img.ctypes.data_as(_u32p) if want_image else None, int(wait))
        if rc != 0:
            raise VrtHipError(f"group_frame failed ({rc}): {self._L.vrt_hip_group_last_error(self._g).decode()}")
        return img.reshape(h, w) if want_image else None

    def frame_batch(self, tw, th, views, origins, pack, want_images=True):
        """vrt_hip_group_frame_batch: len(views) frames with one launch of each kernel per member and one assembly launch;
        returns the images [n, h, w] (or None)."""
        n = len(views)
        w, h = self.members[0].w, self.members[0].h
        v = np.ascontiguousarray(np.asarray(views, np.float32).reshape(n, 16))
        o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(n, 3))
        imgs = np.zeros((n, h, w), np.uint32) if want_images else None
        ptrs = (C.c_void_p * n)(*[imgs[i].ctypes.data for i in range(n)]) if want_images else None
        rc = self._L.vrt_hip_group_frame_batch(self._g, n, float(tw), float(th), _fp(v), _fp(o), int(pack), ptrs, 1)
        if rc != 0:
            raise VrtHipError(f"group_frame_batch failed ({rc}): {self._L.vrt_hip_group_last_error(self._g).decode()}")
        return imgs

    def sync(self):
        rc = self._L.vrt_hip_group_sync(self._g)
        if rc != 0:
            raise VrtHipError(f"group_sync failed ({rc}): {self._L.vrt_hip_group_last_error(self._g).decode()}")

    def close(self):
        if getattr(self, "_g", None):
            for m in self.members:
                m.close()
            self._L.vrt_hip_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

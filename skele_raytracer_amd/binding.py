"""ctypes binding of lib/libskr.so (include/skr.h).  No compute happens here."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

# every symbol include/skr.h declares (tests/test_abi.py checks the library exports them)
EXPORTED_SYMBOLS = [
    "skr_scene_create_from_scn", "skr_scene_create_from_scn_ex", "skr_scene_create_from_arrays", "skr_scene_set_triangle_materials", "skr_scene_set_sphere_ior", "skr_scene_get_fog", "skr_scene_set_fog", "skr_scene_get_spot_lights", "skr_scene_set_spot_lights", "skr_scene_get_spot_cones", "skr_scene_set_light_radii", "skr_scene_get_light_radii", "skr_scene_set_lens", "skr_scene_get_lens", "skr_scene_set_sphere_velocities", "skr_scene_get_sphere_velocities", "skr_scene_set_shutter", "skr_scene_get_shutter", "skr_scene_set_environment", "skr_scene_get_environment", "skr_read_pfm", "skr_scene_add_texture", "skr_scene_get_texture", "skr_scene_texture_count", "skr_scene_set_sphere_textures", "skr_scene_get_sphere_textures", "skr_scene_clear_textures", "skr_scene_set_sphere_emission", "skr_scene_get_sphere_emission", "skr_scene_set_triangle_shadows", "skr_scene_get_triangle_shadows", "skr_scene_set_sphere_tree", "skr_scene_get_sphere_tree", "skr_scene_get_sphere_tree_data", "skr_renderer_read_sphere_tree_work", "skr_scene_destroy", "skr_scene_get_info",
    "skr_scene_get_arrays", "skr_scene_get_culling", "skr_scene_get_trace_culling", "skr_scene_get_shadow_masks", "skr_scene_get_gi_masks", "skr_options_default", "skr_radiance_ray_count", "skr_device_count",
    "skr_renderer_create", "skr_renderer_clone", "skr_renderer_destroy", "skr_render_tiles", "skr_render_tile_list", "skr_tile_costs", "skr_tile_count", "skr_render_rows",
    "skr_renderer_read_counters", "skr_renderer_read_work", "skr_renderer_read_triangle_work", "skr_renderer_count_triangle_work", "skr_renderer_kernel_work", "skr_renderer_reload_switches", "skr_renderer_kernel_timing", "skr_renderer_kernel_ms", "skr_renderer_last_parent_count", "skr_renderer_last_level1_count", "skr_renderer_primary_cache_stats", "skr_render_frame_host", "skr_render_progressive_host", "skr_accumulate", "skr_resolve_accumulated", "skr_write_png", "skr_write_pfm", "skr_write_ppm", "skr_last_error",
    "skr_kernel_variant", "skr_debug_eval",
    "skr_rccl_available", "skr_multi_create", "skr_multi_destroy", "skr_multi_device_count", "skr_multi_renderer", "skr_multi_render_frame",
    "skr_multi_render_frame_host", "skr_comm_unique_id", "skr_comm_create", "skr_comm_destroy", "skr_comm_render_frame", "skr_comm_render_frame_async", "skr_comm_flush", "skr_comm_frame_to_host",
    "skr_shard_tiles_per_rank", "skr_shard_deinterleave_host", "skr_shard_lpt", "skr_shard_by_cost", "skr_shard_plan", "skr_shard_deinterleave_map_host", "skr_multi_render_frame_async", "skr_multi_flush",
    "skr_trace_rays", "skr_camera_rays", "skr_shade_rays", "skr_denoise", "skr_render_denoised_host",
    "skr_adaptive_default", "skr_render_adaptive", "skr_render_adaptive_host",
    "skr_render_adaptive_var", "skr_denoise_var", "skr_render_adaptive_denoised_host",
]

DENOISE_ITERATIONS = 5  # include/skr.h SKR_DENOISE_ITERATIONS: Renderer.denoise's default
# include/skr.h SKR_ADAPTIVE_*: Renderer.render_adaptive's defaults, the luminance floor of the rule and the largest max_passes
ADAPTIVE_MIN_PASSES = 8
ADAPTIVE_MAX_PASSES = 64
ADAPTIVE_THRESHOLD = 0.05
ADAPTIVE_LUM_FLOOR = 0.00390625
ADAPTIVE_PASS_LIMIT = 65535
DENOISE_VAR_SIGMA_L = 4.0  # include/skr.h SKR_DENOISE_VAR_SIGMA_L: the luminance sigma of denoise(variance=...)


class SkrError(RuntimeError):
    pass


class COptions(C.Structure):
    # struct skr_options == reference struct Options (utils.h:26-34) + width/height/use_shadows
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fov", C.c_float), ("monte_carlo", C.c_int32),
                ("num_path_traces", C.c_int32), ("grid_size", C.c_int32), ("max_depth", C.c_int32),
                ("use_shadows", C.c_int32), ("seed", C.c_uint64), ("shade_triangles", C.c_int32), ("progressive_passes", C.c_int32), ("legacy_reflect", C.c_int32)]


# include/skr.h skr_progress_fn: (user, passes_done, passes, h_rgb, h_rgbf) -> non-zero stops the render
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)


class CSceneInfo(C.Structure):
    _fields_ = [("n_spheres", C.c_int32), ("n_triangles", C.c_int32), ("n_point_lights", C.c_int32),
                ("n_vertices", C.c_int32), ("n_directional_dropped", C.c_int32), ("n_fog_skipped", C.c_int32),
                ("n_unknown", C.c_int32), ("n_bad_triangles", C.c_int32), ("film_width", C.c_int32),
                ("film_height", C.c_int32), ("max_depth_parsed", C.c_int32), ("camera", C.c_float * 13),
                ("background", C.c_float * 3), ("ambient", C.c_float * 3), ("n_directional_lights", C.c_int32)]


def lib_path():
    """lib/libskr.so, or the build named by SKR_LIBRARY (kernel experiments: same ABI, other tuning macros)."""
    return os.environ.get("SKR_LIBRARY") or os.path.join(_HERE, "lib", "libskr.so")


_lib = None


def lib():
    """Load libskr.so.  Import torch first when torch is in the process, so that the one
    libamdhip64.so.7 torch ships is the HIP runtime both sides use."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise SkrError("%s is missing: run `make lib` (or __graft_entry__.build()); there is no fallback path" % path)
    try:
        import torch  # noqa: F401  (HIP runtime load order, see docstring)
    except ImportError:
        pass
    L = C.CDLL(path)
    vp = C.c_void_p
    L.skr_scene_create_from_scn.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.skr_scene_create_from_scn_ex.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.skr_scene_create_from_arrays.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, C.POINTER(vp)]
    L.skr_scene_set_triangle_materials.argtypes = [vp, vp]
    L.skr_scene_set_sphere_ior.argtypes = [vp, vp]
    L.skr_scene_get_fog.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_set_fog.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_spot_lights.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_set_spot_lights.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_spot_cones.argtypes = [vp, vp]
    L.skr_scene_set_light_radii.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_light_radii.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_set_lens.argtypes = [vp, C.c_float, C.c_float]
    L.skr_scene_get_lens.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.skr_scene_set_sphere_velocities.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_sphere_velocities.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_set_shutter.argtypes = [vp, C.c_float]
    L.skr_scene_get_shutter.argtypes = [vp, C.POINTER(C.c_float)]
    L.skr_scene_set_environment.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_environment.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_add_texture.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_texture.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_int32)]
    L.skr_scene_texture_count.argtypes = [vp]
    L.skr_scene_set_sphere_textures.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_sphere_textures.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_scene_clear_textures.argtypes = [vp]
    L.skr_scene_set_sphere_emission.argtypes = [vp, vp, C.c_int32]
    L.skr_scene_get_sphere_emission.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.skr_read_pfm.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp]
    L.skr_scene_set_triangle_shadows.argtypes = [vp, C.c_int]
    L.skr_scene_get_triangle_shadows.argtypes = [vp, C.POINTER(C.c_int)]
    L.skr_scene_set_sphere_tree.argtypes = [vp, C.c_int]
    L.skr_scene_get_sphere_tree.argtypes = [vp, C.POINTER(C.c_int)]
    L.skr_scene_get_sphere_tree_data.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp, vp, vp, vp, vp]
    L.skr_renderer_read_sphere_tree_work.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.skr_scene_destroy.argtypes = [vp]
    L.skr_scene_destroy.restype = None
    L.skr_scene_get_info.argtypes = [vp, C.POINTER(CSceneInfo)]
    L.skr_scene_get_arrays.argtypes = [vp, vp, vp, vp]
    L.skr_scene_get_culling.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp, vp]
    L.skr_scene_get_trace_culling.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp, vp, vp]
    L.skr_scene_get_shadow_masks.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), vp]
    L.skr_scene_get_gi_masks.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp]
    L.skr_options_default.argtypes = [C.POINTER(COptions)]
    L.skr_options_default.restype = None
    L.skr_radiance_ray_count.argtypes = [C.POINTER(COptions)]
    L.skr_radiance_ray_count.restype = C.c_uint64
    L.skr_device_count.restype = C.c_int
    L.skr_renderer_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.skr_renderer_clone.argtypes = [vp, C.POINTER(vp)]
    L.skr_renderer_destroy.argtypes = [vp]
    L.skr_renderer_destroy.restype = None
    L.skr_render_tiles.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.skr_tile_count.argtypes = [C.POINTER(COptions), C.c_uint32, C.c_uint32, C.c_uint32]
    L.skr_tile_count.restype = C.c_uint32
    L.skr_render_rows.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.c_uint32, vp, vp, vp]
    L.skr_renderer_read_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.skr_renderer_read_work.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.skr_renderer_read_triangle_work.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.skr_renderer_kernel_work.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.skr_renderer_count_triangle_work.argtypes = [vp, C.c_int]
    L.skr_renderer_reload_switches.argtypes = [vp]
    L.skr_renderer_kernel_timing.argtypes = [vp, C.c_int]
    L.skr_renderer_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    L.skr_renderer_last_parent_count.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.skr_renderer_last_level1_count.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.skr_renderer_primary_cache_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.skr_render_frame_host.argtypes = [vp, C.POINTER(COptions), vp, C.POINTER(C.c_float)]
    L.skr_write_ppm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp]
    L.skr_write_png.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp]
    L.skr_write_pfm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp]
    L.skr_render_progressive_host.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp, vp, PROGRESS_FN, vp, C.POINTER(C.c_float)]
    L.skr_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_int, vp]
    L.skr_resolve_accumulated.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.skr_last_error.restype = C.c_char_p
    L.skr_kernel_variant.restype = C.c_char_p
    L.skr_debug_eval.argtypes = [C.c_int, vp, vp, C.c_uint32, vp]
    L.skr_rccl_available.restype = C.c_int
    L.skr_multi_create.argtypes = [vp, C.c_int, vp, C.POINTER(vp)]
    L.skr_multi_destroy.argtypes = [vp]
    L.skr_multi_destroy.restype = None
    L.skr_multi_device_count.argtypes = [vp]
    L.skr_multi_renderer.argtypes = [vp, C.c_int]
    L.skr_multi_renderer.restype = vp
    L.skr_multi_render_frame.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.POINTER(vp), C.POINTER(C.c_float)]
    L.skr_multi_render_frame_host.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp, C.POINTER(C.c_float)]
    L.skr_comm_unique_id.argtypes = [vp]
    L.skr_comm_create.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.skr_comm_destroy.argtypes = [vp]
    L.skr_comm_destroy.restype = None
    L.skr_comm_render_frame.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.POINTER(vp), vp]
    L.skr_comm_frame_to_host.argtypes = [vp, vp, vp]
    L.skr_comm_render_frame_async.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.POINTER(vp), vp]
    L.skr_comm_flush.argtypes = [vp, C.POINTER(vp), vp]
    L.skr_multi_render_frame_async.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.POINTER(vp)]
    L.skr_multi_flush.argtypes = [vp, C.POINTER(vp)]
    L.skr_render_tile_list.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp, C.c_uint32, vp, vp, vp]
    L.skr_tile_costs.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp]
    L.skr_shard_lpt.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.skr_shard_by_cost.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.skr_shard_plan.argtypes = [vp, C.POINTER(COptions), C.c_uint32, C.c_uint32, vp]
    L.skr_shard_deinterleave_map_host.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_uint32, vp]
    L.skr_shard_tiles_per_rank.argtypes = [C.c_int32, C.c_uint32, C.c_uint32]
    L.skr_shard_tiles_per_rank.restype = C.c_uint32
    L.skr_shard_deinterleave_host.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32]
    L.skr_trace_rays.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.skr_camera_rays.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp, vp]
    L.skr_shade_rays.argtypes = [vp, C.POINTER(COptions), vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.skr_denoise.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp]
    L.skr_render_denoised_host.argtypes = [vp, C.POINTER(COptions), C.c_uint32, vp, vp, C.POINTER(C.c_float)]
    L.skr_adaptive_default.argtypes = [C.POINTER(CAdaptive)]
    L.skr_adaptive_default.restype = None
    L.skr_render_adaptive.argtypes = [vp, C.POINTER(COptions), C.POINTER(CAdaptive), vp, vp, vp, vp]
    L.skr_render_adaptive_host.argtypes = [vp, C.POINTER(COptions), C.POINTER(CAdaptive), vp, vp, vp, C.POINTER(C.c_float)]
    L.skr_render_adaptive_var.argtypes = [vp, C.POINTER(COptions), C.POINTER(CAdaptive), vp, vp, vp, vp, vp]
    L.skr_denoise_var.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.skr_render_adaptive_denoised_host.argtypes = [vp, C.POINTER(COptions), C.POINTER(CAdaptive), C.c_uint32, vp, vp, vp, C.POINTER(C.c_float)]
    _lib = L
    return L


class CAdaptive(C.Structure):
    """include/skr.h skr_adaptive"""
    _fields_ = [("min_passes", C.c_int32), ("max_passes", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32)]


def adaptive_params(threshold=ADAPTIVE_THRESHOLD, min_passes=ADAPTIVE_MIN_PASSES, max_passes=ADAPTIVE_MAX_PASSES):
    """An include/skr.h skr_adaptive; libskr checks the limits (SKR_ERR_ARG)."""
    a = CAdaptive()
    lo, hi = -(1 << 31), (1 << 31) - 1
    a.min_passes = min(max(int(min_passes), lo), hi)
    a.max_passes = min(max(int(max_passes), lo), hi)
    a.threshold = float(threshold)
    return a


def _check(rc, what):
    if rc != 0:
        raise SkrError("%s failed (status %d): %s" % (what, rc, (lib().skr_last_error() or b"").decode()))


class Options:
    """Reference struct Options (utils.h:26-34) with the reference's defaults, plus the
    width/height/use_shadows main() folds in (main.cpp:393-396) and the RNG seed."""

    def __init__(self, width=1920, height=1080, fov=None, gillum=None, jsample=0, depth=3, shadow=False, seed=1, shade_triangles=False, progressive=1, legacy_reflect=False,
                 scn_fov=None):
        c = COptions()
        lib().skr_options_default(C.byref(c))
        if fov is None:  # --scn-fov: fov = 2 x the camera line's half_height_angle (a Scene in scn_fov) unless --fov is given; else utils.h:30
            fov = scene_fov(scn_fov) if scn_fov is not None else 60.0
        c.width, c.height, c.fov = width, height, fov
        if gillum is not None:  # main.cpp:252-253: --gillum N sets monte_carlo and num_path_traces
            c.monte_carlo, c.num_path_traces = 1, gillum
        c.grid_size, c.max_depth, c.use_shadows, c.seed = jsample, depth, int(bool(shadow)), seed
        c.shade_triangles = int(bool(shade_triangles))  # --shade-triangles (include/skr.h): triangles as surfaces, not black holes
        c.progressive_passes = max(1, int(progressive))  # --progressive K: the mean of K frames under the seeds seed .. seed+K-1
        c.legacy_reflect = int(bool(legacy_reflect))  # --legacy-reflect (include/skr.h): the reflection / refraction code behind raytrace.h:44's early return
        self.c = c

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height


def radiance_ray_count(opt):
    return int(lib().skr_radiance_ray_count(C.byref(opt.c)))


class Scene:
    """Host scene (reference struct Scene, scene.h:13-28) in SoA form; see parse_scene()."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    def close(self):
        if self.h:
            try:
                lib().skr_scene_destroy(self.h)
            except TypeError:  # (interpreter teardown)
                pass
            self.h = None

    __del__ = close

    @property
    def info(self):
        i = CSceneInfo()
        _check(lib().skr_scene_get_info(self.h, C.byref(i)), "skr_scene_get_info")
        return i

    def arrays(self):
        i = self.info
        s = np.zeros((i.n_spheres, 14), np.float32)
        t = np.zeros((i.n_triangles, 9), np.float32)
        l = np.zeros((i.n_point_lights, 6), np.float32)
        _check(lib().skr_scene_get_arrays(self.h, s.ctypes.data, t.ctypes.data, l.ctypes.data), "skr_scene_get_arrays")
        return s, t, l

    def culling(self, level=0):
        """(chunk_size, device_tris [n,3,4], node_spheres [nn,8], node_links [nn,4] int32, chunk_spheres [nc,8]) —
        include/skr.h skr_scene_get_culling."""
        cs, nn, nc = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().skr_scene_get_culling(self.h, level, C.byref(cs), C.byref(nn), C.byref(nc), None, None, None, None), "skr_scene_get_culling")
        tris = np.zeros((self.info.n_triangles, 3, 4), np.float32)
        sph = np.zeros((nn.value, 8), np.float32)
        links = np.zeros((nn.value, 4), np.int32)
        ch = np.zeros((nc.value, 8), np.float32)
        _check(lib().skr_scene_get_culling(self.h, level, None, None, None, tris.ctypes.data, sph.ctypes.data, links.ctypes.data, ch.ctypes.data),
               "skr_scene_get_culling")
        return cs.value, tris, sph, links, ch

    def trace_culling(self, level=0):
        """culling() for the trace tree (the ray queries' and the triangle-shadow walk's), plus its ball (centre, radius) float32 [4] —
        include/skr.h skr_scene_get_trace_culling."""
        cs, nn, nc = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().skr_scene_get_trace_culling(self.h, level, C.byref(cs), C.byref(nn), C.byref(nc), None, None, None, None, None), "skr_scene_get_trace_culling")
        tris = np.zeros((self.info.n_triangles, 3, 4), np.float32)
        sph = np.zeros((nn.value, 8), np.float32)
        links = np.zeros((nn.value, 4), np.int32)
        ch = np.zeros((nc.value, 8), np.float32)
        ball = np.zeros(4, np.float32)
        _check(lib().skr_scene_get_trace_culling(self.h, level, None, None, None, tris.ctypes.data, sph.ctypes.data, links.ctypes.data, ch.ctypes.data,
                                                 ball.ctypes.data), "skr_scene_get_trace_culling")
        return cs.value, tris, sph, links, ch, ball

    def shadow_masks(self):
        """(masks [n_lights, 6, cells, cells] uint32, reach2) — include/skr.h skr_scene_get_shadow_masks; n_lights = 0: the scene has none."""
        nl, cells, reach2 = C.c_int32(), C.c_int32(), C.c_float()
        _check(lib().skr_scene_get_shadow_masks(self.h, C.byref(nl), C.byref(cells), C.byref(reach2), None), "skr_scene_get_shadow_masks")
        m = np.zeros((nl.value, 6, cells.value, cells.value), np.uint32)
        _check(lib().skr_scene_get_shadow_masks(self.h, None, None, None, m.ctypes.data), "skr_scene_get_shadow_masks")
        return m, reach2.value

    def gi_masks(self):
        """(table uint32 words, mask_word, wide, dir_cells, grids [2, 8] float32) — include/skr.h skr_scene_get_gi_masks; an empty table: the scene has none."""
        nw, mw, wide, dc = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        grids = np.zeros((2, 8), np.float32)
        _check(lib().skr_scene_get_gi_masks(self.h, C.byref(nw), C.byref(mw), C.byref(wide), C.byref(dc), grids.ctypes.data, None), "skr_scene_get_gi_masks")
        t = np.zeros(nw.value, np.uint32)
        _check(lib().skr_scene_get_gi_masks(self.h, None, None, None, None, None, t.ctypes.data), "skr_scene_get_gi_masks")
        return t, mw.value, wide.value, dc.value, grids

    @property
    def fog(self):
        """The fog volumes [n, 9] = centre(3) radius albedo(3) scattering absorption, in file order (include/skr.h skr_scene_get_fog)."""
        n = C.c_int32()
        _check(lib().skr_scene_get_fog(self.h, None, C.byref(n)), "skr_scene_get_fog")
        rows = np.zeros((n.value, 9), np.float32)
        _check(lib().skr_scene_get_fog(self.h, rows.ctypes.data, C.byref(n)), "skr_scene_get_fog")
        return rows

    def set_fog(self, rows):
        """Replace the fog volumes (rows [n, 9] as `fog` returns them; n = 0: none).  A renderer takes those the scene has when it is made."""
        r = np.ascontiguousarray(rows, np.float32).reshape(-1, 9)
        _check(lib().skr_scene_set_fog(self.h, r.ctypes.data, len(r)), "skr_scene_set_fog")

    @property
    def spot_lights(self):
        """The spot lights [n, 11] = colour(3) position(3) direction(3) angle1 angle2, the file's fields in file order (include/skr.h
        skr_scene_get_spot_lights)."""
        n = C.c_int32()
        _check(lib().skr_scene_get_spot_lights(self.h, None, C.byref(n)), "skr_scene_get_spot_lights")
        rows = np.zeros((n.value, 11), np.float32)
        _check(lib().skr_scene_get_spot_lights(self.h, rows.ctypes.data, C.byref(n)), "skr_scene_get_spot_lights")
        return rows

    def set_spot_lights(self, rows):
        """Replace the spot lights (rows [n, 11] as `spot_lights` returns them; n = 0: none) under the loader's validation.  A renderer
        takes those the scene has when it is made."""
        r = np.ascontiguousarray(rows, np.float32).reshape(-1, 11)
        _check(lib().skr_scene_set_spot_lights(self.h, r.ctypes.data, len(r)), "skr_scene_set_spot_lights")

    @property
    def spot_cones(self):
        """What the host derives once per spot light, [n, 5] = unit axis(3) c1 c2 (include/skr.h skr_scene_get_spot_cones): the values the
        kernels and the checkers read."""
        c = np.zeros((len(self.spot_lights), 5), np.float32)
        _check(lib().skr_scene_get_spot_cones(self.h, c.ctypes.data), "skr_scene_get_spot_cones")
        return c

    @property
    def light_radii(self):
        """The radius of every point and spot light, float32 [n_point + n_spot] in shading order; 0 = a point (include/skr.h
        skr_scene_get_light_radii)."""
        n = C.c_int32()
        _check(lib().skr_scene_get_light_radii(self.h, None, C.byref(n)), "skr_scene_get_light_radii")
        radii = np.zeros(n.value, np.float32)
        _check(lib().skr_scene_get_light_radii(self.h, radii.ctypes.data, C.byref(n)), "skr_scene_get_light_radii")
        return radii

    def set_light_radii(self, radii):
        """Give the point and spot lights a radius (soft shadows; include/skr.h skr_scene_set_light_radii): a scalar for every light, or one
        value per light in shading order.  Finite and >= 0.  A renderer takes those the scene has when it is made; set_spot_lights
        resets them to 0."""
        r = np.asarray(radii, np.float32)
        if r.ndim == 0:
            r = np.full(len(self.light_radii), r, np.float32)
        r = np.ascontiguousarray(r, np.float32).reshape(-1)
        _check(lib().skr_scene_set_light_radii(self.h, r.ctypes.data, len(r)), "skr_scene_set_light_radii")

    @property
    def lens(self):
        """The scene's lens (aperture, focus); aperture 0 = the pinhole camera (include/skr.h skr_scene_get_lens)."""
        a, f = C.c_float(), C.c_float()
        _check(lib().skr_scene_get_lens(self.h, C.byref(a), C.byref(f)), "skr_scene_get_lens")
        return a.value, f.value

    @property
    def velocities(self):
        """The velocity of every sphere, [n_spheres][3]; all 0 = a scene at rest (include/skr.h skr_scene_get_sphere_velocities)."""
        n = C.c_int32(0)
        _check(lib().skr_scene_get_sphere_velocities(self.h, None, C.byref(n)), "skr_scene_get_sphere_velocities")
        v = np.zeros((n.value, 3), np.float32)
        _check(lib().skr_scene_get_sphere_velocities(self.h, v.ctypes.data, C.byref(n)), "skr_scene_get_sphere_velocities")
        return v

    def set_velocities(self, velocities):
        """Give every sphere a velocity (motion blur; include/skr.h skr_scene_set_sphere_velocities states the rule): [n_spheres][3], every
        value finite.  A renderer takes the velocities the scene has when it is made."""
        v = np.ascontiguousarray(velocities, np.float32).reshape(-1)
        if len(v) % 3:
            raise ValueError("velocities: 3 floats per sphere")
        _check(lib().skr_scene_set_sphere_velocities(self.h, v.ctypes.data, len(v) // 3), "skr_scene_set_sphere_velocities")

    @property
    def shutter(self):
        """The scene's shutter S (default 1): a sample's spheres are where they are at a time in [0, S) (include/skr.h skr_scene_get_shutter)."""
        s = C.c_float(0)
        _check(lib().skr_scene_get_shutter(self.h, C.byref(s)), "skr_scene_get_shutter")
        return s.value

    def set_shutter(self, shutter):
        """Set the shutter S, finite and >= 0; 0 = closed: the scene at rest (include/skr.h skr_scene_set_shutter)."""
        _check(lib().skr_scene_set_shutter(self.h, C.c_float(float(shutter))), "skr_scene_set_shutter")

    @property
    def environment(self):
        """The scene's environment, float32 [E, E, 3] with row j first, or None (include/skr.h skr_scene_get_environment)."""
        e = C.c_int32(0)
        _check(lib().skr_scene_get_environment(self.h, None, C.byref(e)), "skr_scene_get_environment")
        if e.value == 0:
            return None
        t = np.zeros((e.value, e.value, 3), np.float32)
        _check(lib().skr_scene_get_environment(self.h, t.ctypes.data, C.byref(e)), "skr_scene_get_environment")
        return t

    def set_environment(self, texels):
        """Give the scene an environment map (include/skr.h skr_scene_set_environment states the rule): [E, E, 3] finite floats, an
        octahedral map with world +y at the centre; rays that miss return it.  None clears it.  A renderer takes the environment the
        scene has when it is made."""
        if texels is None:
            _check(lib().skr_scene_set_environment(self.h, None, 0), "skr_scene_set_environment")
            return
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3 or t.shape[0] == 0:
            raise ValueError("environment: a square [E, E, 3] array")
        _check(lib().skr_scene_set_environment(self.h, t.ctypes.data, t.shape[0]), "skr_scene_set_environment")

    @property
    def textures(self):
        """The scene's textures, a list of float32 [E_k, E_k, 3] arrays with row j first (include/skr.h skr_scene_get_texture)."""
        n = lib().skr_scene_texture_count(self.h)
        if n < 0:
            _check(-n, "skr_scene_texture_count")
        out = []
        for k in range(n):
            e = C.c_int32(0)
            _check(lib().skr_scene_get_texture(self.h, k, None, C.byref(e)), "skr_scene_get_texture")
            t = np.zeros((e.value, e.value, 3), np.float32)
            _check(lib().skr_scene_get_texture(self.h, k, t.ctypes.data, C.byref(e)), "skr_scene_get_texture")
            out.append(t)
        return out

    def add_texture(self, texels):
        """Add a texture (include/skr.h skr_scene_add_texture states the rule): [E, E, 3] finite floats, an octahedral map of a sphere's
        normal with world +y at the centre.  Returns its index, what set_sphere_textures names it by."""
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3 or t.shape[0] == 0:
            raise ValueError("texture: a square [E, E, 3] array")
        k = lib().skr_scene_add_texture(self.h, t.ctypes.data, t.shape[0])
        if k < 0:
            _check(-k, "skr_scene_add_texture")
        return k

    @property
    def sphere_textures(self):
        """The texture index of every sphere, int32 [n_spheres], -1 = none (include/skr.h skr_scene_get_sphere_textures)."""
        n = C.c_int32(0)
        _check(lib().skr_scene_get_sphere_textures(self.h, None, C.byref(n)), "skr_scene_get_sphere_textures")
        x = np.full(n.value, -1, np.int32)
        _check(lib().skr_scene_get_sphere_textures(self.h, x.ctypes.data, C.byref(n)), "skr_scene_get_sphere_textures")
        return x

    def set_sphere_textures(self, indices):
        """Name the texture of every sphere: int [n_spheres], each -1 (none) or the index of a texture the scene holds.  A renderer takes
        the textures and indices the scene has when it is made."""
        x = np.ascontiguousarray(indices, np.int32).reshape(-1)
        _check(lib().skr_scene_set_sphere_textures(self.h, x.ctypes.data, len(x)), "skr_scene_set_sphere_textures")

    def clear_textures(self):
        """Every sphere's texture index back to -1 (the textures stay; include/skr.h skr_scene_clear_textures)."""
        _check(lib().skr_scene_clear_textures(self.h), "skr_scene_clear_textures")

    @property
    def emission(self):
        """The emission of every sphere, float32 [n_spheres, 3], zeros where none was set (include/skr.h skr_scene_get_sphere_emission)."""
        n = C.c_int32(0)
        _check(lib().skr_scene_get_sphere_emission(self.h, None, C.byref(n)), "skr_scene_get_sphere_emission")
        e = np.zeros((n.value, 3), np.float32)
        _check(lib().skr_scene_get_sphere_emission(self.h, e.ctypes.data, C.byref(n)), "skr_scene_get_sphere_emission")
        return e

    def set_emission(self, rgb):
        """Make spheres glow (include/skr.h skr_scene_set_sphere_emission states the rule): [n_spheres, 3] finite floats >= 0, added to
        what shade() returns at that sphere; None clears it.  An emitter lights other surfaces only through --gillum.  A renderer takes
        the emission the scene has when it is made."""
        if rgb is None:
            _check(lib().skr_scene_set_sphere_emission(self.h, None, 0), "skr_scene_set_sphere_emission")
            return
        e = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
        _check(lib().skr_scene_set_sphere_emission(self.h, e.ctypes.data, len(e)), "skr_scene_set_sphere_emission")

    def set_lens(self, aperture, focus=1.0):
        """Give the camera a thin lens (depth of field; include/skr.h skr_scene_set_lens states the rule): aperture radius >= 0 (0: the
        pinhole), focus > 0 in units of the primary ray directions, both finite.  A renderer takes the lens the scene has when it is made."""
        _check(lib().skr_scene_set_lens(self.h, C.c_float(float(aperture)), C.c_float(float(focus))), "skr_scene_set_lens")

    @property
    def triangle_shadows(self):
        """The scene's triangle-shadow switch (include/skr.h skr_scene_set_triangle_shadows)."""
        on = C.c_int()
        _check(lib().skr_scene_get_triangle_shadows(self.h, C.byref(on)), "skr_scene_get_triangle_shadows")
        return bool(on.value)

    def set_triangle_shadows(self, enable):
        """Triangles cast shadows in frames with shade_triangles and shadow (include/skr.h states the rule).  A renderer takes the
        setting the scene has when it is made."""
        _check(lib().skr_scene_set_triangle_shadows(self.h, int(bool(enable))), "skr_scene_set_triangle_shadows")

    def sphere_tree(self):
        """The scene's sphere-tree switch (include/skr.h skr_scene_set_sphere_tree)."""
        on = C.c_int()
        _check(lib().skr_scene_get_sphere_tree(self.h, C.byref(on)), "skr_scene_get_sphere_tree")
        return bool(on.value)

    def set_sphere_tree(self, enable):
        """Frames and shading queries render on the culled sphere walk, spheres in HBM (include/skr.h states the rule).  A renderer takes
        the setting the scene has when it is made."""
        _check(lib().skr_scene_set_sphere_tree(self.h, int(bool(enable))), "skr_scene_set_sphere_tree")

    def sphere_tree_data(self):
        """The sphere tree as a renderer uploads it (include/skr.h skr_scene_get_sphere_tree_data): a dict of chunk_size, n_always (chunks of
        always-tested spheres at the front), spheres [n, 4] float32 in device order, file_index [n] int32, node_spheres [n_nodes, 5] float32
        {centre, R^2, kappa}, node_links [n_nodes, 4] int32 {skip, first chunk, chunk count, smallest file index}, chunk_spheres
        [n_chunks, 5], chunk_links [n_chunks, 3] int32 {smallest file index, first sphere, count}, ball [4]."""
        cs, nn, nc, na = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().skr_scene_get_sphere_tree_data(self.h, C.byref(cs), C.byref(nn), C.byref(nc), C.byref(na), None, None, None, None, None, None, None),
               "skr_scene_get_sphere_tree_data")
        n = self.info.n_spheres
        d = dict(chunk_size=cs.value, n_always=na.value, spheres=np.zeros((n, 4), np.float32), file_index=np.zeros(n, np.int32),
                 node_spheres=np.zeros((nn.value, 5), np.float32), node_links=np.zeros((nn.value, 4), np.int32),
                 chunk_spheres=np.zeros((nc.value, 5), np.float32), chunk_links=np.zeros((nc.value, 3), np.int32), ball=np.zeros(4, np.float32))
        _check(lib().skr_scene_get_sphere_tree_data(self.h, None, None, None, None, d["spheres"].ctypes.data, d["file_index"].ctypes.data,
                                                    d["node_spheres"].ctypes.data, d["node_links"].ctypes.data, d["chunk_spheres"].ctypes.data,
                                                    d["chunk_links"].ctypes.data, d["ball"].ctypes.data), "skr_scene_get_sphere_tree_data")
        return d

    @staticmethod
    def from_arrays(spheres, triangles, point_lights, camera, background=(0, 0, 0), ambient=(0, 0, 0), triangle_materials=None, sphere_ior=None,
                    triangle_shadows=False, sphere_tree=False, light_radii=None, lens=None, velocities=None, shutter=None, environment=None, textures=None,
                    sphere_textures=None, emission=None):
        s = np.ascontiguousarray(spheres, np.float32).reshape(-1, 14)
        t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
        l = np.ascontiguousarray(point_lights, np.float32).reshape(-1, 6)
        cam = np.ascontiguousarray(camera, np.float32).reshape(9)
        bg = np.ascontiguousarray(background, np.float32).reshape(3)
        am = np.ascontiguousarray(ambient, np.float32).reshape(3)
        h = C.c_void_p()
        _check(lib().skr_scene_create_from_arrays(s.ctypes.data, len(s), t.ctypes.data, len(t), l.ctypes.data, len(l),
                                                  cam.ctypes.data, bg.ctypes.data, am.ctypes.data, C.byref(h)),
               "skr_scene_create_from_arrays")
        sc = Scene(h.value)
        if triangle_materials is not None:  # [n_triangles][10] ambient diffuse specular power (--shade-triangles)
            m = np.ascontiguousarray(triangle_materials, np.float32).reshape(len(t), 10)
            _check(lib().skr_scene_set_triangle_materials(sc.h, m.ctypes.data), "skr_scene_set_triangle_materials")
        if sphere_ior is not None:  # [n_spheres] (--legacy-reflect)
            q = np.ascontiguousarray(sphere_ior, np.float32).reshape(len(s))
            _check(lib().skr_scene_set_sphere_ior(sc.h, q.ctypes.data), "skr_scene_set_sphere_ior")
        if triangle_shadows:
            sc.set_triangle_shadows(True)
        if sphere_tree:
            sc.set_sphere_tree(True)
        if light_radii is not None:  # a scalar or [n_point_lights] (soft shadows)
            sc.set_light_radii(light_radii)
        if lens is not None:  # (aperture, focus) (depth of field)
            sc.set_lens(*lens)
        if velocities is not None:  # [n_spheres][3] (motion blur)
            sc.set_velocities(velocities)
        if shutter is not None:
            sc.set_shutter(shutter)
        if environment is not None:  # [E, E, 3] (an image-based background and GI light)
            sc.set_environment(environment)
        for t in (textures or ()):  # [E, E, 3] each, indexed in this order
            sc.add_texture(t)
        if sphere_textures is not None:  # one index per sphere, -1 = none
            sc.set_sphere_textures(sphere_textures)
        if emission is not None:  # [n_spheres, 3], >= 0
            sc.set_emission(emission)
        return sc


SCN_STRICT, SCN_FOG, SCN_TRIANGLE_SHADOWS, SCN_SPHERE_TREE, SCN_SPOT, SCN_MOTION, SCN_TEXTURE, SCN_EMISSION = 1, 2, 4, 8, 16, 32, 64, 128  # include/skr.h SKR_SCN_*
FOG_MAX_VOLUMES = 64        # include/skr.h SKR_FOG_MAX_VOLUMES
ENV_MAX_EDGE = 4096         # include/skr.h SKR_ENV_MAX_EDGE
TEX_MAX, TEX_MAX_EDGE = 16, 1024  # include/skr.h SKR_TEX_MAX, SKR_TEX_MAX_EDGE


def parse_scene(path, echo=False, strict=False, fog=False, triangle_shadows=False, sphere_tree=False, spot=False, motion=False, texture=False, emission=False):
    """Reference `Scene parseScene(std::string)` (scene.cpp:12); strict = SKR_SCN_STRICT (--strict-scn: directional lights kept),
    fog = SKR_SCN_FOG (--scn-fog: spherical_fog lines parsed and shaded), triangle_shadows = SKR_SCN_TRIANGLE_SHADOWS
    (--triangle-shadows: triangles cast shadows in frames with shade_triangles and shadow), sphere_tree = SKR_SCN_SPHERE_TREE
    (--sphere-tree: frames and shading queries on the culled sphere walk, any sphere count), spot = SKR_SCN_SPOT (--scn-spot: spot_light
    lines parsed and shaded), motion = SKR_SCN_MOTION (--scn-motion: velocity lines parsed, the spheres that follow move),
    texture = SKR_SCN_TEXTURE (--scn-texture: texture lines parsed, the spheres that follow carry the image),
    emission = SKR_SCN_EMISSION (--scn-emission: emission lines parsed, the spheres that follow glow)."""
    h = C.c_void_p()
    flags = (SCN_STRICT if strict else 0) | (SCN_FOG if fog else 0) | (SCN_TRIANGLE_SHADOWS if triangle_shadows else 0) | (SCN_SPHERE_TREE if sphere_tree else 0) | (SCN_SPOT if spot else 0) | (SCN_MOTION if motion else 0) | (SCN_TEXTURE if texture else 0) | (SCN_EMISSION if emission else 0)
    _check(lib().skr_scene_create_from_scn_ex(os.fsencode(path), int(echo), flags, C.byref(h)), "skr_scene_create_from_scn_ex")
    return Scene(h.value)


def scene_fov(scene):
    """--scn-fov: the field of view the camera line asks for, 2 x half_height_angle (exact in binary32)."""
    return float(np.float32(2) * np.float32(scene.info.camera[12]))


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    _check(lib().skr_write_ppm(os.fsencode(path), w, h, rgb.ctypes.data), "skr_write_ppm")


def write_png(path, rgb):
    """The bytes of the PPM as an 8-bit RGB PNG (include/skr.h skr_write_png)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    _check(lib().skr_write_png(os.fsencode(path), w, h, rgb.ctypes.data), "skr_write_png")


def write_pfm(path, rgbf):
    """The unquantised float frame [H, W, 3] (top row first) as a PFM file (include/skr.h skr_write_pfm)."""
    rgbf = np.ascontiguousarray(rgbf, np.float32)
    h, w, _ = rgbf.shape
    _check(lib().skr_write_pfm(os.fsencode(path), w, h, rgbf.ctypes.data), "skr_write_pfm")


def read_pfm(path):
    """A colour PFM file as float32 [H, W, 3], top row first: the inverse of write_pfm, bit for bit (include/skr.h skr_read_pfm)."""
    w, h = C.c_uint32(0), C.c_uint32(0)
    _check(lib().skr_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), None), "skr_read_pfm")
    a = np.zeros((h.value, w.value, 3), np.float32)
    _check(lib().skr_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), a.ctypes.data), "skr_read_pfm")
    return a


class Renderer:
    """Device context (scene resident in HBM) + the launches.  Needs a gfx950 GPU."""

    def __init__(self, scene, device=0):
        self.scene = scene
        self.device = device
        h = C.c_void_p()
        _check(lib().skr_renderer_create(scene.h, device, C.byref(h)), "skr_renderer_create")
        self.h = h
        self._env = self._switch_env()

    def clone(self):
        """skr_renderer_clone: a second renderer on the same uploaded scene with its own tables (a second frame in flight); it shares this
        renderer's work counters and must be closed before it."""
        other = Renderer.__new__(Renderer)
        other.scene, other.device, other._source = self.scene, self.device, self
        h = C.c_void_p()
        _check(lib().skr_renderer_clone(self.h, C.byref(h)), "skr_renderer_clone")
        other.h = h
        other._env = self._env
        return other

    @staticmethod
    def _switch_env():
        return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("SKR_")))

    def _sync_switches(self):
        """libskr reads its SKR_* development switches once per renderer; tests and A/B tools change them between
        frames, so the binding asks for a re-read when this process's environment has changed since."""
        env = self._switch_env()
        if env != self._env:
            _check(lib().skr_renderer_reload_switches(self.h), "skr_renderer_reload_switches")
            self._env = env

    def close(self):
        if getattr(self, "h", None):
            try:
                lib().skr_renderer_destroy(self.h)
            except TypeError:  # interpreter teardown: the module's globals are gone, the process is about to free everything
                pass
            self.h = None

    __del__ = close

    def tile_count(self, opt, tile_rows, first_tile=0, tile_stride=1):
        return int(lib().skr_tile_count(C.byref(opt.c), tile_rows, first_tile, tile_stride))

    def render_tiles_into(self, opt, tile_rows, first_tile, tile_stride, rgb_ptr, rgbf_ptr=None, stream=None):
        """Enqueue the kernels of this partition of the frame (skr_render_tiles); pointers are raw device addresses."""
        self._sync_switches()
        _check(lib().skr_render_tiles(self.h, C.byref(opt.c), tile_rows, first_tile, tile_stride, rgb_ptr, rgbf_ptr,
                                      stream), "skr_render_tiles")

    def render_tile_list_into(self, opt, tile_rows, tiles_ptr, n_slots, rgb_ptr, rgbf_ptr=None, stream=None):
        """skr_render_tile_list: slot k of the compact output holds tile tiles[k] (a device array of uint32; 0xFFFFFFFF = empty)."""
        self._sync_switches()
        _check(lib().skr_render_tile_list(self.h, C.byref(opt.c), tile_rows, tiles_ptr, n_slots, rgb_ptr, rgbf_ptr, stream), "skr_render_tile_list")

    def tile_costs(self, opt, tile_rows):
        """Per tile, its counted work in flops (include/skr.h skr_tile_costs)."""
        self._sync_switches()
        n = (opt.height + tile_rows - 1) // tile_rows
        out = np.zeros(n, np.uint64)
        _check(lib().skr_tile_costs(self.h, C.byref(opt.c), tile_rows, out.ctypes.data), "skr_tile_costs")
        return out

    def shard_plan(self, opt, tile_rows, world):
        """slot_of_tile of the map a frame step of `world` ranks uses (include/skr.h skr_shard_plan)."""
        n = (opt.height + tile_rows - 1) // tile_rows
        out = np.zeros(n, np.uint32)
        _check(lib().skr_shard_plan(self.h, C.byref(opt.c), tile_rows, world, out.ctypes.data), "skr_shard_plan")
        return out

    def render(self, opt, want_float=False, tile_rows=None, first_tile=0, tile_stride=1):
        """Render (a partition of) the frame into torch tensors on this device.  Returns
        (rgb uint8 [rows, W, 3], float32 image or None); rows are tile-major compact."""
        import torch
        dev = torch.device("cuda", self.device)
        tile_rows = tile_rows or opt.height
        n = self.tile_count(opt, tile_rows, first_tile, tile_stride)
        rows = n * tile_rows
        rgb = torch.zeros((rows, opt.width, 3), dtype=torch.uint8, device=dev)
        rgbf = torch.zeros((rows, opt.width, 3), dtype=torch.float32, device=dev) if want_float else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.render_tiles_into(opt, tile_rows, first_tile, tile_stride, rgb.data_ptr(),
                                   rgbf.data_ptr() if want_float else None, stream)
        return rgb, rgbf

    def render_rows(self, opt, y0, y1, want_float=False):
        import torch
        dev = torch.device("cuda", self.device)
        rgb = torch.zeros((y1 - y0, opt.width, 3), dtype=torch.uint8, device=dev)
        rgbf = torch.zeros((y1 - y0, opt.width, 3), dtype=torch.float32, device=dev) if want_float else None
        self._sync_switches()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib().skr_render_rows(self.h, C.byref(opt.c), y0, y1, rgb.data_ptr(),
                                         rgbf.data_ptr() if want_float else None, stream), "skr_render_rows")
        return rgb, rgbf

    def render_progressive_host(self, opt, every=0, want_float=False, progress=None):
        """include/skr.h skr_render_progressive_host: the whole frame (the mean of opt's progressive passes) into host arrays;
        progress(passes_done, passes, rgb, rgbf) is called after every `every` passes with the mean so far (views of the
        returned arrays; return True to stop).  Returns (rgb uint8 [H, W, 3], rgbf float32 or None, device ms)."""
        self._sync_switches()
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        rgbf = np.zeros((opt.height, opt.width, 3), np.float32) if want_float else None
        cb = PROGRESS_FN((lambda user, done, total, b, f: int(bool(progress(done, total, rgb, rgbf)))) if progress else (lambda *a: 0))
        ms = C.c_float()
        _check(lib().skr_render_progressive_host(self.h, C.byref(opt.c), every, rgb.ctypes.data, rgbf.ctypes.data if want_float else None,
                                                 cb if progress else PROGRESS_FN(), None, C.byref(ms)), "skr_render_progressive_host")
        return rgb, rgbf, ms.value

    def counters(self, reset=True):
        out = (C.c_uint64 * 3)()
        _check(lib().skr_renderer_read_counters(self.h, out, int(reset)), "skr_renderer_read_counters")
        return {"radiance_rays": int(out[0]), "sphere_hits": int(out[1]), "shadow_rays": int(out[2])}

    def work(self, reset=True):
        """counters() plus sphere_tests (include/skr.h skr_renderer_read_work)."""
        out = (C.c_uint64 * 4)()
        _check(lib().skr_renderer_read_work(self.h, out, int(reset)), "skr_renderer_read_work")
        return {"radiance_rays": int(out[0]), "sphere_hits": int(out[1]), "shadow_rays": int(out[2]), "sphere_tests": int(out[3])}

    def kernel_work(self):
        """work() of the one kernel kernel_ms() times, in the last launch made with kernel timing on (include/skr.h skr_renderer_kernel_work)."""
        out = (C.c_uint64 * 4)()
        _check(lib().skr_renderer_kernel_work(self.h, out), "skr_renderer_kernel_work")
        return {"radiance_rays": int(out[0]), "sphere_hits": int(out[1]), "shadow_rays": int(out[2]), "sphere_tests": int(out[3])}

    def count_triangle_work(self, enable=True):
        _check(lib().skr_renderer_count_triangle_work(self.h, int(enable)), "skr_renderer_count_triangle_work")

    def triangle_work(self, reset=True):
        """What the triangle walks executed (include/skr.h skr_renderer_read_triangle_work): call it BEFORE work(reset=True)."""
        out = (C.c_uint64 * 3)()
        _check(lib().skr_renderer_read_triangle_work(self.h, out, int(reset)), "skr_renderer_read_triangle_work")
        return {"cull_tests": int(out[0]), "triangle_tests": int(out[1]), "reference_triangle_tests": int(out[2])}

    def sphere_tree_work(self, reset=True):
        """What the sphere tree's walks executed while count_triangle_work was on (include/skr.h skr_renderer_read_sphere_tree_work)."""
        out = (C.c_uint64 * 2)()
        _check(lib().skr_renderer_read_sphere_tree_work(self.h, out, int(reset)), "skr_renderer_read_sphere_tree_work")
        return {"cull_tests": int(out[0]), "sphere_tests": int(out[1])}

    def kernel_timing(self, enable=True):
        _check(lib().skr_renderer_kernel_timing(self.h, int(enable)), "skr_renderer_kernel_timing")

    def kernel_ms(self):
        """(mean ms of the dominant kernel, number of launches) since the last call; synchronises."""
        ms, n = C.c_float(), C.c_int32()
        _check(lib().skr_renderer_kernel_ms(self.h, C.byref(ms), C.byref(n)), "skr_renderer_kernel_ms")
        return ms.value, n.value

    def last_parent_count(self):
        n = C.c_uint32()
        _check(lib().skr_renderer_last_parent_count(self.h, C.byref(n)), "skr_renderer_last_parent_count")
        return n.value

    def primary_cache_stats(self):
        """(builds, replays): how many frames of this renderer built the node pipeline's level-0 stage and how many reused it."""
        b, p = C.c_uint64(), C.c_uint64()
        _check(lib().skr_renderer_primary_cache_stats(self.h, C.byref(b), C.byref(p)), "skr_renderer_primary_cache_stats")
        return b.value, p.value

    def last_level1_count(self):
        n = C.c_uint32()
        _check(lib().skr_renderer_last_level1_count(self.h, C.byref(n)), "skr_renderer_last_level1_count")
        return n.value

    @staticmethod
    def kernel_variant():
        return (lib().skr_kernel_variant() or b"").decode()

    def trace(self, rays, any_hit=False):
        """Trace rays (float32 [n, 8] on this device, the include/skr.h skr_ray layout: make_rays) against the scene, on torch's
        current stream (include/skr.h skr_trace_rays).  Returns Hits(t, kind, index, normal): views of one float32 [n, 8] buffer in the
        skr_hit layout (t float32 [n], kind and index int32 [n], normal float32 [n, 3]); any_hit=True: int32 [n], 1 where the closest
        hit would not be a miss."""
        import torch
        dev = torch.device("cuda", self.device)
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or rays.device != dev:
            raise SkrError("trace: rays must be a float32 [n, 8] tensor on %s (make_rays)" % dev)
        rays = rays.contiguous()
        n = rays.shape[0]
        if n >= 1 << 32:
            raise SkrError("trace: at most 2^32 - 1 rays per call")
        out = torch.empty(n, dtype=torch.int32, device=dev) if any_hit else torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n == 0:  # (an empty tensor has no address to pass)
            return out if any_hit else Hits(out[:, 0], out.view(torch.int32)[:, 1], out.view(torch.int32)[:, 2], out[:, 3:6], out)
        self._sync_switches()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib().skr_trace_rays(self.h, rays.data_ptr(), n, TRACE_ANY_HIT if any_hit else 0, out.data_ptr(), stream), "skr_trace_rays")
        if any_hit:
            return out
        ints = out.view(torch.int32)
        return Hits(out[:, 0], ints[:, 1], ints[:, 2], out[:, 3:6], out)

    def camera_rays(self, opt, sample=0):
        """The primary rays of AA sample `sample` of a frame with options opt (include/skr.h skr_camera_rays): float32 [h, w, 8] on this
        device, on torch's current stream.  trace(camera_rays(opt).view(-1, 8)) gives the frame's depth, id and normal buffers."""
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty((opt.height, opt.width, 8), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib().skr_camera_rays(self.h, C.byref(opt.c), sample, out.data_ptr(), stream), "skr_camera_rays")
        return out

    def shade(self, rays, opt, sample=0, keys=None):
        """The radiance of rays (float32 [n, 8] on this device, the include/skr.h skr_ray layout: make_rays, camera_rays) under options
        opt, on torch's current stream (include/skr.h skr_shade_rays): float32 [n, 3], what shade() returns for each ray.  keys (int32 or
        uint32 [n] on this device; None = the ray index) and sample are the counter RNG's pixel and AA words of each ray, so
        shade(camera_rays(opt, s).view(-1, 8), opt, s, keys=y * width + x) is the frame's sample s, bit for bit."""
        import torch
        dev = torch.device("cuda", self.device)
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or rays.device != dev:
            raise SkrError("shade: rays must be a float32 [n, 8] tensor on %s (make_rays)" % dev)
        rays = rays.contiguous()
        n = rays.shape[0]
        if n >= 1 << 32:
            raise SkrError("shade: at most 2^32 - 1 rays per call")
        if keys is not None:
            if keys.dtype not in (torch.int32, torch.uint32) or keys.dim() != 1 or keys.shape[0] != n or keys.device != dev:
                raise SkrError("shade: keys must be an int32 or uint32 [%d] tensor on %s" % (n, dev))
            keys = keys.contiguous()
        if not 0 <= int(sample) < 1 << 32:
            raise SkrError("shade: sample must fit 32 bits")
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n == 0:  # (an empty tensor has no address to pass)
            return out
        self._sync_switches()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib().skr_shade_rays(self.h, C.byref(opt.c), rays.data_ptr(), n, int(sample), None if keys is None else keys.data_ptr(),
                                        out.data_ptr(), stream), "skr_shade_rays")
        return out

    def denoise(self, rgbf, hits, iterations=DENOISE_ITERATIONS, variance=None):
        """The edge-aware denoiser (include/skr.h skr_denoise) on torch's current stream: rgbf float32 [H, W, 3] on this device, hits the
        guides — a Hits or its float32 raw buffer ([H * W, 8] or [H, W, 8]) of the pixel-centre camera rays of the frame's options:
        r.trace(r.camera_rays(opt_with_grid_0).view(-1, 8)), with opt_with_grid_0 = opt with jsample 0.  Returns (rgb uint8 [H, W, 3],
        rgbf float32 [H, W, 3]) device tensors; iterations 0 .. 16, 0 = the input itself.  variance: a float32 [H, W] tensor of each pixel's
        measured variance of its mean luminance (render_adaptive(want_variance=True)), taken in place of the spatial estimate wherever it
        is >= 0 (include/skr.h skr_denoise_var); None: the spatial estimate everywhere."""
        import torch
        dev = torch.device("cuda", self.device)
        if rgbf.dtype != torch.float32 or rgbf.dim() != 3 or rgbf.shape[2] != 3 or rgbf.device != dev:
            raise SkrError("denoise: rgbf must be a float32 [H, W, 3] tensor on %s" % dev)
        h, w = int(rgbf.shape[0]), int(rgbf.shape[1])
        raw = hits.raw if isinstance(hits, Hits) else hits
        if raw.dtype != torch.float32 or raw.device != dev or raw.numel() != h * w * 8:
            raise SkrError("denoise: hits must be the [%d, 8] float32 guides of the frame on %s (Renderer.trace)" % (h * w, dev))
        if variance is not None and (variance.dtype != torch.float32 or variance.device != dev or tuple(variance.shape) != (h, w)):
            raise SkrError("denoise: variance must be a float32 [%d, %d] tensor on %s" % (h, w, dev))
        rgbf, raw = rgbf.contiguous(), raw.contiguous()
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if variance is None:
                _check(lib().skr_denoise(self.h, w, h, rgbf.data_ptr(), raw.data_ptr(), int(iterations), out.data_ptr(), rgb.data_ptr(), stream), "skr_denoise")
            else:
                variance = variance.contiguous()
                _check(lib().skr_denoise_var(self.h, w, h, rgbf.data_ptr(), raw.data_ptr(), variance.data_ptr(), int(iterations), out.data_ptr(), rgb.data_ptr(),
                                             stream), "skr_denoise_var")
        return rgb, out

    def render_adaptive(self, opt, threshold=ADAPTIVE_THRESHOLD, min_passes=ADAPTIVE_MIN_PASSES, max_passes=ADAPTIVE_MAX_PASSES, want_float=False,
                        want_variance=False):
        """Adaptive sampling (include/skr.h skr_render_adaptive): every pixel gets min_passes passes of opt (seeds seed, seed+1, ...) and
        more, up to max_passes, while the standard error of its mean luminance exceeds threshold x that mean.  Returns (rgb uint8
        [H, W, 3], rgbf float32 [H, W, 3] or None, passes uint32 [H, W]) device tensors, written on torch's current stream; the call
        itself is synchronous (one 4-byte count is read back per round).  min_passes == max_passes == K is render(opt with progressive=K).
        want_variance: a fourth tensor is appended, float32 [H, W], the variance of each pixel's mean luminance (-1 where it had fewer
        than two passes): what denoise(variance=...) takes (include/skr.h skr_render_adaptive_var)."""
        import torch
        dev = torch.device("cuda", self.device)
        a = adaptive_params(threshold, min_passes, max_passes)
        rgb = torch.zeros((opt.height, opt.width, 3), dtype=torch.uint8, device=dev)
        rgbf = torch.zeros((opt.height, opt.width, 3), dtype=torch.float32, device=dev) if want_float else None
        passes = torch.empty((opt.height, opt.width), dtype=torch.uint32, device=dev)  # (every word is written)
        self._sync_switches()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if want_variance:
                var = torch.empty((opt.height, opt.width), dtype=torch.float32, device=dev)  # (every word is written)
                _check(lib().skr_render_adaptive_var(self.h, C.byref(opt.c), C.byref(a), rgb.data_ptr(), rgbf.data_ptr() if want_float else None,
                                                     passes.data_ptr(), var.data_ptr(), stream), "skr_render_adaptive_var")
                return rgb, rgbf, passes, var
            _check(lib().skr_render_adaptive(self.h, C.byref(opt.c), C.byref(a), rgb.data_ptr(), rgbf.data_ptr() if want_float else None,
                                             passes.data_ptr(), stream), "skr_render_adaptive")
        return rgb, rgbf, passes

    def render_adaptive_host(self, opt, threshold=ADAPTIVE_THRESHOLD, min_passes=ADAPTIVE_MIN_PASSES, max_passes=ADAPTIVE_MAX_PASSES, want_float=False):
        """render_adaptive into host arrays (include/skr.h skr_render_adaptive_host).  Returns (rgb uint8 [H, W, 3], rgbf float32 or
        None, passes uint32 [H, W], device ms)."""
        a = adaptive_params(threshold, min_passes, max_passes)
        self._sync_switches()
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        rgbf = np.zeros((opt.height, opt.width, 3), np.float32) if want_float else None
        passes = np.zeros((opt.height, opt.width), np.uint32)
        ms = C.c_float()
        _check(lib().skr_render_adaptive_host(self.h, C.byref(opt.c), C.byref(a), rgb.ctypes.data, rgbf.ctypes.data if want_float else None,
                                              passes.ctypes.data, C.byref(ms)), "skr_render_adaptive_host")
        return rgb, rgbf, passes, ms.value

    def render_adaptive_denoised(self, opt, threshold=ADAPTIVE_THRESHOLD, min_passes=ADAPTIVE_MIN_PASSES, max_passes=ADAPTIVE_MAX_PASSES,
                                 iterations=DENOISE_ITERATIONS, want_float=False):
        """include/skr.h skr_render_adaptive_denoised_host: the adaptive frame with its measured variance, its guides and the denoiser under
        that variance, into host arrays.  Returns (rgb uint8 [H, W, 3], rgbf float32 or None, passes uint32 [H, W], device ms); the same
        bits as render_adaptive(..., want_float=True, want_variance=True), then denoise(rgbf, trace(camera_rays(opt with jsample 0)
        .view(-1, 8)), iterations, variance)."""
        a = adaptive_params(threshold, min_passes, max_passes)
        self._sync_switches()
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        rgbf = np.zeros((opt.height, opt.width, 3), np.float32) if want_float else None
        passes = np.zeros((opt.height, opt.width), np.uint32)
        ms = C.c_float()
        _check(lib().skr_render_adaptive_denoised_host(self.h, C.byref(opt.c), C.byref(a), int(iterations), rgb.ctypes.data,
                                                       rgbf.ctypes.data if want_float else None, passes.ctypes.data, C.byref(ms)),
               "skr_render_adaptive_denoised_host")
        return rgb, rgbf, passes, ms.value

    def render_denoised(self, opt, iterations=DENOISE_ITERATIONS, want_float=False):
        """include/skr.h skr_render_denoised_host: the whole frame (the mean of opt's progressive passes), its guides and the denoiser,
        into host arrays.  Returns (rgb uint8 [H, W, 3], rgbf float32 or None, device ms); the same bits as render(opt, want_float=True),
        then denoise(rgbf, trace(camera_rays(opt with jsample 0).view(-1, 8)), iterations)."""
        self._sync_switches()
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        rgbf = np.zeros((opt.height, opt.width, 3), np.float32) if want_float else None
        ms = C.c_float()
        _check(lib().skr_render_denoised_host(self.h, C.byref(opt.c), int(iterations), rgb.ctypes.data, rgbf.ctypes.data if want_float else None,
                                              C.byref(ms)), "skr_render_denoised_host")
        return rgb, rgbf, ms.value


TRACE_ANY_HIT = 1  # include/skr.h SKR_TRACE_ANY_HIT


class Hits:
    """The result of Renderer.trace: views of one float32 [n, 8] buffer `raw` in the include/skr.h skr_hit layout."""

    def __init__(self, t, kind, index, normal, raw):
        self.t, self.kind, self.index, self.normal, self.raw = t, kind, index, normal, raw

    def __iter__(self):
        return iter((self.t, self.kind, self.index, self.normal))


def make_rays(origins, directions, tmax=None, ignore_triangle=None, device=None):
    """Pack rays into a CUDA float32 [n, 8] tensor in the include/skr.h skr_ray layout: origins and directions [n, 3] (tensors or
    arrays); tmax (scalar or [n]; None = +inf: no limit); ignore_triangle (scalar or [n] file indices; None = -1: none).  The tensor
    lives on `device` (default: the origins' CUDA device, else the current one)."""
    import torch
    if device is None:
        device = origins.device if isinstance(origins, torch.Tensor) and origins.is_cuda else torch.device("cuda", torch.cuda.current_device())
    o = torch.as_tensor(origins, dtype=torch.float32, device=device).reshape(-1, 3)
    d = torch.as_tensor(directions, dtype=torch.float32, device=device).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise SkrError("make_rays: %d origins and %d directions" % (n, d.shape[0]))
    rays = torch.empty((n, 8), dtype=torch.float32, device=device)
    rays[:, 0:3] = o
    rays[:, 3] = float("inf") if tmax is None else torch.as_tensor(tmax, dtype=torch.float32, device=device).expand(n)
    rays[:, 4:7] = d
    ign = -1 if ignore_triangle is None else torch.as_tensor(ignore_triangle, dtype=torch.int32, device=device).expand(n)
    rays.view(torch.int32)[:, 7] = ign
    return rays


COMM_ID_BYTES = 128


def rccl_available():
    return bool(lib().skr_rccl_available())


def comm_unique_id():
    """An RCCL id (rank 0 makes it; the caller broadcasts the 128 bytes by whatever transport it has)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().skr_comm_unique_id(buf), "skr_comm_unique_id")
    return bytes(buf)


class Comm:
    """One rank of the native frame step (include/skr.h skr_comm_*): this rank's tiles, ONE RCCL all-gather, rank 0's
    de-interleave on the device — all inside libskr, enqueued on the caller's stream."""

    def __init__(self, renderer, rank, world, unique_id=None):
        self.renderer, self.rank, self.world = renderer, rank, world
        h = C.c_void_p()
        idbuf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
        _check(lib().skr_comm_create(renderer.h, renderer.device, idbuf, rank, world, C.byref(h)), "skr_comm_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            try:
                lib().skr_comm_destroy(self.h)
            except TypeError:  # (interpreter teardown)
                pass
            self.h = None

    __del__ = close

    def render_frame(self, opt, tile_rows, stream=None):
        """Enqueue one frame; returns the device address of rank 0's finished frame (None on the other ranks)."""
        self.renderer._sync_switches()
        d = C.c_void_p()
        _check(lib().skr_comm_render_frame(self.h, C.byref(opt.c), tile_rows, C.byref(d), stream), "skr_comm_render_frame")
        return d.value

    def render_frame_async(self, opt, tile_rows, stream=None, want_previous=True):
        """Enqueue one frame with its collective on the communicator's own stream (include/skr.h skr_comm_render_frame_async);
        returns the device address of the PREVIOUS call's frame (rank 0; None on the first call, on the other ranks, and when not asked for)."""
        self.renderer._sync_switches()
        d = C.c_void_p()
        _check(lib().skr_comm_render_frame_async(self.h, C.byref(opt.c), tile_rows, C.byref(d) if want_previous else None, stream), "skr_comm_render_frame_async")
        return d.value

    def flush(self, stream=None):
        """Ends a run of render_frame_async calls: `stream` waits for the last collective; returns the last frame's address (rank 0)."""
        d = C.c_void_p()
        _check(lib().skr_comm_flush(self.h, C.byref(d), stream), "skr_comm_flush")
        return d.value

    def frame_to_host(self, opt, stream=None):
        """Rank 0: the frame of the last render_frame as a numpy array (waits for the stream)."""
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        _check(lib().skr_comm_frame_to_host(self.h, rgb.ctypes.data, stream), "skr_comm_frame_to_host")
        return rgb


class Multi:
    """One process, N devices (include/skr.h skr_multi_*)."""

    def __init__(self, scene, n_devices):
        h = C.c_void_p()
        _check(lib().skr_multi_create(scene.h, n_devices, None, C.byref(h)), "skr_multi_create")
        self.h, self.n = h, n_devices

    def close(self):
        if getattr(self, "h", None):
            try:
                lib().skr_multi_destroy(self.h)
            except TypeError:  # (interpreter teardown)
                pass
            self.h = None

    __del__ = close

    def render_frame_host(self, opt, tile_rows=8):
        rgb = np.zeros((opt.height, opt.width, 3), np.uint8)
        ms = C.c_float()
        _check(lib().skr_multi_render_frame_host(self.h, C.byref(opt.c), tile_rows, rgb.ctypes.data, C.byref(ms)), "skr_multi_render_frame_host")
        return rgb, ms.value

    def render_frame_async(self, opt, tile_rows=8, want_previous=True):
        """skr_multi_render_frame_async: returns the device address of the PREVIOUS call's frame (0 on the first call)."""
        prev = C.c_void_p()
        _check(lib().skr_multi_render_frame_async(self.h, C.byref(opt.c), tile_rows, C.byref(prev) if want_previous else None), "skr_multi_render_frame_async")
        return prev.value or 0

    def flush(self):
        last = C.c_void_p()
        _check(lib().skr_multi_flush(self.h, C.byref(last)), "skr_multi_flush")
        return last.value or 0

    def counters(self, reset=True):
        tot = {"radiance_rays": 0, "sphere_hits": 0, "shadow_rays": 0}
        for i in range(self.n):
            out = (C.c_uint64 * 3)()
            _check(lib().skr_renderer_read_counters(lib().skr_multi_renderer(self.h, i), out, int(reset)), "skr_renderer_read_counters")
            for k, name in enumerate(tot):
                tot[name] += int(out[k])
        return tot


def shard_tiles_per_rank(height, tile_rows, world):
    return int(lib().skr_shard_tiles_per_rank(height, tile_rows, world))


def shard_lpt(cost, world):
    """The cost-aware map: slot_of_tile[t] = rank * k_max + slot (include/skr.h skr_shard_lpt)."""
    c = np.ascontiguousarray(cost, np.uint64)
    out = np.zeros(len(c), np.uint32)
    _check(lib().skr_shard_lpt(c.ctypes.data, len(c), world, out.ctypes.data), "skr_shard_lpt")
    return out


def shard_by_cost(cost, world):
    """The frame steps' rule on given costs: `t mod world` unless that is more than 10 % off balance, then LPT (include/skr.h skr_shard_by_cost)."""
    c = np.ascontiguousarray(cost, np.uint64)
    out = np.zeros(len(c), np.uint32)
    _check(lib().skr_shard_by_cost(c.ctypes.data, len(c), world, out.ctypes.data), "skr_shard_by_cost")
    return out


def shard_deinterleave_map_host(gathered, width, height, tile_rows, slot_of_tile):
    g = np.ascontiguousarray(gathered, np.uint8)
    m = np.ascontiguousarray(slot_of_tile, np.uint32)
    out = np.zeros((height, width, 3), np.uint8)
    _check(lib().skr_shard_deinterleave_map_host(g.ctypes.data, out.ctypes.data, width, height, tile_rows, m.ctypes.data), "skr_shard_deinterleave_map_host")
    return out


def shard_deinterleave_host(gathered, width, height, tile_rows, world):
    g = np.ascontiguousarray(gathered, np.uint8)
    out = np.zeros((height, width, 3), np.uint8)
    _check(lib().skr_shard_deinterleave_host(g.ctypes.data, out.ctypes.data, width, height, tile_rows, world), "skr_shard_deinterleave_host")
    return out


def debug_eval(op, inp, out_words_per_record, device=0, n=None):
    """Run the arithmetic-spec debug kernel on n records (uint32 words).  n: the record count where the input is not one row per
    record (ops 15 and 16 of include/skr.h: a scene, then the records); by default the rows of `inp`."""
    import torch
    dev = torch.device("cuda", device)
    a = torch.from_numpy(np.ascontiguousarray(inp).view(np.uint32).astype(np.int64)).to(torch.int64)
    a = a.to(dev).to(torch.int32).contiguous()  # same bits as uint32
    n = a.shape[0] if n is None else int(n)
    o = torch.zeros((n, out_words_per_record), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().skr_debug_eval(op, a.data_ptr(), o.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream),
               "skr_debug_eval")
    torch.cuda.synchronize(dev)
    return o.cpu().numpy().view(np.uint32)

"""ctypes mirror of include/simplepath_hip.h (the C-ABI boundary).

Only plain pointers and sizes cross the boundary.  The library is built in-tree
(simplepath_amd/_build/libsimplepath_hip.so); importing this module fails loudly when it is
missing -- there is no CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SP_LIB_PATH: an alternative build of the same library (experiments, e.g. compile-time variants)
LIB_PATH = os.environ.get("SP_LIB_PATH") or os.path.join(_HERE, "_build", "libsimplepath_hip.so")

SP_OK = 0
SP_ERR_PARSE, SP_ERR_IO, SP_ERR_ARG, SP_ERR_HIP, SP_ERR_UNSUPPORTED, SP_ERR_STATE = -1, -2, -3, -4, -5, -6

INTEGRATORS = {
    "mandelbrot": 1,
    "brute_force": 2,
    "brute_force_iterative": 3,
    "brute_force_iterative_rr": 4,
    "iterative_rrnee": 5,
    "direct_lighting": 6,
    "whitted": 7,
}


class sp_affine(C.Structure):
    _fields_ = [("vx", C.c_float * 3), ("vy", C.c_float * 3), ("vz", C.c_float * 3), ("p", C.c_float * 3)]


class sp_linear(C.Structure):
    _fields_ = [("vx", C.c_float * 3), ("vy", C.c_float * 3), ("vz", C.c_float * 3)]


class sp_material_desc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("base", C.c_int32),
        ("lambert_albedo", C.c_float * 3), ("microfacet_r", C.c_float * 3),
        ("alpha_x", C.c_float), ("alpha_y", C.c_float), ("microfacet_ior", C.c_float),
        ("sample_visible_area", C.c_int32), ("coat_ior", C.c_float), ("coat_color", C.c_float * 3),
    ]


class sp_xform_shape(C.Structure):
    _fields_ = [("object_to_world", sp_affine), ("world_to_object", sp_affine),
                ("normal_to_world", sp_linear), ("material", C.c_int32), ("kind", C.c_int32)]


class sp_light_desc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("image", C.c_int32), ("radiance", C.c_float * 3),
                ("object_to_world", sp_affine), ("world_to_object", sp_affine),
                ("normal_to_world", sp_linear)]


class sp_env_image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pixels", C.POINTER(C.c_float)),
                ("max_radiance", C.c_float), ("reserved", C.c_int32),
                ("light_to_world", sp_linear), ("world_to_light", sp_linear)]


class sp_camera_desc(C.Structure):
    _fields_ = [("transform", sp_affine), ("film_width", C.c_int32), ("film_height", C.c_int32)]


class sp_scene_info(C.Structure):
    _fields_ = [
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("russian_roulette_depth", C.c_int32), ("max_depth", C.c_int32),
        ("integrator_type", C.c_int32), ("num_triangles", C.c_int32), ("num_vertices", C.c_int32),
        ("num_shapes", C.c_int32), ("num_lights", C.c_int32), ("num_materials", C.c_int32),
        ("output_file_name", C.c_char * 256),
    ]


class sp_scene_desc(C.Structure):
    _fields_ = [
        ("info", sp_scene_info), ("camera", sp_camera_desc),
        ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
        ("indices", C.POINTER(C.c_uint32)), ("tri_material", C.POINTER(C.c_int32)),
        ("shapes", C.POINTER(sp_xform_shape)),
        ("prim_kind", C.POINTER(C.c_int32)), ("prim_index", C.POINTER(C.c_int32)), ("num_prims", C.c_int64),
        ("lights", C.POINTER(sp_light_desc)), ("materials", C.POINTER(sp_material_desc)),
        ("env_images", C.POINTER(sp_env_image)), ("num_env_images", C.c_int32), ("reserved", C.c_int32),
    ]


class sp_render_params(C.Structure):
    _fields_ = [
        ("integrator", C.c_int32), ("samples_per_pixel", C.c_uint32),
        ("tile_ids", C.POINTER(C.c_int32)), ("num_tiles", C.c_int64),
        ("stream", C.c_void_p), ("bvh_mode", C.c_int32), ("flags", C.c_int32),
        # ABI 4
        ("d_tile_ids", C.c_void_p), ("waves_per_simd", C.c_int32), ("chunks_per_pixel", C.c_int32),
        ("chunk_max_gb", C.c_float),
        # ABI 5
        ("tile_order_factor", C.c_float),
        # ABI 6
        ("tail_fraction", C.c_float), ("reserved", C.c_int32),
    ]


SP_WALK_AUTO, SP_WALK_STACKLESS = 0, 1


class sp_upload_params(C.Structure):
    _fields_ = [("bvh_mode", C.c_int32), ("walk", C.c_int32), ("stack_max_levels", C.c_int32),
                ("no_wide_bvh", C.c_int32), ("env_replay", C.c_int32), ("sah_leaf", C.c_int32),
                ("binary_closest", C.c_int32), ("reserved", C.c_int32)]


class sp_render_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("samples", C.c_uint64),
                ("rng_draws", C.c_uint64), ("kernel_ms", C.c_float), ("pipeline", C.c_int32),
                ("launches", C.c_int32), ("primary_hits", C.c_uint64), ("stage_ms", C.c_float * 4),
                ("parts", C.c_int32), ("stack_depth", C.c_int32), ("tail_tiles", C.c_int32), ("tail_chunks", C.c_int32)]


class sp_bvh_info(C.Structure):
    _fields_ = [("depth", C.c_int32), ("wide_depth", C.c_int32), ("light_depth", C.c_int32),
                ("stack_depth", C.c_int32), ("nodes", C.c_int64), ("slots", C.c_int64)]


SP_BUILDER_AUTO, SP_BUILDER_HOST, SP_BUILDER_DEVICE, SP_BUILDER_DEVICE_SAH = 0, 1, 2, 4
BUILDERS = {"auto": SP_BUILDER_AUTO, "host": SP_BUILDER_HOST, "device": SP_BUILDER_DEVICE,
            "device_sah": SP_BUILDER_DEVICE_SAH}


class sp_build_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32), ("reserved", C.c_int32 * 2)]


SP_FINISH_AUTO, SP_FINISH_HOST, SP_FINISH_DEVICE = 0, 1, 2
FINISHES = {"auto": SP_FINISH_AUTO, "host": SP_FINISH_HOST, "device": SP_FINISH_DEVICE}


class sp_build_params_ex(C.Structure):
    """sp_build_params with the finish behind it; the library tells the two apart by struct_size"""
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32), ("reserved", C.c_int32 * 2),
                ("finish", C.c_int32), ("reserved2", C.c_int32 * 3)]


class sp_wide_check(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("finish", C.c_int32),
                ("records", C.c_int64), ("holes", C.c_int64), ("slots", C.c_int64),
                ("depth", C.c_int32), ("reserved", C.c_int32), ("errors", C.c_int64),
                ("first_error_kind", C.c_int32), ("reserved2", C.c_int32), ("first_error_node", C.c_int64),
                ("hash_nodes", C.c_uint64), ("hash_records", C.c_uint64), ("hash_parents", C.c_uint64)]


class sp_bvh_check(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32),
                ("nodes", C.c_int64), ("leaves", C.c_int64), ("slots", C.c_int64),
                ("depth", C.c_int32), ("max_leaf", C.c_int32), ("errors", C.c_int64),
                ("first_error_kind", C.c_int32), ("reserved", C.c_int32), ("first_error_node", C.c_int64),
                ("hash", C.c_uint64)]


class sp_mesh_update(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32),
                ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("num_vertices", C.c_int64), ("reserved", C.c_int32 * 4)]


class sp_refit_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("refitted", C.c_int32),
                ("binary_passes", C.c_int32), ("wide_passes", C.c_int32),
                ("ms_copy", C.c_float), ("ms_pack", C.c_float), ("ms_binary", C.c_float), ("ms_wide", C.c_float),
                ("ms_total", C.c_float), ("scratch_bytes", C.c_int64)]


class sp_env_update(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("image", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("pixels", C.POINTER(C.c_float)), ("d_pixels", C.c_void_p),
                ("max_radiance", C.c_float), ("reserved0", C.c_int32),
                ("light_to_world", sp_linear), ("world_to_light", sp_linear), ("reserved", C.c_int32 * 4)]


class sp_env_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rebuilt", C.c_int32), ("guided", C.c_int32), ("reserved", C.c_int32),
                ("ms_upload", C.c_float), ("ms_clamp", C.c_float), ("ms_func", C.c_float), ("ms_rows", C.c_float),
                ("ms_marginal", C.c_float), ("ms_guides", C.c_float), ("ms_total", C.c_float), ("reserved2", C.c_int32),
                ("scratch_bytes", C.c_int64)]


ENV_TABLES = ("radiance", "cond_func", "cond_cdf", "cond_int", "marg_func", "marg_cdf", "cond_guide", "marg_guide")
SP_ENV_SCALARS = 8
SP_ENV_BUILDER_HOST, SP_ENV_BUILDER_DEVICE = 0, 1
ENV_BUILDERS = {"host": SP_ENV_BUILDER_HOST, "device": SP_ENV_BUILDER_DEVICE}


class sp_env_check(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("nu", C.c_int32), ("nv", C.c_int32),
                ("guided", C.c_int32), ("cond_bits", C.c_int32), ("marg_bits", C.c_int32), ("marg_int_bits", C.c_uint32),
                ("mismatches", C.c_int64), ("first_table", C.c_int32), ("reserved", C.c_int32),
                ("first_index", C.c_int64), ("hash", C.c_uint64 * 10)]


SP_QUERY_CLOSEST, SP_QUERY_ANY = 0, 1
QUERY_MODES = {"closest": SP_QUERY_CLOSEST, "any": SP_QUERY_ANY}


class sp_ray(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("tmin", C.c_float), ("d", C.c_float * 3), ("tmax", C.c_float)]


class sp_ray_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("kind", C.c_int32), ("index", C.c_int32), ("material", C.c_int32),
                ("beta", C.c_float), ("gamma", C.c_float), ("reserved", C.c_uint32 * 2)]


class sp_ray_query(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32),
                ("d_rays", C.c_void_p), ("num_rays", C.c_int64), ("stream", C.c_void_p),
                ("d_hits", C.c_void_p), ("d_normals", C.c_void_p), ("d_occluded", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class sp_ray_query_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_int32), ("rays", C.c_uint64), ("hits", C.c_uint64),
                ("kernel_ms", C.c_float), ("stack_depth", C.c_int32)]


class sp_view_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("integrator", C.c_int32), ("samples_per_pixel", C.c_uint32),
                ("num_views", C.c_int32), ("cameras", C.POINTER(sp_camera_desc)), ("d_cameras", C.c_void_p),
                ("tile_ids", C.POINTER(C.c_int32)), ("d_tile_ids", C.c_void_p), ("num_tiles", C.c_int64),
                ("stream", C.c_void_p), ("waves_per_simd", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class sp_radiance_ray(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("seed", C.c_uint32), ("d", C.c_float * 3), ("reserved", C.c_uint32)]


class sp_radiance_query(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("integrator", C.c_int32), ("d_rays", C.c_void_p), ("num_rays", C.c_int64),
                ("samples_per_ray", C.c_uint32), ("waves_per_simd", C.c_int32), ("flags", C.c_int32),
                ("reserved0", C.c_int32), ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class sp_camera_ray_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("first_sample", C.c_uint32), ("num_samples", C.c_uint32),
                ("reserved0", C.c_int32), ("tile_ids", C.POINTER(C.c_int32)), ("d_tile_ids", C.c_void_p),
                ("num_tiles", C.c_int64), ("camera", C.POINTER(sp_camera_desc)), ("stream", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class sp_feature_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samples_per_pixel", C.c_uint32),
                ("tile_ids", C.POINTER(C.c_int32)), ("d_tile_ids", C.c_void_p), ("num_tiles", C.c_int64),
                ("tile_samples", C.POINTER(C.c_uint32)), ("d_tile_samples", C.c_void_p),
                ("camera", C.POINTER(sp_camera_desc)), ("stream", C.c_void_p),
                ("d_ids", C.c_void_p), ("d_coverage", C.c_void_p), ("d_depth", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_albedo", C.c_void_p), ("reserved", C.c_int32 * 4)]


class sp_feature_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_int32), ("camera_rays", C.c_uint64), ("hits", C.c_uint64),
                ("kernel_ms", C.c_float), ("stack_depth", C.c_int32)]


class sp_denoiser_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("tile_ids", C.POINTER(C.c_int32)), ("d_tile_ids", C.c_void_p), ("num_tiles", C.c_int64),
                ("reserved", C.c_int32 * 4)]


SP_DENOISE_DEMODULATE = 1


class sp_denoise_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("flags", C.c_int32), ("reserved0", C.c_int32),
                ("d_color", C.c_void_p), ("d_albedo", C.c_void_p), ("d_normal", C.c_void_p), ("d_depth", C.c_void_p),
                ("d_coverage", C.c_void_p), ("d_out", C.c_void_p),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_coverage", C.c_float), ("albedo_floor", C.c_float), ("depth_floor", C.c_float),
                ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class sp_denoise_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_int32), ("pixels", C.c_uint64), ("taps", C.c_uint64),
                ("kernel_ms", C.c_float), ("reserved", C.c_int32)]


class sp_progress_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("integrator", C.c_int32),
                ("tile_ids", C.POINTER(C.c_int32)), ("d_tile_ids", C.c_void_p), ("num_tiles", C.c_int64),
                ("waves_per_simd", C.c_int32), ("tile_order_factor", C.c_float), ("reserved", C.c_int32 * 2)]


class sp_pixel_state(C.Structure):
    _fields_ = [("mt", C.c_uint64 * 312), ("mt_pos", C.c_uint64), ("draws", C.c_uint64),
                ("sum", C.c_float * 3), ("reserved", C.c_uint32)]


class sp_adaptive_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_float), ("min_samples", C.c_uint32),
                ("max_samples", C.c_uint32), ("step", C.c_uint32), ("floor", C.c_float), ("reserved", C.c_uint32 * 2)]


class sp_adaptive_result(C.Structure):
    _fields_ = [("active_tiles", C.c_int64), ("samples_total", C.c_uint64), ("min_done", C.c_uint32),
                ("max_done", C.c_uint32), ("max_error", C.c_float), ("reserved", C.c_uint32)]


class sp_pixel_noise(C.Structure):
    _fields_ = [("mean", C.c_float), ("m2", C.c_float)]


# Every symbol declared in include/simplepath_hip.h, with its ctypes signature.
SIGNATURES = {
    "sp_progress_create_adaptive": (C.c_int, [C.c_void_p, C.POINTER(sp_progress_params), C.POINTER(C.c_void_p)]),
    "sp_adaptive_round": (C.c_int, [C.c_void_p, C.POINTER(sp_adaptive_params), C.c_void_p, C.c_void_p,
                                    C.POINTER(sp_render_stats), C.POINTER(sp_adaptive_result)]),
    "sp_adaptive_round_host": (C.c_int, [C.c_void_p, C.POINTER(sp_adaptive_params), C.POINTER(C.c_float),
                                         C.POINTER(sp_render_stats), C.POINTER(sp_adaptive_result)]),
    "sp_adaptive_tile_samples": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]),
    "sp_adaptive_tile_errors": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_int64]),
    "sp_adaptive_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint32), C.c_int64]),
    "sp_adaptive_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint32), C.c_int64]),
    "sp_progress_create": (C.c_int, [C.c_void_p, C.POINTER(sp_progress_params), C.POINTER(C.c_void_p)]),
    "sp_progress_free": (None, [C.c_void_p]),
    "sp_progress_render": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(sp_render_stats)]),
    "sp_progress_render_host": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(sp_render_stats)]),
    "sp_progress_samples": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "sp_progress_device_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "sp_progress_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint32)]),
    "sp_progress_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32]),
    "sp_version": (C.c_char_p, []),
    "sp_build_id": (C.c_char_p, []),
    "sp_last_error": (C.c_char_p, []),
    "sp_string_to_integrator": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32)]),
    "sp_scene_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "sp_scene_load_string": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "sp_scene_from_desc": (C.c_int, [C.POINTER(sp_scene_desc), C.POINTER(C.c_void_p)]),
    "sp_scene_free": (None, [C.c_void_p]),
    "sp_scene_get_info": (C.c_int, [C.c_void_p, C.POINTER(sp_scene_info)]),
    "sp_scene_get_desc": (C.c_int, [C.c_void_p, C.POINTER(sp_scene_desc)]),
    "sp_scene_set_resolution": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "sp_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                    C.c_int32, C.c_int32, C.POINTER(sp_camera_desc)]),
    "sp_scene_set_camera": (C.c_int, [C.c_void_p, C.POINTER(sp_camera_desc)]),
    "sp_render_views": (C.c_int, [C.c_void_p, C.POINTER(sp_view_params), C.c_void_p, C.POINTER(sp_render_stats)]),
    "sp_render_views_host": (C.c_int, [C.c_void_p, C.POINTER(sp_view_params), C.POINTER(C.c_float),
                                       C.POINTER(sp_render_stats)]),
    "sp_tile_count": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "sp_tile_origin": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sp_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "sp_scene_upload": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "sp_scene_upload_ex": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(sp_upload_params)]),
    "sp_scene_upload_with": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(sp_upload_params), C.POINTER(sp_build_params)]),
    "sp_scene_bvh_check": (C.c_int, [C.c_void_p, C.POINTER(sp_bvh_check)]),
    "sp_scene_bvh_build_check": (C.c_int, [C.c_void_p, C.POINTER(sp_upload_params), C.POINTER(sp_build_params),
                                           C.POINTER(sp_bvh_check)]),
    "sp_scene_wide_check": (C.c_int, [C.c_void_p, C.POINTER(sp_wide_check)]),
    "sp_scene_wide_build_check": (C.c_int, [C.c_void_p, C.POINTER(sp_upload_params), C.c_void_p, C.POINTER(sp_wide_check)]),
    "sp_scene_update_mesh": (C.c_int, [C.c_void_p, C.POINTER(sp_mesh_update), C.POINTER(sp_refit_stats)]),
    "sp_scene_refit_build_check": (C.c_int, [C.c_void_p, C.POINTER(sp_upload_params), C.POINTER(sp_build_params),
                                             C.POINTER(sp_mesh_update), C.POINTER(sp_bvh_check), C.POINTER(sp_wide_check)]),
    "sp_scene_set_materials": (C.c_int, [C.c_void_p, C.POINTER(sp_material_desc), C.c_int32]),
    "sp_scene_set_lights": (C.c_int, [C.c_void_p, C.POINTER(sp_light_desc), C.c_int32]),
    "sp_scene_set_env_image": (C.c_int, [C.c_void_p, C.POINTER(sp_env_update), C.POINTER(sp_env_stats)]),
    "sp_scene_env_check": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(sp_env_check)]),
    "sp_scene_env_build_check": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(sp_env_check)]),
    "sp_scene_trace_rays": (C.c_int, [C.c_void_p, C.POINTER(sp_ray_query), C.POINTER(sp_ray_query_stats)]),
    "sp_scene_trace_rays_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(sp_ray_query_stats)]),
    "sp_scene_radiance_rays": (C.c_int, [C.c_void_p, C.POINTER(sp_radiance_query), C.c_void_p, C.POINTER(sp_render_stats)]),
    "sp_scene_radiance_rays_host": (C.c_int, [C.c_void_p, C.POINTER(sp_radiance_query), C.c_void_p, C.c_void_p,
                                              C.POINTER(sp_render_stats)]),
    "sp_scene_camera_rays": (C.c_int, [C.c_void_p, C.POINTER(sp_camera_ray_params), C.c_void_p, C.POINTER(sp_feature_stats)]),
    "sp_scene_camera_rays_host": (C.c_int, [C.c_void_p, C.POINTER(sp_camera_ray_params), C.c_void_p,
                                            C.POINTER(sp_feature_stats)]),
    "sp_scene_features": (C.c_int, [C.c_void_p, C.POINTER(sp_feature_params), C.POINTER(sp_feature_stats)]),
    "sp_scene_features_host": (C.c_int, [C.c_void_p, C.POINTER(sp_feature_params), C.POINTER(sp_feature_stats)]),
    "sp_denoiser_create": (C.c_int, [C.POINTER(sp_denoiser_params), C.POINTER(C.c_void_p)]),
    "sp_denoiser_free": (None, [C.c_void_p]),
    "sp_denoiser_device_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "sp_denoiser_run": (C.c_int, [C.c_void_p, C.POINTER(sp_denoise_params), C.POINTER(sp_denoise_stats)]),
    "sp_denoiser_run_host": (C.c_int, [C.c_void_p, C.POINTER(sp_denoise_params), C.POINTER(sp_denoise_stats)]),
    "sp_render_tiles": (C.c_int, [C.c_void_p, C.POINTER(sp_render_params), C.c_void_p, C.POINTER(sp_render_stats)]),
    "sp_render_tiles_host": (C.c_int, [C.c_void_p, C.POINTER(sp_render_params), C.POINTER(C.c_float),
                                       C.POINTER(sp_render_stats)]),
    "sp_scene_bvh_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sp_scene_device_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "sp_scene_bvh_build_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(sp_bvh_info)]),
    "sp_tiles_to_image": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64,
                                    C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sp_write_pfm": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "sp_rsqrt_table_get": (C.c_int, [C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    "sp_rsqrt_table_set": (C.c_int, [C.POINTER(C.c_uint32), C.c_int32, C.c_uint32, C.c_uint32]),
    "sp_rsqrt_table_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sp_host_rsqrt_emulated": (C.c_float, [C.c_float]),
}

_lib = None


def lib():
    """Load the in-tree HIP library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C simplepath_amd` or __graft_entry__.build(); "
                "the MI355X path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def build_identity() -> dict:
    """Which library this process runs: its path, the build's content hash (sp_build_id, ABI 5)
    and the SHA-256 prefix of the .so file itself -- recorded in every bench line, so a swapped
    library (SP_LIB_PATH) is visible."""
    import hashlib
    L = lib()
    with open(LIB_PATH, "rb") as f:
        so_sha = hashlib.sha256(f.read()).hexdigest()[:16]
    return {"path": os.path.relpath(os.path.realpath(LIB_PATH), os.path.dirname(_HERE)),
            "build_id": L.sp_build_id().decode(), "so_sha256_16": so_sha,
            "default": os.path.realpath(LIB_PATH) == os.path.realpath(os.path.join(_HERE, "_build", "libsimplepath_hip.so"))}


class SimplePathError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def check(rc: int) -> None:
    if rc != SP_OK:
        raise SimplePathError(rc, lib().sp_last_error().decode(errors="replace"))

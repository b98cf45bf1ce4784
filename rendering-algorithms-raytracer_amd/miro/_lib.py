"""ctypes binding of libmrt.so (include/mrt.h).  Loads the in-tree build only;
raises if it is missing -- there is no fallback path."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MRT_LIB", os.path.join(_PKG, "lib", "libmrt.so"))

MRT_OK = 0
ABI_VERSION = 10   # include/mrt.h MRT_ABI_VERSION: the struct layouts below
ERRORS = {-1: "MRT_ERR_INVALID", -2: "MRT_ERR_IO", -3: "MRT_ERR_HIP", -4: "MRT_ERR_BUILD",
          -5: "MRT_ERR_NOT_BUILT", -6: "MRT_ERR_OVERFLOW", -7: "MRT_ERR_NO_DEVICE"}

# Every symbol include/mrt.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "mrt_last_error", "mrt_abi_version", "mrt_device_count", "mrt_scene_create", "mrt_scene_destroy",
    "mrt_scene_add_material", "mrt_scene_add_light", "mrt_scene_add_obj", "mrt_scene_add_mesh",
    "mrt_scene_mesh_info", "mrt_scene_mesh_export", "mrt_scene_set_background", "mrt_scene_set_num_paths", "mrt_scene_set_subdivs", "mrt_scene_set_material_optics", "mrt_scene_set_material_dispersion", "mrt_scene_set_material_gloss", "mrt_scene_set_material_translucency",
    "mrt_scene_build_bvh", "mrt_scene_bvh_info", "mrt_scene_bvh_export", "mrt_scene_bvh_import",
    "mrt_scene_upload", "mrt_render", "mrt_render_buckets_async", "mrt_unpack_buckets_async",
    "mrt_render_frame_async", "mrt_trace", "mrt_trace_async", "mrt_scene_last_stats", "mrt_rcp_nr",
    "mrt_rsqrt_nr", "mrt_debug_libm", "mrt_set_tuning", "mrt_render_batch_async", "mrt_unpack_batch_async",
    "mrt_debug_wave_log", "mrt_device_wall_clock_khz", "mrt_hdr_info", "mrt_hdr_load", "mrt_scene_add_texture",
    "mrt_scene_set_env_map", "mrt_scene_set_material_env_map", "mrt_scene_dome_info", "mrt_scene_dome_export", "mrt_scene_make_blas",
    "mrt_scene_add_instance", "mrt_scene_blas_info", "mrt_scene_blas_export", "mrt_scene_set_material_emission",
    "mrt_scene_set_material_sample_env", "mrt_scene_set_path_trace", "mrt_scene_prim_object",
    "mrt_image_info", "mrt_image_load", "mrt_scene_add_texture_typed", "mrt_scene_set_material_maps",
    "mrt_scene_mesh_set_texcoords", "mrt_scene_mesh_texcoords", "mrt_scene_set_mesh_motion", "mrt_scene_walk_info",
    "mrt_render_batch_frames_async", "mrt_ipc_export", "mrt_ipc_open", "mrt_ipc_close", "mrt_get_tuning",
    "mrt_walk_arrays_fit", "mrt_sample_rays", "mrt_sample_rays_async", "mrt_camera_rays",
    "mrt_trace_rays", "mrt_trace_rays_async", "mrt_shade_hits", "mrt_shade_hits_async", "mrt_hit_surfaces",
    "mrt_hit_surfaces_async", "mrt_scene_update_mesh", "mrt_scene_update_mesh_async",
    "mrt_scene_update_instances", "mrt_scene_update_instances_async", "mrt_scene_instance_count",
    "mrt_scene_instance_info", "mrt_scene_deform_mesh", "mrt_scene_deform_mesh_async",
    "mrt_debug_live_resources", "mrt_sample_lights", "mrt_sample_lights_async",
    "mrt_scene_light_sample_cap", "mrt_light_samples", "mrt_light_samples_async",
    "mrt_scene_update_lights", "mrt_scene_update_lights_async", "mrt_scene_update_material",
    "mrt_scene_update_material_async", "mrt_scene_update_texture", "mrt_scene_update_texture_async",
    "mrt_scene_texture_update_status", "mrt_scene_dome_export_derived", "mrt_scene_upload_count",
    "mrt_scene_rebuild_bvh", "mrt_scene_rebuild_bvh_async", "mrt_scene_bvh_cost", "mrt_debug_bin_rays",
]


class mrt_material(C.Structure):
    _fields_ = [("type", C.c_int32), ("kd", C.c_float * 3), ("ka", C.c_float * 3), ("ks", C.c_float * 3),
                ("spec_exp", C.c_float), ("spec_amt", C.c_float), ("le", C.c_float * 3), ("emitted", C.c_float)]


class mrt_light(C.Structure):
    _fields_ = [("type", C.c_int32), ("pos", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3),
                ("v3", C.c_float * 3), ("power", C.c_float), ("samples", C.c_int32),
                ("noise_threshold", C.c_float), ("cast_shadows", C.c_int32), ("texture", C.c_int32),
                ("transparent_shadows", C.c_int32)]


class mrt_camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("look_at", C.c_float * 3), ("up", C.c_float * 3), ("fov_deg", C.c_float),
                ("aperture", C.c_float), ("focus_plane", C.c_float), ("shutter_speed", C.c_float)]


class mrt_mesh(C.Structure):
    _fields_ = [("verts", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("vidx", C.POINTER(C.c_uint32)), ("nidx", C.POINTER(C.c_uint32)),
                ("nv", C.c_int32), ("nn", C.c_int32), ("nt", C.c_int32),
                ("vert_stride", C.c_int32), ("normal_stride", C.c_int32)]


class mrt_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("a", C.c_float), ("b", C.c_float), ("prim", C.c_int32), ("inst", C.c_int32)]


class mrt_surface(C.Structure):
    _fields_ = [("p", C.c_float * 3), ("n", C.c_float * 3), ("geo_n", C.c_float * 3), ("tan", C.c_float * 3),
                ("bitan", C.c_float * 3), ("u", C.c_float), ("v", C.c_float), ("material", C.c_int32),
                ("mesh", C.c_int32), ("tri", C.c_int32), ("inst", C.c_int32)]


class mrt_bvh_info(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("leaves", C.c_int32), ("prims", C.c_int32), ("bin_nodes", C.c_int32),
                ("bin_leaves", C.c_int32), ("max_depth", C.c_int32), ("build_ms", C.c_double),
                ("device_bytes", C.c_uint64)]


class mrt_ipc_handle(C.Structure):
    _fields_ = [("handle", C.c_uint8 * 64), ("offset", C.c_uint64), ("size", C.c_uint64)]


class mrt_render_opts(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("device", C.c_int32), ("count_visits", C.c_int32),
                ("want_rgb8", C.c_int32), ("want_hits", C.c_int32), ("seed", C.c_uint32),
                ("devices", C.POINTER(C.c_int32)), ("n_devices", C.c_int32)]


class mrt_stats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("node_visits", C.c_uint64),
                ("leaf_visits", C.c_uint64), ("primary_node_visits", C.c_uint64),
                ("primary_leaf_visits", C.c_uint64), ("primary_hits", C.c_uint64), ("primary_wave_steps", C.c_uint64),
                ("primary_uniform_visits", C.c_uint64), ("kernel_ms", C.c_float), ("primary_ms", C.c_float),
                ("shade_ms", C.c_float), ("max_stack", C.c_int32),
                ("primary_span_us", C.c_float), ("primary_ramp_us", C.c_float), ("primary_tail_us", C.c_float),
                ("shade_span_us", C.c_float), ("shade_ramp_us", C.c_float), ("shade_tail_us", C.c_float),
                ("secondary_rays", C.c_uint64), ("shadow_wave_steps", C.c_uint64), ("shadow_node_visits", C.c_uint64),
                ("fused", C.c_int32), ("chain", C.c_int32), ("chain_budget_bytes", C.c_uint64),
                ("chain_chunks", C.c_uint32), ("chain_fallbacks", C.c_int32)]


class mrt_bin_probe(C.Structure):
    _fields_ = [("o", C.c_void_p), ("d", C.c_void_p), ("n", C.c_uint32), ("has_n_dev", C.c_int32), ("n_dev", C.c_uint32),
                ("mul1", C.c_uint32), ("sub", C.c_uint32), ("cap1", C.c_uint32), ("mul2", C.c_uint32),
                ("nrays", C.c_void_p), ("m", C.c_uint32), ("lo", C.c_float * 3), ("inv", C.c_float * 3),
                ("dbits", C.c_int32), ("obits", C.c_int32), ("grid", C.c_int32), ("hits", C.c_void_p),
                ("hit_base", C.c_void_p), ("inst_class", C.c_void_p), ("n_inst", C.c_int32), ("n_world", C.c_int32),
                ("inst_cell", C.c_void_p), ("inst_inv", C.c_void_p), ("keys", C.c_void_p), ("hist", C.c_void_p),
                ("perm", C.c_void_p)]


_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)
_bp = C.POINTER(C.c_uint8)
_lib = None


class MRTError(RuntimeError):
    pass


def build_info(L=None):
    """The source hash embedded in the loaded libmrt.so (Makefile, tools/source_hash.py)
    next to the hash of the sources beside it: {"library": ..., "sources": ..., "match": ...}
    ("sources" is None where the tools are not shipped)."""
    L = L or load()
    try:
        lib_hash = (C.c_char * 17).in_dll(L, "mrt_source_hash").value.decode()
    except ValueError:
        lib_hash = None
    src_hash = None
    tools = os.path.join(os.path.dirname(_PKG), "tools")
    if os.path.exists(os.path.join(tools, "source_hash.py")):
        import importlib.util
        spec = importlib.util.spec_from_file_location("mrt_source_hash", os.path.join(tools, "source_hash.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        src_hash = mod.source_hash()
    return {"library": lib_hash, "sources": src_hash, "match": lib_hash is not None and lib_hash == src_hash}


def load():
    """Load libmrt.so (fails loudly when the HIP build is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MRTError(f"libmrt.so not built at {LIB_PATH}; run __graft_entry__.build() "
                       f"(make -C rendering-algorithms-raytracer_amd)")
    # One HIP runtime per process: if PyTorch-ROCm is importable, load it first so
    # libmrt's libamdhip64.so.7 resolves to the runtime torch already mapped
    # (torch ships its own copy; two HIP/HSA runtimes cannot share the device).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    L.mrt_last_error.restype = C.c_char_p
    # the structures below must match the library's: a stale build would read them
    # with another layout (e.g. ignore mrt_light.transparent_shadows, ABI 7)
    got = L.mrt_abi_version()
    if got != ABI_VERSION:
        raise MRTError(f"{LIB_PATH} has ABI {got}, this binding expects {ABI_VERSION}: rebuild it "
                       f"(__graft_entry__.build() or make -C rendering-algorithms-raytracer_amd)")
    L.mrt_scene_create.restype = C.c_void_p
    L.mrt_scene_destroy.argtypes = [C.c_void_p]
    L.mrt_scene_add_material.argtypes = [C.c_void_p, C.POINTER(mrt_material)]
    L.mrt_scene_add_light.argtypes = [C.c_void_p, C.POINTER(mrt_light)]
    L.mrt_scene_add_obj.argtypes = [C.c_void_p, C.c_char_p, _fp, C.c_int]
    L.mrt_scene_add_mesh.argtypes = [C.c_void_p, C.POINTER(mrt_mesh), C.c_int]
    L.mrt_scene_mesh_info.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
    L.mrt_scene_mesh_export.argtypes = [C.c_void_p, C.c_int, _fp, _fp, _up, _up]
    L.mrt_scene_set_background.argtypes = [C.c_void_p, _fp]
    L.mrt_scene_set_num_paths.argtypes = [C.c_void_p, C.c_int]
    L.mrt_scene_set_subdivs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.mrt_scene_set_material_optics.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    L.mrt_scene_set_material_gloss.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.mrt_scene_set_material_dispersion.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp]
    L.mrt_scene_set_material_translucency.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.mrt_scene_set_material_emission.argtypes = [C.c_void_p, C.c_int, C.c_float, _fp]
    L.mrt_scene_set_material_sample_env.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mrt_scene_set_path_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.mrt_scene_prim_object.argtypes = [C.c_void_p, C.c_int32, _ip, _ip, _ip]
    L.mrt_scene_build_bvh.argtypes = [C.c_void_p]
    L.mrt_scene_bvh_info.argtypes = [C.c_void_p, C.POINTER(mrt_bvh_info)]
    L.mrt_scene_bvh_export.argtypes = [C.c_void_p, _fp, _ip, _fp, _ip]
    L.mrt_scene_bvh_import.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _fp, _ip, _fp, _ip]
    L.mrt_scene_upload.argtypes = [C.c_void_p, C.c_int]
    L.mrt_render.argtypes = [C.c_void_p, C.POINTER(mrt_camera), C.POINTER(mrt_render_opts), _fp, _bp, C.c_void_p]
    L.mrt_render_buckets_async.argtypes = [C.c_void_p, C.POINTER(mrt_camera), C.POINTER(mrt_render_opts),
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.mrt_unpack_buckets_async.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    L.mrt_render_batch_async.argtypes = [C.c_void_p, C.POINTER(mrt_camera), C.c_int32, C.POINTER(mrt_render_opts),
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mrt_unpack_batch_async.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mrt_render_batch_frames_async.argtypes = [C.c_void_p, C.POINTER(mrt_camera), C.c_int32,
                                                C.POINTER(mrt_render_opts), C.c_void_p, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
    L.mrt_ipc_export.argtypes = [C.c_void_p, C.POINTER(mrt_ipc_handle)]
    L.mrt_ipc_open.argtypes = [C.POINTER(mrt_ipc_handle), C.c_int, C.POINTER(C.c_void_p)]
    L.mrt_ipc_close.argtypes = [C.c_void_p]
    L.mrt_render_frame_async.argtypes = [C.c_void_p, C.POINTER(mrt_camera), C.POINTER(mrt_render_opts),
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.mrt_trace.argtypes = [C.c_void_p, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, C.c_void_p]
    L.mrt_trace_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(L, "mrt_sample_rays"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_sample_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                      C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
        L.mrt_sample_rays_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                            C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mrt_camera_rays.argtypes = [C.POINTER(mrt_camera), C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    if hasattr(L, "mrt_shade_hits"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        vp = C.c_void_p
        L.mrt_trace_rays.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp]
        L.mrt_trace_rays_async.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp, vp]
        L.mrt_shade_hits.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_int32, C.c_uint32, C.c_int32, vp]
        L.mrt_shade_hits_async.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_int32, C.c_uint32, C.c_int32, vp, vp]
        L.mrt_hit_surfaces.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
        L.mrt_hit_surfaces_async.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
    if hasattr(L, "mrt_sample_lights"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        vp = C.c_void_p
        L.mrt_sample_lights.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, vp]
        L.mrt_sample_lights_async.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                              vp, vp, vp]
    if hasattr(L, "mrt_light_samples"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        vp = C.c_void_p
        L.mrt_scene_light_sample_cap.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_int32)]
        L.mrt_light_samples.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                        vp, vp, vp, vp]
        L.mrt_light_samples_async.argtypes = L.mrt_light_samples.argtypes + [vp]
    if hasattr(L, "mrt_scene_update_mesh"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_scene_update_mesh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.mrt_scene_update_mesh_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "mrt_scene_update_instances"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_scene_update_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_float)]
        L.mrt_scene_update_instances_async.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.mrt_scene_instance_count.argtypes = [C.c_void_p]
        L.mrt_scene_instance_info.argtypes = [C.c_void_p, C.c_int32, _ip, _fp, _fp, _fp, _fp]
    if hasattr(L, "mrt_scene_deform_mesh"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_scene_deform_mesh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.mrt_scene_deform_mesh_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "mrt_scene_update_lights"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        vp = C.c_void_p
        L.mrt_scene_update_lights.argtypes = [vp, vp, C.c_int32]
        L.mrt_scene_update_lights_async.argtypes = [vp, vp, C.c_int32, vp]
        L.mrt_scene_update_material.argtypes = [vp, C.c_int, vp]
        L.mrt_scene_update_material_async.argtypes = [vp, C.c_int, vp, vp]
        L.mrt_scene_update_texture.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_float)]
        L.mrt_scene_update_texture_async.argtypes = [vp, C.c_int32, vp, vp]
        L.mrt_scene_texture_update_status.argtypes = [vp, _ip]
        L.mrt_scene_dome_export_derived.argtypes = [vp, C.c_int32, _fp, _ip, _ip]
        L.mrt_scene_upload_count.argtypes = [vp]
    if hasattr(L, "mrt_scene_rebuild_bvh"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_scene_rebuild_bvh.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.mrt_scene_rebuild_bvh_async.argtypes = [C.c_void_p, C.c_void_p]
        L.mrt_scene_bvh_cost.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mrt_scene_last_stats.argtypes = [C.c_void_p, C.POINTER(mrt_stats)]
    L.mrt_set_tuning.argtypes = [C.c_char_p, C.c_int]
    if hasattr(L, "mrt_get_tuning"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_get_tuning.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    if hasattr(L, "mrt_walk_arrays_fit"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_walk_arrays_fit.argtypes = [C.c_uint64, C.c_uint64]
    L.mrt_debug_wave_log.argtypes =[C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
    L.mrt_device_wall_clock_khz.argtypes = [C.c_void_p]
    L.mrt_hdr_info.argtypes = [C.c_char_p, _ip, _ip]
    L.mrt_hdr_load.argtypes = [C.c_char_p, _fp, C.c_int32, C.c_int32]
    L.mrt_scene_add_texture.argtypes = [C.c_void_p, _fp, C.c_int32, C.c_int32]
    L.mrt_image_info.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.mrt_image_load.argtypes = [C.c_char_p, _fp, C.c_int32, C.c_int32]
    L.mrt_scene_add_texture_typed.argtypes = [C.c_void_p, _fp, C.c_int32, C.c_int32, C.c_int32]
    L.mrt_scene_set_material_maps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.mrt_scene_mesh_set_texcoords.argtypes = [C.c_void_p, C.c_int, _fp, C.c_int32, C.POINTER(C.c_uint32)]
    L.mrt_scene_set_mesh_motion.argtypes = [C.c_void_p, C.c_int, _fp]
    L.mrt_scene_mesh_texcoords.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_uint32)]
    L.mrt_scene_set_env_map.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    L.mrt_scene_set_material_env_map.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_float]
    L.mrt_scene_dome_info.argtypes = [C.c_void_p, C.c_int32, _ip, _ip]
    L.mrt_scene_dome_export.argtypes = [C.c_void_p, C.c_int32] + [_fp] * 9
    L.mrt_scene_make_blas.argtypes = [C.c_void_p, _ip, C.c_int32]
    L.mrt_scene_add_instance.argtypes = [C.c_void_p, C.c_int32, _fp]
    L.mrt_scene_blas_info.argtypes = [C.c_void_p, C.c_int32, _ip, _ip, _ip]
    L.mrt_scene_blas_export.argtypes = [C.c_void_p, C.c_int32, _fp, _ip, _fp, _ip]
    if hasattr(L, "mrt_scene_walk_info"):
        L.mrt_scene_walk_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(L, "mrt_debug_libm"):   # (absent from round-4 builds loaded for A/B runs via MRT_LIB)
        L.mrt_debug_libm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    if hasattr(L, "mrt_debug_bin_rays"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_debug_bin_rays.argtypes = [C.POINTER(mrt_bin_probe)]
    if hasattr(L, "mrt_debug_live_resources"):   # (absent from earlier builds loaded for A/B runs via MRT_LIB)
        L.mrt_debug_live_resources.argtypes = []
        L.mrt_debug_live_resources.restype = C.c_int64
    L.mrt_rcp_nr.argtypes = [C.c_float]
    L.mrt_rcp_nr.restype = C.c_float
    L.mrt_rsqrt_nr.argtypes = [C.c_float]
    L.mrt_rsqrt_nr.restype = C.c_float
    _lib = L
    return L


def check(rc, what=""):
    """Raise MRTError for a negative status, return rc otherwise."""
    if rc < 0:
        msg = load().mrt_last_error().decode(errors="replace")
        raise MRTError(f"{what}: {ERRORS.get(rc, rc)}: {msg}")
    return rc


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])

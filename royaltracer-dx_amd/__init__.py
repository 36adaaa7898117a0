"""royaltracer-dx_amd — ctypes binding of the MI355X wavefront path tracer (librtx_hip.so).

The product path is the HIP library only.  Importing this package raises ImportError if
librtx_hip.so has not been built, and Context() raises RtxError if no GPU can be opened:
there is no CPU fallback and nothing under oracle/ is ever imported from here.

The C-ABI is declared in include/rtx.h (hot path) and include/rtx_host.h (scene-loader /
material / camera layer mirroring the reference's ObjLoader / Manipulator / Renderer).
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTX_LIB_PATH") or os.path.join(_HERE, "librtx_hip.so")   # RTX_LIB_PATH: tooling builds (make PROFILE=1)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (hipcc --offload-arch=gfx950) "
        "or `python -c 'import __graft_entry__ as g; g.build()'`.  There is no CPU fallback.")

# PyTorch wheels bundle their own libamdhip64.so.7.  A process must hold ONE HIP runtime, otherwise the second
# one to initialise sees no devices and stream / device-pointer interop (rtx_set_stream, rtx_bind_accum) is
# meaningless.  Import torch first (when present) so that librtx_hip.so binds to the runtime torch uses.
if os.environ.get("RTX_NO_TORCH_PRELOAD", "0") != "1":
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional: the library only needs the HIP runtime
        pass

lib = C.CDLL(LIB_PATH)

RTX_OK = 0
FLAG_LAMBERT_ONLY = 1
FLAG_JITTER = 2
FLAG_TRANSMISSION = 4
FLAG_BLOCK_TILES = 8
K_RAYGEN, K_TRACE, K_SHADE, K_SHADOW, K_ACCUM, K_SORT, K_BOUNCE, K_ADAPT, K_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8
KERNEL_NAMES = {K_RAYGEN: "raygen", K_TRACE: "trace_closest", K_SHADE: "shade", K_SHADOW: "trace_shadow", K_ACCUM: "accumulate", K_SORT: "sort", K_BOUNCE: "bounce_fused", K_ADAPT: "adaptive"}
OPT_KERNEL_TIMING, OPT_PATHS_PER_BATCH, OPT_SORT_MATERIALS, OPT_LDS_NODES, OPT_SMALL_SCENE, OPT_FUSED_BOUNCE, OPT_BOUNCE_VARIANT = 1, 2, 3, 4, 5, 6, 7
OPT_REFILL_MIN, OPT_STACK_PRIVATE, OPT_TRACE_SCHED, OPT_GPU_REFIT, OPT_BLOCKS_PER_CU, OPT_LPT_ORDER, OPT_FUSED_BVH, OPT_WORK_STEALING, OPT_COMPACT_STATE, OPT_OVERLAP_SHADOW = 8, 9, 10, 11, 12, 13, 14, 15, 16, 18
OPT_RESTIR_WAVEFRONT, OPT_RESTIR_CHUNKS, OPT_OCCLUDER_CACHE, OPT_RESTIR_LANES, OPT_SHADE_DENSE, OPT_MERGE_RAYS, OPT_TAPER = 19, 20, 21, 22, 23, 24, 25
OPT_BVH_REINSERT, OPT_BVH_SPLIT, OPT_ANYHIT_ORDER, OPT_RESTIR_LANE_MIN, OPT_TRACE_COUNTERS, OPT_ASYNC, OPT_OCTANT_SORT, OPT_SAMPLE_INTERLEAVE, OPT_NODE_STRIDE, OPT_RESTIR_KEYS, OPT_LDS_NODES_CLOSEST, OPT_PARTIAL_REFIT = 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37
OPT_GPU_BUILD = 38
OPT_STACK_CAP = 39
OPT_DEFORM_REBUILD = 40
OPT_SHARED_PRIMARY = 41
OPT_DENOISE_LDS_STEP = 42
OPT_SMALL_SLABS = 43
TEX_SRGB = 1          # rtx_set_texture flag: the bytes are sRGB-encoded
MAP_KD = 0            # rtx_set_material_map slot
MAP_OPACITY = 2       # ... the alpha cut-out slot: reads the texture's alpha byte (1 is not a slot)
MAP_NORMAL = 4        # ... the tangent-space normal map slot: reads the texture's RGB bytes through Nt (3 is not a slot)
MAP_KS = 6            # ... the specular colour slot: reads the RGB bytes, sRGB honoured (5, 7 and 9 are not slots)
MAP_PR = 8            # ... the roughness slot: reads the green byte through the linear table
MAP_PM = 10           # ... the metalness slot: reads the blue byte through the linear table
MAP_KE = 12           # the emission slot (include/rtx.h, EMISSION MAPS; 11 is not a slot): multiplies an emitter's Ke; RGB bytes, sRGB honoured
ENV_HIDDEN = 1        # rtx_set_environment flag: primary rays that miss stay black


class RtxError(RuntimeError):
    pass


class Params(C.Structure):
    """rtx_params (include/rtx.h)."""
    _fields_ = [(n, C.c_uint32) for n in (
        "width", "height", "spp", "sample_base", "max_bounces", "nee_samples", "rr_start",
        "frame_seed", "flags", "tile_size", "shard_rank", "shard_count")]

    def __init__(self, width=1920, height=1080, spp=1, sample_base=1, max_bounces=8, nee_samples=1,
                 rr_start=3, frame_seed=1, flags=0, tile_size=64, shard_rank=0, shard_count=1):
        super().__init__(width, height, spp, sample_base, max_bounces, nee_samples, rr_start,
                         frame_seed, flags, tile_size, shard_rank, shard_count)

    def copy(self, **kw):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d.update(kw)
        return Params(**d)


class Stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_extension", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("paths", C.c_uint64), ("kernel_ms", C.c_double * K_COUNT), ("kernel_launches", C.c_uint64 * K_COUNT),
                ("kernel_items", C.c_uint64 * K_COUNT), ("render_ms", C.c_double),
                ("bvh_nodes", C.c_uint32), ("triangles", C.c_uint32), ("lights", C.c_uint32), ("materials", C.c_uint32),
                ("primary_hits", C.c_uint64), ("bvh_refits", C.c_uint32), ("bvh_refs", C.c_uint32), ("restir_stale_history_reads", C.c_uint64)]

    @property
    def rays(self):
        return self.rays_primary + self.rays_extension + self.rays_shadow


_vp, _u32, _fp = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)


def _sig(name, restype, *argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


# ---- include/rtx.h ----
_sig("rtx_create", C.c_int, C.c_int, C.POINTER(_vp))
_sig("rtx_destroy", None, _vp)
_sig("rtx_last_error", C.c_char_p, _vp)
_sig("rtx_set_option", C.c_int, _vp, C.c_int, C.c_int64)
_sig("rtx_set_stream", C.c_int, _vp, _vp)
_sig("rtx_set_materials", C.c_int, _vp, _vp, _u32)
_sig("rtx_add_mesh", C.c_int, _vp, _vp, _u32, _vp, _u32, _vp, _u32p)
_sig("rtx_add_instance", C.c_int, _vp, _u32, _fp, _u32p)
_sig("rtx_set_instance_transform", C.c_int, _vp, _u32, _fp)
_sig("rtx_set_instance_visible", C.c_int, _vp, _u32, C.c_int)
_sig("rtx_update_mesh_vertices", C.c_int, _vp, _u32, _vp, _u32)
_sig("rtx_commit_scene", C.c_int, _vp)
_sig("rtx_set_mesh_uvs", C.c_int, _vp, _u32, _vp, _u32)
_sig("rtx_set_texture", C.c_int, _vp, _u32, _vp, _u32, _u32, _u32)
_sig("rtx_set_material_map", C.c_int, _vp, _u32, _u32, C.c_int32)
_sig("rtx_debug_texture_sample", C.c_int, _vp, _u32, _vp, _u32, _vp)
_sig("rtx_debug_albedo", C.c_int, _vp, _vp, _vp, _u32, _vp)
_sig("rtx_debug_opacity", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_shading_normal", C.c_int, _vp, _vp, _vp, _u32, _vp)
_sig("rtx_set_ess_table", C.c_int, _vp, _vp, _u32)
_sig("rtx_debug_specular", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_emission", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_light_sample", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_ess", C.c_int, _vp, _u32, _vp, _vp, _u32, _vp)
_sig("rtx_debug_tri_tangents", C.c_int, _vp, _u32, _u32, _vp)
_sig("rtx_set_environment", C.c_int, _vp, _vp, _u32, _vp, C.c_float, _u32)
_sig("rtx_debug_env_sample", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_env_eval", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_env_tables", C.c_int, _vp, _vp, _vp, _vp)
_sig("rtx_set_camera", C.c_int, _vp, _fp, _fp)
class Lens(C.Structure):
    """rtx_lens (include/rtx.h): the thin-lens camera"""
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float), ("reserved", C.c_uint32 * 2)]


_sig("rtx_set_lens", C.c_int, _vp, C.POINTER(Lens))
_sig("rtx_focus_distance_at", C.c_int, _vp, _u32, _u32, _u32, _u32, _fp)
_sig("rtx_save_scene_cache", C.c_int, _vp, C.c_char_p)
_sig("rtx_load_scene_cache", C.c_int, _vp, C.c_char_p)
_sig("rtx_bind_accum", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtx_clear_accum", C.c_int, _vp, _u32, _u32)
_sig("rtx_render", C.c_int, _vp, C.POINTER(Params))
_sig("rtx_read_accum", C.c_int, _vp, _vp, C.c_size_t)
class Adaptive(C.Structure):
    """rtx_adaptive (include/rtx.h)"""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float), ("dark_floor", C.c_float), ("reserved", C.c_uint32 * 3)]


class AdaptiveResult(C.Structure):
    """rtx_adaptive_result (include/rtx.h)"""
    _fields_ = [("passes", C.c_uint32), ("chunks", C.c_uint32), ("chunks_converged", C.c_uint32), ("chunks_at_max", C.c_uint32), ("pixel_samples", C.c_uint64)]


_sig("rtx_render_adaptive", C.c_int, _vp, C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(AdaptiveResult))
class DenoiseParams(C.Structure):
    """rtx_denoise_params (include/rtx.h); 0 = the default of a field"""
    _fields_ = [("levels", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_color", C.c_float), ("sigma_plane", C.c_float), ("reserved", C.c_uint32 * 4)]


class DenoiseResult(C.Structure):
    """rtx_denoise_result (include/rtx.h)"""
    _fields_ = [("levels", C.c_uint32), ("pixels_filtered", C.c_uint32), ("pixels_passed", C.c_uint32), ("guides_ms", C.c_double), ("filter_ms", C.c_double)]


_sig("rtx_denoise", C.c_int, _vp, _u32, _u32, C.POINTER(DenoiseParams), C.POINTER(DenoiseResult))
_sig("rtx_read_denoised", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtx_read_denoised_srgb8", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtx_debug_denoise_guides", C.c_int, _vp, _u32, _u32, _vp)
_sig("rtx_debug_denoise_map_guides", C.c_int, _vp, _u32, _u32, _vp)
DENOISE_ALBEDO, DENOISE_MAPPED_NORMALS = 1, 2      # rtx_denoise_params.flags, the first of DenoiseParams.reserved's four words
class DenoiseVarParams(C.Structure):
    """rtx_denoise_var_params (include/rtx.h); 0 = the default of a field"""
    _fields_ = [("levels", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_var", C.c_float), ("sigma_plane", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


_sig("rtx_denoise_variance", C.c_int, _vp, _u32, _u32, C.POINTER(DenoiseVarParams), C.POINTER(DenoiseResult))
_sig("rtx_read_adaptive_half", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtx_debug_denoise_variance", C.c_int, _vp, _u32, _u32, _u32, _vp)
_sig("rtx_render_v6_pass1", C.c_int, _vp, C.POINTER(Params))
_sig("rtx_render_restir", C.c_int, _vp, C.POINTER(Params))
_sig("rtx_restir_reset", C.c_int, _vp)
_sig("rtx_restir_state_slab_bytes", C.c_int, C.POINTER(Params), C.POINTER(C.c_size_t))
_sig("rtx_restir_pack_state", C.c_int, _vp, C.POINTER(Params), _vp)
_sig("rtx_restir_unpack_state", C.c_int, _vp, C.POINTER(Params), _vp)
class HaloPeer(C.Structure):
    """rtx_halo_peer (include/rtx.h): one neighbour of a rank in the halo exchange of the ReSTIR history"""
    _fields_ = [(n, C.c_uint32) for n in ("rank", "send_x0", "send_y0", "send_x1", "send_y1", "recv_x0", "recv_y0", "recv_x1", "recv_y1")] + \
               [(n, C.c_uint64) for n in ("send_offset", "send_bytes", "recv_offset", "recv_bytes")]


_sig("rtx_restir_halo_plan", C.c_int, C.POINTER(Params), _u32, C.POINTER(HaloPeer), _u32, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_sig("rtx_restir_pack_halo", C.c_int, _vp, C.POINTER(Params), _u32, _vp)
_sig("rtx_restir_unpack_halo", C.c_int, _vp, C.POINTER(Params), _u32, _vp)
_sig("rtx_debug_tree_hash", C.c_int, _vp, C.POINTER(C.c_uint64))
_sig("rtx_debug_tree_cost", C.c_int, _vp, C.POINTER(C.c_double))
_sig("rtx_debug_read_host_build", C.c_int, _vp, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))
_sig("rtx_debug_host_checksums", C.c_int, _vp, C.POINTER(C.c_uint64))
_sig("rtx_debug_read_tree", C.c_int, _vp, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)
_sig("rtx_debug_build_info", C.c_int, _vp, C.POINTER(C.c_double), _u32p)
_sig("rtx_read_restir_last", C.c_int, _vp, _vp, _vp, _vp, C.c_size_t)
_sig("rtx_pass1_slots", C.c_size_t, _u32, _u32)
_sig("rtx_read_pass1_buffers", C.c_int, _vp, _vp, _vp, _vp, C.c_size_t)
_sig("rtx_read_srgb8", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtx_get_stats", C.c_int, _vp, C.POINTER(Stats))
_sig("rtx_read_layer", C.c_int, _vp, _u32, _u32, _u32, _vp, C.c_size_t)
_sig("rtx_get_lights", C.c_int, _vp, _vp, _u32, _u32p)
_sig("rtx_shard_slab_bytes", C.c_int, C.POINTER(Params), C.POINTER(C.c_size_t))
_sig("rtx_pack_tiles", C.c_int, _vp, C.POINTER(Params), _vp)
_sig("rtx_unpack_tiles", C.c_int, _vp, C.POINTER(Params), _vp)
_sig("rtx_debug_primary_rays", C.c_int, _vp, C.POINTER(Params), _u32, _vp)
_sig("rtx_debug_primary_seeds", C.c_int, _vp, C.POINTER(Params), _u32, _vp)
_sig("rtx_debug_trace_closest", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_trace_any", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_trace_stats", C.c_int, _vp, _vp, _u32, _vp)
_sig("rtx_debug_validate_bvh", C.c_int, _vp)
_sig("rtx_debug_trace_counters", C.c_int, _vp, C.POINTER(C.c_uint64))
_sig("rtx_debug_surface", C.c_int, _vp, _vp, _vp, _u32, _vp)
_sig("rtx_debug_bsdf_eval", C.c_int, _vp, _u32, _u32, _vp, _u32, _vp)
_sig("rtx_debug_bsdf_sample", C.c_int, _vp, _u32, _u32, _vp, _u32, _vp)
_sig("rtx_debug_tea", C.c_int, _vp, _u32p, _u32, _vp)
# ---- include/rtx_host.h ----
_sig("rtxh_scene_cornell", _vp)
_sig("rtxh_scene_sponza_class", _vp, _u32, _u32)
_sig("rtxh_scene_bistro_class", _vp, _u32, _u32)
_sig("rtxh_scene_sponza_class_hard", _vp, _u32, _u32)
_sig("rtxh_scene_bistro_class_hard", _vp, _u32, _u32)
_sig("rtxh_scene_from_obj", _vp, C.POINTER(C.c_char_p), _u32, C.c_char_p)
_sig("rtxh_scene_from_obj_ex", _vp, C.POINTER(C.c_char_p), _u32, C.c_char_p, _u32)
_sig("rtxh_scene_opacity_map", C.c_int, _vp, _u32)
_sig("rtxh_scene_from_obj_ex2", _vp, C.POINTER(C.c_char_p), _u32, C.c_char_p, _u32, C.c_float)
_sig("rtxh_scene_normal_map", C.c_int, _vp, _u32)
_sig("rtxh_scene_spec_map", C.c_int, _vp, _u32, _u32)
_sig("rtxh_scene_emission_map", C.c_int, _vp, _u32)
_sig("rtxh_scene_free", None, _vp)
_sig("rtxh_scene_save", C.c_int, _vp, C.c_char_p)
_sig("rtxh_scene_load", _vp, C.c_char_p)
_sig("rtxh_last_error", C.c_char_p)
_sig("rtxh_scene_num_materials", _u32, _vp)
_sig("rtxh_scene_materials", _vp, _vp)
class MaterialExt(C.Structure):
    """rtxh_material_ext (include/rtx_host.h)"""
    _fields_ = [("Ni", C.c_float), ("Ns", C.c_float), ("Pcr", C.c_float), ("aniso", C.c_float), ("anisor", C.c_float), ("illum", C.c_int32),
                ("Ka", C.c_float * 3), ("Tf", C.c_float * 3), ("map", C.c_int32 * 13)]


MAP_SLOTS = ("Ka", "Kd", "Ks", "Ke", "Ns", "bump", "d", "disp", "refl", "Pr", "Pm", "Ps", "norm")
_sig("rtxh_scene_material_ext", C.c_int, _vp, _u32, C.POINTER(MaterialExt))
_sig("rtxh_scene_num_textures", _u32, _vp)
_sig("rtxh_scene_texture", C.c_char_p, _vp, _u32)
_sig("rtxh_scene_texture_pixels", C.c_int, _vp, _u32, C.POINTER(_vp), _u32p, _u32p)
_sig("rtxh_scene_mesh_uvs", C.c_int, _vp, _u32, C.POINTER(_vp), _u32p)
_sig("rtxh_read_image", C.c_int, C.c_char_p, _vp, C.c_uint64, _u32p, _u32p)
_sig("rtxh_read_hdr_image", C.c_int, C.c_char_p, _vp, C.c_uint64, _u32p, _u32p)
_sig("rtxh_env_from_latlong", C.c_int, _vp, _u32, _u32, _u32, _vp)
_sig("rtxh_scene_num_meshes", _u32, _vp)
_sig("rtxh_scene_mesh", C.c_int, _vp, _u32, C.POINTER(_vp), _u32p, C.POINTER(_vp), _u32p, C.POINTER(_vp))
_sig("rtxh_scene_num_instances", _u32, _vp)
_sig("rtxh_scene_instance", C.c_int, _vp, _u32, _u32p, _fp)
_sig("rtxh_scene_num_triangles", C.c_uint64, _vp)
_sig("rtxh_scene_camera", C.c_int, _vp, _fp, _fp, _fp, _fp, _fp, _fp)
_sig("rtxh_scene_view_proj", C.c_int, _vp, C.c_float, _fp, _fp)
_sig("rtxh_scene_upload", C.c_int, _vp, _vp, C.c_float)
_sig("rtxh_lookat", None, _fp, _fp, _fp, _fp)
_sig("rtxh_perspective_fov_rh", None, C.c_float, C.c_float, C.c_float, C.c_float, _fp)
_sig("rtxh_generate_ess_lut", None, C.c_float, _fp)
_sig("rtxh_mat4_inverse", None, _fp, _fp)
_sig("rtxh_half_round", C.c_float, C.c_float)
_sig("rtxh_bvh_check", C.c_int, _vp, _u32, _u32p, _u32p, _u32p)
_sig("rtxh_bvh_refit_check", C.c_int, _vp, _vp, _u32)
_sig("rtxh_bvh8_check", C.c_int, _vp, _u32, _u32p, _u32p)
_sig("rtxh_bvh8_stats", C.c_int, _vp, _u32, _vp, _u32p)
_sig("rtxh_bvh_option", C.c_int, C.c_char_p, C.c_double)
_sig("rtxh_bvh_replay", C.c_int, _vp, _u32, _vp, _u32, C.c_int, _u32, _vp, _u32p)
_sig("rtxh_scene_small_occluders", C.c_int, _vp, _u32p)
_sig("rtxh_scene_anyhit_order", C.c_int, _vp, _u32p)
_sig("rtxh_write_png", C.c_int, C.c_char_p, _vp, _u32, _u32)
_sig("rtxh_write_ppm", C.c_int, C.c_char_p, _vp, _u32, _u32)
_sig("rtxh_write_exr", C.c_int, C.c_char_p, _vp, _u32, _u32)
_sig("rtxh_scene_small_records", C.c_int, _vp, _vp, _vp, _u32, _u32p, _fp, _fp)
_sig("rtxh_scene_small_slabs", C.c_int, _vp, _vp, _vp, _u32, _u32p, _u32p)
_sig("rtxh_scene_set_camera", C.c_int, _vp, _fp, _fp, _fp)
_sig("rtxh_scene_set_mesh_vertices", C.c_int, _vp, _u32, _vp, _u32)
_sig("rtxh_renderer_set_mesh_vertices", C.c_int, _vp, _u32, _vp, _u32)
_sig("rtxh_renderer_create", _vp, _u32, _u32, C.c_char_p, C.c_int)
_sig("rtxh_renderer_set_scene", C.c_int, _vp, _vp)
_sig("rtxh_renderer_params", C.POINTER(Params), _vp)
_sig("rtxh_renderer_restir_params", C.POINTER(Params), _vp)
_sig("rtxh_renderer_set_mode", C.c_int, _vp, C.c_int)
_sig("rtxh_renderer_context", _vp, _vp)
_sig("rtxh_renderer_on_init", C.c_int, _vp)
_sig("rtxh_renderer_on_update", C.c_int, _vp)
_sig("rtxh_renderer_set_instance_transform", C.c_int, _vp, _u32, _vp)
_sig("rtxh_renderer_set_instance_visible", C.c_int, _vp, _u32, C.c_int)
_sig("rtxh_renderer_on_render", C.c_int, _vp)
_sig("rtxh_renderer_read_accum", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtxh_renderer_read_output", C.c_int, _vp, _vp, C.c_size_t)
_sig("rtxh_renderer_denoise_variance", C.c_int, _vp, C.POINTER(DenoiseVarParams), C.POINTER(DenoiseResult))
_sig("rtxh_renderer_on_key_up", C.c_int, _vp, C.c_uint8)
_sig("rtxh_renderer_display_layer", _u32, _vp)
_sig("rtxh_renderer_destroy", None, _vp)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(_vp)


def _fptr(a):
    return a.ctypes.data_as(_fp)


# ------------------------------------------------------------------------------------------------
# host layer
# ------------------------------------------------------------------------------------------------
def _host_maps(fn, *slot):
    """accessor of _SCENE_MAP_SLOTS over one of the host layer's rtxh_scene_*_map functions"""
    return lambda scene, n: [int(fn(scene._h, i, *slot)) for i in range(n)]


# the map slots of a scene: (Scene attribute, rtx_set_material_map slot, accessor(scene, material count) -> per material the index into `textures` or -1).  Scene.__init__ fills
# the attributes from it and Context.bind_maps binds them by it (a duck-typed scene only needs the attributes it has)
_SCENE_MAP_SLOTS = (
    ("material_maps", MAP_KD, lambda scene, n: [scene.textures.index(e["maps"]["Kd"]) if "Kd" in e["maps"] else -1 for e in scene.material_ext]),
    ("opacity_maps", MAP_OPACITY, _host_maps(lib.rtxh_scene_opacity_map)),
    ("normal_maps", MAP_NORMAL, _host_maps(lib.rtxh_scene_normal_map)),
    ("ks_maps", MAP_KS, _host_maps(lib.rtxh_scene_spec_map, MAP_KS)),
    ("pr_maps", MAP_PR, _host_maps(lib.rtxh_scene_spec_map, MAP_PR)),
    ("pm_maps", MAP_PM, _host_maps(lib.rtxh_scene_spec_map, MAP_PM)),
    ("ke_maps", MAP_KE, _host_maps(lib.rtxh_scene_emission_map)),
)


class Scene:
    """A host-side scene in the reference's data model (global Material table, per-model
    Vertex / index / materialID arrays, instance list).  Arrays are numpy copies."""

    def __init__(self, handle):
        if not handle:
            raise RtxError("scene creation failed: " + lib.rtxh_last_error().decode())
        self._h = handle
        n = lib.rtxh_scene_num_materials(handle)
        buf = (C.c_float * (n * 32)).from_address(lib.rtxh_scene_materials(handle)) if n else []
        self.materials = np.array(buf, dtype=np.float32).reshape(n, 32)
        self.textures = [lib.rtxh_scene_texture(handle, i).decode() for i in range(lib.rtxh_scene_num_textures(handle))]
        self.material_ext = []                       # per material (OBJ / MTL scenes only): the MTL fields and map ids beside the 128-byte record
        for i in range(n):
            x = MaterialExt()
            if lib.rtxh_scene_material_ext(handle, i, C.byref(x)) != RTX_OK:
                break
            self.material_ext.append(dict(Ni=x.Ni, Ns=x.Ns, Pcr=x.Pcr, aniso=x.aniso, anisor=x.anisor, illum=x.illum, Ka=list(x.Ka), Tf=list(x.Tf),
                                          maps={MAP_SLOTS[k]: self.textures[x.map[k]] for k in range(13) if x.map[k] >= 0}))
        # what the host loaded for the diffuse maps (Context.upload binds it): per texture the decoded (H, W, 4) uint8 image or None; per material the texture id of its map_Kd or -1
        self.texture_pixels = []
        for i in range(len(self.textures)):
            px, tw, th = _vp(), _u32(), _u32()
            lib.rtxh_scene_texture_pixels(handle, i, C.byref(px), C.byref(tw), C.byref(th))
            self.texture_pixels.append(np.array((C.c_uint8 * (tw.value * th.value * 4)).from_address(px.value), dtype=np.uint8).reshape(th.value, tw.value, 4) if px.value else None)
        # ... and per slot of _SCENE_MAP_SLOTS, per material, the texture id the host bound or -1: material_maps (map_Kd), opacity_maps (map_d; alpha byte = the file's alpha
        # channel for a 32-bit TGA, else its first channel), normal_maps (norm; on request map_Bump / bump, as it is or converted from a height map), ks_maps / pr_maps /
        # pm_maps (map_Ks / map_Pr / map_Pm), ke_maps (map_Ke); ess_table: the 17-row energy table that goes with a roughness map, else None
        for attr, _, accessor in _SCENE_MAP_SLOTS:
            setattr(self, attr, accessor(self, n))
        self.ess_table = ess_table_rows(17) if any(t >= 0 for t in self.pr_maps) else None
        self.meshes, self.uvs = [], []
        for i in range(lib.rtxh_scene_num_meshes(handle)):
            v, idx, mid = _vp(), _vp(), _vp()
            nv, ni = _u32(), _u32()
            lib.rtxh_scene_mesh(handle, i, C.byref(v), C.byref(nv), C.byref(idx), C.byref(ni), C.byref(mid))
            verts = np.array((C.c_float * (nv.value * 7)).from_address(v.value), dtype=np.float32).reshape(-1, 7) if nv.value else np.zeros((0, 7), np.float32)
            indices = np.array((C.c_uint32 * ni.value).from_address(idx.value), dtype=np.uint32) if ni.value else np.zeros(0, np.uint32)
            matids = np.array((C.c_uint32 * ni.value).from_address(mid.value), dtype=np.uint32) if ni.value else np.zeros(0, np.uint32)
            self.meshes.append((verts, indices, matids))
            uv, nuv = _vp(), _u32()
            lib.rtxh_scene_mesh_uvs(handle, i, C.byref(uv), C.byref(nuv))
            self.uvs.append(np.array((C.c_float * (nuv.value * 2)).from_address(uv.value), dtype=np.float32).reshape(-1, 2) if uv.value else None)      # per corner (index entry), or None
        self.instances = []
        for i in range(lib.rtxh_scene_num_instances(handle)):
            mesh = _u32()
            m = np.zeros(16, np.float32)
            lib.rtxh_scene_instance(handle, i, C.byref(mesh), _fptr(m))
            self.instances.append((mesh.value, m))
        self.num_triangles = lib.rtxh_scene_num_triangles(handle)
        e, c, u = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        fov, zn, zf = C.c_float(), C.c_float(), C.c_float()
        lib.rtxh_scene_camera(handle, _fptr(e), _fptr(c), _fptr(u), C.byref(fov), C.byref(zn), C.byref(zf))
        self.eye, self.center, self.up, self.fovy_deg, self.znear, self.zfar = e, c, u, fov.value, zn.value, zf.value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:                      # module globals are gone at interpreter shutdown
            lib.rtxh_scene_free(h)

    @classmethod
    def cornell(cls):
        return cls(lib.rtxh_scene_cornell())

    @classmethod
    def sponza_class(cls, target_tris=262144, seed=260, hard=False):
        """the Sponza-class atrium; hard=True: the size distribution of the real asset (host/Scenes.h)"""
        return cls((lib.rtxh_scene_sponza_class_hard if hard else lib.rtxh_scene_sponza_class)(target_tris, seed))

    @classmethod
    def bistro_class(cls, target_tris=3800000, seed=3800, hard=False):
        return cls((lib.rtxh_scene_bistro_class_hard if hard else lib.rtxh_scene_bistro_class)(target_tris, seed))

    @classmethod
    def from_obj(cls, files, mtl_dir, textures=True, cutouts=True, kd_alpha=False, normal_maps=True, bump=None, flip_y=False, spec_maps=True, emission_maps=True):
        """textures=False: decode no image; cutouts=False: bind no map_d image as an opacity map; kd_alpha=True: a material without a map_d whose map_Kd file is a
        32-bit TGA gets that texture as its opacity map too (rtx_render --no-textures / --no-cutouts / --kd-alpha); normal_maps=False: bind no norm image as a normal
        map; bump="normal": a material without a norm takes its map_Bump / bump image as a normal map, bump=S (a number): as a height map converted with strength S;
        flip_y=True: DirectX-style maps, green negated on load (--no-normal-maps / --bump-as-normal / --bump-height S / --normal-flip-y); spec_maps=False: bind no
        map_Ks / map_Pr / map_Pm image and leave the records as parsed (with them, a bound map sets a zero Ks / Pr / Pm to one: --no-spec-maps); emission_maps=False: bind no map_Ke image and leave the records as parsed (with them, a bound map sets a Ke of
        (0, 0, 0) to (1, 1, 1): --no-emission-maps)"""
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        flags = (0 if textures else 1) | (0 if cutouts else 2) | (4 if kd_alpha else 0) | (0 if normal_maps else 8) | (16 if bump == "normal" else 0) | (32 if flip_y else 0) | (0 if spec_maps else 64) | (0 if emission_maps else 128)
        if bump is not None and bump != "normal":
            return cls(lib.rtxh_scene_from_obj_ex2(arr, len(files), mtl_dir.encode(), flags, float(bump)))
        return cls(lib.rtxh_scene_from_obj_ex(arr, len(files), mtl_dir.encode(), flags))

    def set_camera(self, eye, center, up=(0.0, 1.0, 0.0)):
        e, c, u = (np.asarray(v, np.float32) for v in (eye, center, up))
        lib.rtxh_scene_set_camera(self._h, _fptr(e), _fptr(c), _fptr(u))
        self.eye, self.center, self.up = e, c, u

    def set_mesh_vertices(self, mesh, verts):
        """new vertices (n, 7) for mesh `mesh`, topology kept: same count, column 6 (Vertex.normal.w) unchanged; updates the handle and the numpy copy"""
        v = _f32(verts).reshape(-1, 7)
        if lib.rtxh_scene_set_mesh_vertices(self._h, int(mesh), _ptr(v), len(v)) != RTX_OK:
            raise RtxError("rtxh_scene_set_mesh_vertices failed: " + lib.rtxh_last_error().decode())
        old = self.meshes[mesh]
        self.meshes[mesh] = (v.copy(), old[1], old[2])
        self.cache_path = None                         # (a loaded scene no longer matches its file: Context.upload goes through the arrays)

    def bounds(self):
        """world-space bounding box of all instances -> (lo, hi)"""
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for mesh, m in self.instances:
            v = self.meshes[mesh][0][:, :3]
            if len(v):
                M = np.asarray(m, np.float32).reshape(4, 4)              # column-major 16 floats: element (r, c) at m[c * 4 + r]
                w = v @ M[:3, :3] + M[3, :3]
                lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
        return lo, hi

    def frame_bounds(self):
        """camera for a model that brings none (an OBJ asset): inside the bounding box at 40 % of its height, 35 % of the way in from one end of its longer horizontal
        axis, looking along that axis (Sponza: down the nave)"""
        lo, hi = self.bounds()
        c, ext = (lo + hi) * 0.5, hi - lo
        ax = 0 if ext[0] >= ext[2] else 2
        eye, ctr = c.copy(), c.copy()
        eye[1] = ctr[1] = lo[1] + 0.4 * ext[1]
        eye[ax] = c[ax] - 0.35 * ext[ax]
        self.set_camera(eye, ctr)

    def save(self, path):
        """write the binary scene cache: this scene + its BVH / shading records / LUTs (built on the host, no GPU needed)"""
        if lib.rtxh_scene_save(self._h, str(path).encode()) != RTX_OK:
            raise RtxError("rtxh_scene_save failed: " + lib.rtxh_last_error().decode())

    @classmethod
    def load(cls, path):
        """a scene from a binary cache file; Context.upload(scene) then hands the prebuilt arrays to the GPU without rebuilding"""
        s = cls(lib.rtxh_scene_load(str(path).encode()))
        s.cache_path = str(path)
        return s

    def small_records(self):
        """-> (records (n,20) f32, triangle ids (n,2) i32, delta, cm) of the tiny-scene pre-test, or None"""
        recs, ids = np.zeros((64, 20), np.float32), np.zeros((64, 2), np.int32)
        n, d, cm = _u32(), C.c_float(), C.c_float()
        if lib.rtxh_scene_small_records(self._h, _ptr(recs), _ptr(ids), 64, C.byref(n), C.byref(d), C.byref(cm)) != RTX_OK or n.value == 0:
            return None
        return recs[:n.value], ids[:n.value], d.value, cm.value

    def small_slabs(self):
        """-> (slabs (n,10) f32: w1 xyz, c1, h1, w2 xyz, c2, h2; excess (n,) f32, -1 = not a quad; pair mask) of the tiny-scene pre-test's slab form, or None"""
        slabs, ex = np.zeros((64, 10), np.float32), np.zeros(64, np.float32)
        n, m = _u32(), _u32()
        if lib.rtxh_scene_small_slabs(self._h, _ptr(slabs), _ptr(ex), 64, C.byref(n), C.byref(m)) != RTX_OK or n.value == 0:
            return None
        return slabs[:n.value], ex[:n.value], m.value

    def small_occluders(self):
        """number of leading tiny-scene records that are NOT faces of the scene's convex hull"""
        n = _u32()
        if lib.rtxh_scene_small_occluders(self._h, C.byref(n)) != RTX_OK:
            raise RtxError("rtxh_scene_small_occluders failed")
        return n.value

    def anyhit_order(self):
        """the any-hit visiting order the commit-time probe picks for this scene (0 slot order, 1 nearest octant first, 2 farthest first); host only"""
        n = _u32()
        if lib.rtxh_scene_anyhit_order(self._h, C.byref(n)) != RTX_OK:
            raise RtxError("rtxh_scene_anyhit_order failed")
        return n.value

    def view_proj(self, aspect):
        v, p = np.zeros(16, np.float32), np.zeros(16, np.float32)
        lib.rtxh_scene_view_proj(self._h, C.c_float(aspect), _fptr(v), _fptr(p))
        return v, p


def lookat(eye, center, up):
    e, c, u, v = _f32(eye), _f32(center), _f32(up), np.zeros(16, np.float32)
    lib.rtxh_lookat(_fptr(e), _fptr(c), _fptr(u), _fptr(v))
    return v


def perspective_fov_rh(fovy_rad, aspect, zn, zf):
    p = np.zeros(16, np.float32)
    lib.rtxh_perspective_fov_rh(fovy_rad, aspect, zn, zf, _fptr(p))
    return p


def ess_table_rows(rows):
    """an energy table for Context.set_ess_table: (rows, 16) float32, row r = generate_ess_lut(r / (rows - 1))"""
    return np.stack([generate_ess_lut(np.float32(r) / np.float32(rows - 1)) for r in range(rows)]).astype(np.float32)


def generate_ess_lut(roughness):
    lut = np.zeros(16, np.float32)
    lib.rtxh_generate_ess_lut(roughness, _fptr(lut))
    return lut


def mat4_inverse(m):
    m, o = _f32(m).reshape(16), np.zeros(16, np.float32)
    lib.rtxh_mat4_inverse(_fptr(m), _fptr(o))
    return o


def half_round(x):
    return lib.rtxh_half_round(C.c_float(x))


def read_image(path):
    """the host layer's texture readers (binary PPM / PGM, uncompressed or RLE 24- / 32-bit TGA) -> (H, W, 4) uint8, row 0 on top"""
    w, h = _u32(), _u32()
    if lib.rtxh_read_image(str(path).encode(), None, 0, C.byref(w), C.byref(h)) != RTX_OK:
        raise RtxError("read_image: " + lib.rtxh_last_error().decode())
    out = np.zeros((h.value, w.value, 4), np.uint8)
    lib.rtxh_read_image(str(path).encode(), _ptr(out), out.nbytes, C.byref(w), C.byref(h))
    return out


def read_hdr_image(path):
    """the host layer's high-dynamic-range readers (Radiance .hdr: RGBE, flat or new-style RLE, -Y H +X W; colour .pfm, either byte order) -> (H, W, 3) float32, row 0 on top"""
    w, h = _u32(), _u32()
    if lib.rtxh_read_hdr_image(str(path).encode(), None, 0, C.byref(w), C.byref(h)) != RTX_OK:
        raise RtxError("read_hdr_image: " + lib.rtxh_last_error().decode())
    out = np.zeros((h.value, w.value, 3), np.float32)
    lib.rtxh_read_hdr_image(str(path).encode(), _ptr(out), out.nbytes, C.byref(w), C.byref(h))
    return out


def latlong_to_octahedral(img, n):
    """a latitude-longitude image (H, W, 3) float32 — row 0 = +Y, column centre phi = 2 pi (x + 0.5) / W, direction (sin t sin p, cos t, -sin t cos p) — as the (n, n, 3)
    octahedral map Context.set_environment takes: every texel the mean of S x S nearest lookups, S = clamp(ceil(W / (2 n)), 2, 16)"""
    a = _f32(img)
    if a.ndim != 3 or a.shape[2] != 3:
        raise RtxError("latlong_to_octahedral: the image must be (H, W, 3) float32")
    out = np.zeros((int(n), int(n), 3), np.float32)
    if lib.rtxh_env_from_latlong(_ptr(a), a.shape[1], a.shape[0], int(n), _ptr(out)) != RTX_OK:
        raise RtxError("latlong_to_octahedral: " + lib.rtxh_last_error().decode())
    return out


def bvh_refit_check(before, after):
    a, b = _f32(before).reshape(-1, 9), _f32(after).reshape(-1, 9)
    return lib.rtxh_bvh_refit_check(_ptr(a), _ptr(b), len(a))


def bvh_check(world_tris):
    w = _f32(world_tris).reshape(-1, 9)
    nodes, depth, leaf = _u32(), _u32(), _u32()
    rc = lib.rtxh_bvh_check(_ptr(w), len(w), C.byref(nodes), C.byref(depth), C.byref(leaf))
    return rc, nodes.value, depth.value, leaf.value


def write_image(path, image):
    """(H, W, 4) uint8 sRGB -> .png / .ppm; (H, W, 4) float32 accumulation buffer -> .exr (xyz / count)"""
    a = np.ascontiguousarray(image)
    h, w = a.shape[:2]
    if path.endswith(".exr"):
        rc = lib.rtxh_write_exr(path.encode(), _ptr(_f32(a)), w, h)
    else:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        rc = (lib.rtxh_write_ppm if path.endswith(".ppm") else lib.rtxh_write_png)(path.encode(), _ptr(a), w, h)
    if rc != 0:
        raise RtxError("could not write " + path)


def bvh8_stats(world_tris):
    """(hist of leaf-slot sizes 0..4 + internal slots, wide node count) of the device tree built for these triangles"""
    w = _f32(world_tris).reshape(-1, 9)
    hist = np.zeros(6, np.uint32); nodes = _u32()
    rc = lib.rtxh_bvh8_stats(_ptr(w), len(w), _ptr(hist), C.byref(nodes))
    return rc, hist, nodes.value


def restir_halo_plan(params, halo_px):
    """rtx_restir_halo_plan (no context, no GPU): ([HaloPeer ...] in ascending rank order, send bytes, receive bytes) of params.shard_rank in the RTX_FLAG_BLOCK_TILES deal"""
    peers = (HaloPeer * 64)(); n = _u32(); st, rt_ = C.c_uint64(), C.c_uint64()
    if lib.rtx_restir_halo_plan(C.byref(params), halo_px, peers, 64, C.byref(n), C.byref(st), C.byref(rt_)) != 0:
        raise RtxError("rtx_restir_halo_plan: " + (lib.rtx_last_error(None) or b"").decode())
    return [peers[i] for i in range(n.value)], st.value, rt_.value


def bvh_option(key, value):
    """process-wide builder default (csrc/rtx_scene_host.hpp BvhBuildOptions); contexts created afterwards start with it"""
    if lib.rtxh_bvh_option(key.encode(), float(value)) != 0:
        raise RtxError("unknown BVH builder option " + key)


def bvh_replay(world_tris, rays8, any_hit=False, any_order=0):
    """host replay of the device traversal on the tree the current builder options give: (hits (n, 4): t, node steps, triangle tests, id bits; leaf entries)"""
    w = _f32(world_tris).reshape(-1, 9); r = _f32(rays8).reshape(-1, 8)
    out = np.zeros((len(r), 4), np.float32); refs = _u32()
    rc = lib.rtxh_bvh_replay(_ptr(w), len(w), _ptr(r), len(r), int(any_hit), any_order, _ptr(out), C.byref(refs))
    if rc != 0:
        raise RtxError("rtxh_bvh_replay failed: %d" % rc)
    return out, refs.value


def bvh8_check(world_tris):
    w = _f32(world_tris).reshape(-1, 9)
    nodes, stack = _u32(), _u32()
    rc = lib.rtxh_bvh8_check(_ptr(w), len(w), C.byref(nodes), C.byref(stack))
    return rc, nodes.value, stack.value


# ------------------------------------------------------------------------------------------------
# the hot path
# ------------------------------------------------------------------------------------------------
class Context:
    """One rtx_ctx (one GPU)."""

    def __init__(self, device=0):
        h = _vp()
        rc = lib.rtx_create(device, C.byref(h))
        if rc != RTX_OK:
            raise RtxError(f"rtx_create({device}) failed ({rc}): {lib.rtx_last_error(None).decode()}")
        self._h = h
        self.device = device
        self.width = self.height = 0

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:          # (at interpreter shutdown the module globals may already be gone: the process's exit frees the context)
            lib.rtx_destroy(h)

    __del__ = close

    def _ck(self, rc, what):
        if rc != RTX_OK:
            raise RtxError(f"{what} failed ({rc}): {lib.rtx_last_error(self._h).decode()}")

    def set_option(self, opt, value):
        self._ck(lib.rtx_set_option(self._h, opt, int(value)), "rtx_set_option")

    def set_stream(self, stream_handle):
        self._ck(lib.rtx_set_stream(self._h, _vp(stream_handle) if stream_handle else None), "rtx_set_stream")

    def set_materials(self, mats):
        m = _f32(mats).reshape(-1, 32)
        self._ck(lib.rtx_set_materials(self._h, _ptr(m), len(m)), "rtx_set_materials")

    def add_mesh(self, verts, indices, matids):
        v = _f32(verts).reshape(-1, 7)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(matids, dtype=np.uint32)
        out = _u32()
        self._ck(lib.rtx_add_mesh(self._h, _ptr(v), len(v), _ptr(i), len(i), _ptr(m), C.byref(out)), "rtx_add_mesh")
        return out.value

    def add_instance(self, mesh, o2w):
        m = _f32(o2w).reshape(16)
        out = _u32()
        self._ck(lib.rtx_add_instance(self._h, mesh, _fptr(m), C.byref(out)), "rtx_add_instance")
        return out.value

    def set_instance_transform(self, inst, o2w):
        m = _f32(o2w).reshape(16)
        self._ck(lib.rtx_set_instance_transform(self._h, inst, _fptr(m)), "rtx_set_instance_transform")

    def set_instance_visible(self, inst, visible):
        """InstanceMask 0 / 0xFF: a hidden instance exists for no ray and lights nothing, ids stay; the next commit() is a refit, never a rebuild"""
        self._ck(lib.rtx_set_instance_visible(self._h, int(inst), 1 if visible else 0), "rtx_set_instance_visible")

    def update_mesh_vertices(self, mesh, verts):
        """new vertices (n, 7) for a mesh whose topology stays; the next commit() re-derives this mesh's instances and refits (OPT_DEFORM_REBUILD)"""
        v = _f32(verts).reshape(-1, 7)
        self._ck(lib.rtx_update_mesh_vertices(self._h, int(mesh), _ptr(v), len(v)), "rtx_update_mesh_vertices")

    def set_mesh_uvs(self, mesh, uvs):
        """per-corner texture coordinates of a mesh: (index count, 2) float32, one (u, v) per index entry; None clears (every corner then has (0, 0))"""
        if uvs is None:
            self._ck(lib.rtx_set_mesh_uvs(self._h, int(mesh), None, 0), "rtx_set_mesh_uvs")
            return
        a = _f32(uvs).reshape(-1, 2)
        self._ck(lib.rtx_set_mesh_uvs(self._h, int(mesh), _ptr(a), len(a)), "rtx_set_mesh_uvs")

    def set_texture(self, tex, rgba8, srgb=True):
        """texture `tex` of the context's table (== the current count appends) := rgba8 (H, W, 4) uint8, row 0 on top, alpha ignored"""
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise RtxError("set_texture: pixels must be (H, W, 4) uint8")
        self._ck(lib.rtx_set_texture(self._h, int(tex), _ptr(a), a.shape[1], a.shape[0], TEX_SRGB if srgb else 0), "rtx_set_texture")

    def set_material_map(self, material, tex, slot=MAP_KD):
        """the material's map in `slot` (MAP_KD, MAP_OPACITY, MAP_NORMAL, MAP_KS, MAP_PR, MAP_PM, MAP_KE) := texture id `tex`, -1 / None = none"""
        self._ck(lib.rtx_set_material_map(self._h, int(material), int(slot), -1 if tex is None else int(tex)), "rtx_set_material_map")

    def texture_sample(self, tex, uvs):
        """the device's sampler at (n, 2) texture coordinates -> (n, 4) float32: r, g, b, 0"""
        a = _f32(uvs).reshape(-1, 2)
        out = np.zeros((len(a), 4), np.float32)
        self._ck(lib.rtx_debug_texture_sample(self._h, int(tex), _ptr(a), len(a), _ptr(out)), "rtx_debug_texture_sample")
        return out

    def albedo(self, hits4, rays8=None):
        """the device's per-hit diffuse colour at hit records (trace_closest) -> (n, 4) float32: Kd' (the material's Kd where it has no map), texture id bits or 0xFFFFFFFF"""
        h = _f32(hits4).reshape(-1, 4)
        r = _f32(rays8).reshape(-1, 8) if rays8 is not None else None
        out = np.zeros((len(h), 4), np.float32)
        self._ck(lib.rtx_debug_albedo(self._h, _ptr(r) if r is not None else None, _ptr(h), len(h), _ptr(out)), "rtx_debug_albedo")
        return out

    def opacity(self, hits4):
        """the alpha test of the cut-outs at hit records (trace_closest), by the device function the traversal runs -> (n, 2) float32: alpha, opacity texture id bits;
        (1.0, 0xFFFFFFFF) for a miss, a triangle that is not a cut-out triangle, and every hit while no cut-out is active"""
        h = _f32(hits4).reshape(-1, 4)
        out = np.zeros((len(h), 2), np.float32)
        self._ck(lib.rtx_debug_opacity(self._h, _ptr(h), len(h), _ptr(out)), "rtx_debug_opacity")
        return out

    def shading_normal(self, rays8, hits4):
        """the shading normal under the normal maps at (ray, hit record) pairs (trace_closest), by the device functions k_shade runs -> (n, 4) float32: n', normal
        texture id bits or 0xFFFFFFFF (an emitter, a material without a map, no normal map active: n' is surface()'s normal); a miss gives (0, 0, 0, 0xFFFFFFFF)"""
        r = _f32(rays8).reshape(-1, 8); h = _f32(hits4).reshape(-1, 4)
        out = np.zeros((len(h), 4), np.float32)
        self._ck(lib.rtx_debug_shading_normal(self._h, _ptr(r), _ptr(h), len(h), _ptr(out)), "rtx_debug_shading_normal")
        return out

    def set_ess_table(self, table):
        """the energy table of the specular maps: (rows, 16) float32, row r = the multiscatter LUT of roughness r / (rows - 1), 2 <= rows <= 256; None clears.  Needs commit()"""
        if table is None:
            self._ck(lib.rtx_set_ess_table(self._h, None, 0), "rtx_set_ess_table")
            return
        a = _f32(table)
        if a.ndim != 2 or a.shape[1] != 16:
            raise ValueError("set_ess_table: a (rows, 16) array")
        self._ck(lib.rtx_set_ess_table(self._h, _ptr(a), a.shape[0]), "rtx_set_ess_table")

    def specular(self, hits4):
        """Ks', Pr', Pm' under the specular maps at hit records (trace_closest), by the device function k_shade runs -> ((n, 5) float32, (n, 3) uint32: the ks / pr / pm
        texture ids or 0xFFFFFFFF); a miss gives zeros and 0xFFFFFFFF"""
        h = _f32(hits4).reshape(-1, 4)
        out = np.zeros((len(h), 8), np.float32)
        self._ck(lib.rtx_debug_specular(self._h, _ptr(h), len(h), _ptr(out)), "rtx_debug_specular")
        return out[:, :5].copy(), out[:, 5:].copy().view(np.uint32)

    def emission(self, hits4):
        """Ke' and q under the emission maps at hit records (trace_closest), by the device function k_shade runs -> ((n, 4) float32: Ke', q[prim]; (n,) uint32: the
        emission texture id or 0xFFFFFFFF); a non-emitter or a miss gives zeros and 0xFFFFFFFF"""
        h = _f32(hits4).reshape(-1, 4)
        out = np.zeros((len(h), 8), np.float32)
        self._ck(lib.rtx_debug_emission(self._h, _ptr(h), len(h), _ptr(out)), "rtx_debug_emission")
        return out[:, :4].copy(), out[:, 4].copy().view(np.uint32)

    def light_sample(self, seeds):
        """the first half of a triangle-light NEE sample at (n, 2) uint32 seeds, by the device functions nee_sample runs -> dict: light (n,) uint32, point (n, 3), st (n, 2),
        em (n, 3) = em * tl, pdf_l (n,), seed (n, 2) uint32 after the three draws; RtxError (RTX_ERR_STATE) for a scene without a light list"""
        a = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 2)
        out = np.zeros((len(a), 12), np.float32)
        self._ck(lib.rtx_debug_light_sample(self._h, _ptr(a), len(a), _ptr(out)), "rtx_debug_light_sample")
        return dict(light=out[:, 0].copy().view(np.uint32), point=out[:, 1:4].copy(), st=out[:, 4:6].copy(), em=out[:, 6:9].copy(), pdf_l=out[:, 9].copy(),
                    seed=out[:, 10:12].copy().view(np.uint32))

    def ess(self, material, pr, ndotv):
        """the Ess the view terms would use for `material` at (Pr', NdotV) pairs: the energy table where the material has a roughness map and a table is set, else its LUT"""
        a = _f32(pr).reshape(-1); b = _f32(ndotv).reshape(-1)
        if len(a) != len(b):
            raise ValueError("ess: pr and ndotv differ in length")
        out = np.zeros(len(a), np.float32)
        self._ck(lib.rtx_debug_ess(self._h, int(material), _ptr(a), _ptr(b), len(a), _ptr(out)), "rtx_debug_ess")
        return out

    def tri_tangents(self, first=0, count=None):
        """the device's tangent table: (count, 6) float32, object-space T and B per global triangle id; RtxError (RTX_ERR_STATE) while no normal map is active"""
        if count is None:
            count = self.stats().triangles - first
        out = np.zeros((count, 6), np.float32)
        self._ck(lib.rtx_debug_tri_tangents(self._h, int(first), int(count), _ptr(out)), "rtx_debug_tri_tangents")
        return out

    def bind_maps(self, scene):
        """the optional texture attributes of a scene (duck-typed): `uvs` — per mesh an (index count, 2) array or None; `textures` — a list whose entries are (H, W, 4)
        uint8 arrays or (array, srgb) pairs, anything else (a file name without pixels) is skipped; `material_maps` — per material an index into `textures` or -1 / None;
        `opacity_maps`, `normal_maps`, `ks_maps`, `pr_maps`, `pm_maps`, `ke_maps` — likewise for the MAP_OPACITY, MAP_NORMAL, MAP_KS, MAP_PR, MAP_PM and MAP_KE slots; `ess_table` — a
        (rows, 16) energy table for set_ess_table, or None.  A map whose texture was skipped is not bound."""
        for mesh, uv in enumerate(getattr(scene, "uvs", None) or []):
            if uv is not None and len(uv):
                self.set_mesh_uvs(mesh, uv)
        ids = {}
        texs = getattr(scene, "texture_pixels", None)            # (a host-loaded Scene keeps the file names in `textures` and the decoded images here)
        for i, t in enumerate((getattr(scene, "textures", None) if texs is None else texs) or []):
            px, srgb = t if isinstance(t, tuple) else (t, True)
            if isinstance(px, np.ndarray) and px.ndim == 3:
                ids[i] = len(ids)
                self.set_texture(ids[i], px, srgb)
        for attr, slot, _ in _SCENE_MAP_SLOTS:
            for mat, t in enumerate(getattr(scene, attr, None) or []):
                if t is not None and t >= 0 and t in ids:
                    self.set_material_map(mat, ids[t], slot)
        if getattr(scene, "ess_table", None) is not None:
            self.set_ess_table(scene.ess_table)

    def set_environment(self, img, to_world=None, scale=1.0, hidden=False):
        """environment lighting: img = (N, N, 3) float32 octahedral map of linear radiance (row = v, column = u; latlong_to_octahedral makes one), or None to clear;
        to_world = 16 floats (column-vector matrix, only its orthonormal upper 3x3 is used) or None = identity; scale multiplies the radiance; hidden: camera rays that
        miss stay black.  Needs commit()"""
        if img is None:
            self._ck(lib.rtx_set_environment(self._h, None, 0, None, 1.0, 0), "rtx_set_environment")
            self._env_n = 0
            return
        a = _f32(img)
        if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
            raise RtxError("set_environment: the map must be (N, N, 3) float32")
        m = _f32(to_world).reshape(16) if to_world is not None else None
        self._ck(lib.rtx_set_environment(self._h, _ptr(a), a.shape[0], _ptr(m) if m is not None else None, float(scale), ENV_HIDDEN if hidden else 0), "rtx_set_environment")
        self._env_n = a.shape[0]

    def env_tables(self):
        """the environment's tables as the device holds them -> texels (N, N, 4) float32 (r, g, b, pmf), marginal (N,), conditional (N, N)"""
        n = getattr(self, "_env_n", 0)
        if not n:
            raise RtxError("env_tables: no environment set through this Context")
        tex, marg, cond = np.zeros((n, n, 4), np.float32), np.zeros(n, np.float32), np.zeros((n, n), np.float32)
        self._ck(lib.rtx_debug_env_tables(self._h, _ptr(tex), _ptr(marg), _ptr(cond)), "rtx_debug_env_tables")
        return tex, marg, cond

    def env_sample(self, seeds):
        """the device's environment sampler at (n, 2) uint32 seeds -> (n, 12) float32: world direction, pdf, L, texel bits, seed after the four draws (bits), 0, 0"""
        s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros((len(s), 12), np.float32)
        self._ck(lib.rtx_debug_env_sample(self._h, _ptr(s), len(s), _ptr(out)), "rtx_debug_env_sample")
        return out

    def env_eval(self, dirs):
        """the device's environment lookup at (n, 3) world directions -> (n, 8) float32: L, pdf, texel bits, r3, 0, 0"""
        d = _f32(dirs).reshape(-1, 3)
        out = np.zeros((len(d), 8), np.float32)
        self._ck(lib.rtx_debug_env_eval(self._h, _ptr(d), len(d), _ptr(out)), "rtx_debug_env_eval")
        return out

    def commit(self):
        self._ck(lib.rtx_commit_scene(self._h), "rtx_commit_scene")

    def set_camera(self, view, proj):
        v, p = _f32(view).reshape(16), _f32(proj).reshape(16)
        self._ck(lib.rtx_set_camera(self._h, _fptr(v), _fptr(p)), "rtx_set_camera")

    def set_lens(self, radius, focus=1.0):
        """the thin-lens camera (rtx_set_lens): aperture radius and focus distance along the view axis, world units; radius 0 or set_lens(None) = the pinhole; a Lens is
        passed as it is.  Camera state: no commit, survives set_camera, clears nothing"""
        if radius is None:
            self._ck(lib.rtx_set_lens(self._h, None), "rtx_set_lens")
            return
        lens = radius if isinstance(radius, Lens) else Lens(float(radius), float(focus))
        self._ck(lib.rtx_set_lens(self._h, C.byref(lens)), "rtx_set_lens")

    def focus_distance_at(self, width, height, x, y):
        """autofocus (rtx_focus_distance_at): the view-axis depth of the first hit of pixel (x, y)'s pinhole ray in a width x height image; 0.0 = a miss"""
        d = C.c_float()
        self._ck(lib.rtx_focus_distance_at(self._h, width, height, x, y, C.byref(d)), "rtx_focus_distance_at")
        return np.float32(d.value)

    def save_scene_cache(self, path):
        self._ck(lib.rtx_save_scene_cache(self._h, str(path).encode()), "rtx_save_scene_cache")

    def load_scene_cache(self, path):
        self._ck(lib.rtx_load_scene_cache(self._h, str(path).encode()), "rtx_load_scene_cache")

    def upload(self, scene, aspect):
        """rtx_set_materials / add_mesh / add_instance / commit / set_camera from a Scene (array path); a Scene.load()-ed scene
        goes through rtx_load_scene_cache instead (prebuilt BVH)."""
        if getattr(scene, "cache_path", None):
            self.load_scene_cache(scene.cache_path)
            self.set_camera(*scene.view_proj(aspect))
            return
        self.set_materials(scene.materials)
        for v, i, m in scene.meshes:
            self.add_mesh(v, i, m)
        for mesh, o2w in scene.instances:
            self.add_instance(mesh, o2w)
        self.bind_maps(scene)
        env = getattr(scene, "environment", None)                 # an (N, N, 3) map, or a dict of set_environment's arguments (img, to_world, scale, hidden)
        if env is not None:
            self.set_environment(**env) if isinstance(env, dict) else self.set_environment(env)
        self.commit()
        self.set_camera(*scene.view_proj(aspect))

    def bind_accum(self, device_ptr, nbytes):
        self._ck(lib.rtx_bind_accum(self._h, _vp(device_ptr) if device_ptr else None, nbytes), "rtx_bind_accum")

    def clear(self, width, height):
        self.width, self.height = width, height
        self._ck(lib.rtx_clear_accum(self._h, width, height), "rtx_clear_accum")

    def render(self, params):
        self.width, self.height = params.width, params.height
        self._ck(lib.rtx_render(self._h, C.byref(params)), "rtx_render")

    def render_adaptive(self, params, min_spp, step_spp, max_spp, threshold, dark_floor=0.0):
        """rtx_render_adaptive: sample every 256-slot chunk until its pixels pass the noise threshold or it holds max_spp samples (params.spp is ignored) -> AdaptiveResult"""
        self.width, self.height = params.width, params.height
        a, res = Adaptive(int(min_spp), int(step_spp), int(max_spp), float(threshold), float(dark_floor)), AdaptiveResult()
        self._ck(lib.rtx_render_adaptive(self._h, C.byref(params), C.byref(a), C.byref(res)), "rtx_render_adaptive")
        return res

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(lib.rtx_read_accum(self._h, _ptr(out), out.nbytes), "rtx_read_accum")
        return out

    def denoise(self, width, height, levels=0, sigma_color=0.0, sigma_plane=0.0, normal_power_log2=0, result=True, albedo=False, mapped_normals=False, variance=False, sigma_var=0.0):
        """rtx_denoise: the edge-avoiding a-trous filter over the mean of u1, guided by first-hit position, normal and material (0 = a field's default) -> DenoiseResult.
        albedo: RTX_DENOISE_ALBEDO, filter the image divided by the first hit's Kd' so that texture detail survives; mapped_normals: RTX_DENOISE_MAPPED_NORMALS, the normal
        stop compares normal-mapped shading normals.  result=False passes no result struct: on a caller-bound stream the call then only enqueues (no host join) and returns None.
        variance=True: rtx_denoise_variance — the colour stop is scaled by each pixel's own noise (sigma_var standard deviations, 0 = 4) instead of sigma_color, which must
        then stay 0; the image must have been sampled by render_adaptive alone (threshold 0 for a fixed sample count)"""
        flags = (DENOISE_ALBEDO if albedo else 0) | (DENOISE_MAPPED_NORMALS if mapped_normals else 0)
        if variance:
            if sigma_color:
                raise ValueError("denoise: sigma_color has no meaning with variance=True (sigma_var scales the colour stop)")
            vp = DenoiseVarParams(int(levels), int(normal_power_log2), float(sigma_var), float(sigma_plane), flags)
            res = DenoiseResult() if result else None
            self._ck(lib.rtx_denoise_variance(self._h, int(width), int(height), C.byref(vp), C.byref(res) if result else None), "rtx_denoise_variance")
            return res
        if sigma_var:
            raise ValueError("denoise: sigma_var needs variance=True")
        dp = DenoiseParams(int(levels), int(normal_power_log2), float(sigma_color), float(sigma_plane), (C.c_uint32 * 4)(flags, 0, 0, 0))
        res = DenoiseResult() if result else None
        self._ck(lib.rtx_denoise(self._h, int(width), int(height), C.byref(dp), C.byref(res) if result else None), "rtx_denoise")
        return res

    def read_denoised(self):
        """the denoised image (H, W, 4) float32: xyz, w = 1"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(lib.rtx_read_denoised(self._h, _ptr(out), out.nbytes), "rtx_read_denoised")
        return out

    def read_denoised_srgb8(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._ck(lib.rtx_read_denoised_srgb8(self._h, _ptr(out), out.nbytes), "rtx_read_denoised_srgb8")
        return out

    def read_adaptive_half(self):
        """`half` (H, W, 4) float32: render_adaptive's running sum of the odd sample ids, the second input of denoise(variance=True)"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(lib.rtx_read_adaptive_half(self._h, _ptr(out), out.nbytes), "rtx_read_adaptive_half")
        return out

    def denoise_variance_input(self, width, height, albedo=False):
        """(H, W, 2) float32: level 0's (v, gv) as denoise(variance=True) reads them — the variance of the mean's luminance and its 3 x 3 prefilter; (0, 0) where not filterable"""
        out = np.zeros((height, width, 2), np.float32)
        self._ck(lib.rtx_debug_denoise_variance(self._h, int(width), int(height), DENOISE_ALBEDO if albedo else 0, _ptr(out)), "rtx_debug_denoise_variance")
        return out

    def denoise_guides(self, width, height):
        """the filter's guides (H, W, 8) float32: P3, material word as uint bits (0xFFFFFFFF = not filterable by geometry, P and n then 0), n3, 0"""
        out = np.zeros((height, width, 8), np.float32)
        self._ck(lib.rtx_debug_denoise_guides(self._h, int(width), int(height), _ptr(out)), "rtx_debug_denoise_guides")
        return out

    def denoise_map_guides(self, width, height):
        """the filter's map guides (H, W, 8) float32: A3 = max(Kd', 2^-6), 0, nm3 = the normal-mapped shading normal, 0; (1, 1, 1, 0, 0, 0, 0, 0) where not filterable by geometry"""
        out = np.zeros((height, width, 8), np.float32)
        self._ck(lib.rtx_debug_denoise_map_guides(self._h, int(width), int(height), _ptr(out)), "rtx_debug_denoise_map_guides")
        return out

    def render_v6_pass1(self, params):
        """the reference's own pass 1 (RIS direct light + SamplePathSimple); see rtx_render_v6_pass1"""
        self.width, self.height = params.width, params.height
        self._ck(lib.rtx_render_v6_pass1(self._h, C.byref(params)), "rtx_render_v6_pass1")

    def render_restir(self, params):
        """`params.spp` consecutive ReSTIR frames (pass 1 + temporal + spatial) with the current camera"""
        self.width, self.height = params.width, params.height
        self._ck(lib.rtx_render_restir(self._h, C.byref(params)), "rtx_render_restir")

    def restir_state_slab_bytes(self, params):
        b = C.c_size_t()
        self._ck(lib.rtx_restir_state_slab_bytes(C.byref(params), C.byref(b)), "rtx_restir_state_slab_bytes")
        return b.value

    def restir_pack_state(self, params, device_ptr):
        self._ck(lib.rtx_restir_pack_state(self._h, C.byref(params), _vp(device_ptr)), "rtx_restir_pack_state")

    def restir_unpack_state(self, params, device_ptr):
        self._ck(lib.rtx_restir_unpack_state(self._h, C.byref(params), _vp(device_ptr)), "rtx_restir_unpack_state")

    def restir_pack_halo(self, params, halo_px, device_ptr):
        self._ck(lib.rtx_restir_pack_halo(self._h, C.byref(params), halo_px, _vp(device_ptr)), "rtx_restir_pack_halo")

    def restir_unpack_halo(self, params, halo_px, device_ptr):
        self._ck(lib.rtx_restir_unpack_halo(self._h, C.byref(params), halo_px, _vp(device_ptr)), "rtx_restir_unpack_halo")

    def restir_reset(self):
        self._ck(lib.rtx_restir_reset(self._h), "rtx_restir_reset")

    def read_restir_last(self):
        n = lib.rtx_pass1_slots(self.width, self.height)
        di, gi, sd = np.zeros((n, 40), np.uint8), np.zeros((n, 40), np.uint8), np.zeros((n, 60), np.uint8)
        self._ck(lib.rtx_read_restir_last(self._h, _ptr(di), _ptr(gi), _ptr(sd), n), "rtx_read_restir_last")
        return di, gi, sd

    def read_pass1_buffers(self):
        n = lib.rtx_pass1_slots(self.width, self.height)
        di, gi, sd = np.zeros((n, 40), np.uint8), np.zeros((n, 40), np.uint8), np.zeros((n, 60), np.uint8)
        self._ck(lib.rtx_read_pass1_buffers(self._h, _ptr(di), _ptr(gi), _ptr(sd), n), "rtx_read_pass1_buffers")
        return di, gi, sd

    def read_srgb8(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._ck(lib.rtx_read_srgb8(self._h, _ptr(out), out.nbytes), "rtx_read_srgb8")
        return out

    def read_layer(self, layer, width=None, height=None):
        """gOutput layer `layer`: 0 = the image, 10-17 = first-hit debug attributes, others black (rtx_read_layer)"""
        w, h = width or self.width, height or self.height
        out = np.zeros((h, w, 4), np.uint8)
        self._ck(lib.rtx_read_layer(self._h, layer, w, h, _ptr(out), out.nbytes), "rtx_read_layer")
        return out

    def stats(self):
        s = Stats()
        self._ck(lib.rtx_get_stats(self._h, C.byref(s)), "rtx_get_stats")
        return s

    def lights(self):
        n = _u32()
        self._ck(lib.rtx_get_lights(self._h, None, 0, C.byref(n)), "rtx_get_lights")
        out = np.zeros((n.value, 20), np.float32)
        if n.value:
            self._ck(lib.rtx_get_lights(self._h, _ptr(out), n.value, C.byref(n)), "rtx_get_lights")
        return out

    def slab_bytes(self, params):
        b = C.c_size_t()
        self._ck(lib.rtx_shard_slab_bytes(C.byref(params), C.byref(b)), "rtx_shard_slab_bytes")
        return b.value

    def pack_tiles(self, params, device_ptr):
        self._ck(lib.rtx_pack_tiles(self._h, C.byref(params), _vp(device_ptr)), "rtx_pack_tiles")

    def unpack_tiles(self, params, device_ptr):
        self.width, self.height = params.width, params.height
        self._ck(lib.rtx_unpack_tiles(self._h, C.byref(params), _vp(device_ptr)), "rtx_unpack_tiles")

    # kernel-level entry points
    def primary_rays(self, params, sample_id=1):
        out = np.zeros((params.height * params.width, 8), np.float32)
        self._ck(lib.rtx_debug_primary_rays(self._h, C.byref(params), sample_id, _ptr(out)), "rtx_debug_primary_rays")
        return out

    def primary_seeds(self, params, sample_id=1):
        """the seed state (s0, s1) the paths of primary_rays start from: after the jitter's draws and the lens's -> (H * W, 2) uint32"""
        out = np.zeros((params.height * params.width, 2), np.uint32)
        self._ck(lib.rtx_debug_primary_seeds(self._h, C.byref(params), sample_id, _ptr(out)), "rtx_debug_primary_seeds")
        return out

    def trace_closest(self, rays8):
        r = _f32(rays8).reshape(-1, 8)
        out = np.zeros((len(r), 4), np.float32)
        self._ck(lib.rtx_debug_trace_closest(self._h, _ptr(r), len(r), _ptr(out)), "rtx_debug_trace_closest")
        return out

    def trace_any(self, rays8):
        r = _f32(rays8).reshape(-1, 8)
        out = np.zeros(len(r), np.uint8)
        self._ck(lib.rtx_debug_trace_any(self._h, _ptr(r), len(r), _ptr(out)), "rtx_debug_trace_any")
        return out

    def tree_hash(self):
        """(hash of the node records, hash of the leaf-ordered triangle records) of the wide tree as the device holds it"""
        h = (C.c_uint64 * 2)()
        self._ck(lib.rtx_debug_tree_hash(self._h, h), "rtx_debug_tree_hash")
        return int(h[0]), int(h[1])

    def tree_cost(self):
        """(visit cost of the resident tree now, right after its last build): sum over the wide nodes of half-area(node) / half-area(root); reproducible to the bit"""
        out = (C.c_double * 2)()
        self._ck(lib.rtx_debug_tree_cost(self._h, out), "rtx_debug_tree_cost")
        return float(out[0]), float(out[1])

    def read_tree(self, which=0):
        """(node records (n, 80) uint8, leaf-ordered triangle records (m, 12) float32) of the device (which=0) or of the host builder's mirror (which=1)"""
        st = self.stats()
        nodes, tris = np.empty((st.bvh_nodes, 80), np.uint8), np.empty((st.bvh_refs, 12), np.float32)
        self._ck(lib.rtx_debug_read_tree(self._h, int(which), nodes.ctypes.data_as(C.c_void_p), C.c_uint64(nodes.nbytes), tris.ctypes.data_as(C.c_void_p), C.c_uint64(tris.nbytes)), "rtx_debug_read_tree")
        return nodes, tris

    def read_host_build(self):
        """(binary tree (n, 16) float32, leaf order (m,) uint32) as the host builder keeps them for refits; empty after a GPU build"""
        nb, lb = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib.rtx_debug_read_host_build(self._h, None, C.byref(nb), None, C.byref(lb)), "rtx_debug_read_host_build")
        nodes, order = np.empty((nb.value // 64, 16), np.float32), np.empty(lb.value // 4, np.uint32)
        self._ck(lib.rtx_debug_read_host_build(self._h, nodes.ctypes.data_as(C.c_void_p), C.byref(nb), order.ctypes.data_as(C.c_void_p), C.byref(lb)), "rtx_debug_read_host_build")
        return nodes, order

    def host_checksums(self):
        """hashes of the host-side scene and build state: (mesh indices, mesh vertices, materials, instances, leaf order, binary tree, wide mirror, shade + objtris + slots)"""
        h = (C.c_uint64 * 8)()
        self._ck(lib.rtx_debug_host_checksums(self._h, h), "rtx_debug_host_checksums")
        return tuple(int(x) for x in h)

    def build_info(self):
        """the last geometry-changing commit: dict(ms=(boxes + keys, sort, PLOC, top on the host, layout), nodes, refs, ploc_rounds, clusters_top); ms all 0 after a host build"""
        ms, cn = (C.c_double * 5)(), (C.c_uint32 * 4)()
        self._ck(lib.rtx_debug_build_info(self._h, ms, cn), "rtx_debug_build_info")
        return dict(ms=tuple(ms), nodes=cn[0], refs=cn[1], ploc_rounds=cn[2], clusters_top=cn[3])

    def trace_counters(self):
        """(node steps, triangle tests) of the closest-hit rays and of the any-hit rays since the last call (OPT_TRACE_COUNTERS 1)"""
        out = (C.c_uint64 * 4)()
        self._ck(lib.rtx_debug_trace_counters(self._h, out), "rtx_debug_trace_counters")
        return tuple(int(v) for v in out)

    def validate_bvh(self):
        """0 when the resident wide BVH (as built, or as refitted on the GPU) covers every triangle inside its decoded boxes"""
        return lib.rtx_debug_validate_bvh(self._h)

    def trace_stats(self, rays8):
        """(n,4): t, node steps, triangle tests, prim bits of a closest-hit BVH traversal"""
        r = _f32(rays8).reshape(-1, 8)
        out = np.zeros((len(r), 4), np.float32)
        self._ck(lib.rtx_debug_trace_stats(self._h, _ptr(r), len(r), _ptr(out)), "rtx_debug_trace_stats")
        return out

    def surface(self, rays8, hits4):
        r, h = _f32(rays8).reshape(-1, 8), _f32(hits4).reshape(-1, 4)
        out = np.zeros((len(r), 16), np.float32)
        self._ck(lib.rtx_debug_surface(self._h, _ptr(r), _ptr(h), len(r), _ptr(out)), "rtx_debug_surface")
        return out

    def bsdf_eval(self, mat_id, flags, n_wo_wi):
        q = _f32(n_wo_wi).reshape(-1, 9)
        out = np.zeros((len(q), 8), np.float32)
        self._ck(lib.rtx_debug_bsdf_eval(self._h, mat_id, flags, _ptr(q), len(q), _ptr(out)), "rtx_debug_bsdf_eval")
        return out

    def bsdf_sample(self, mat_id, flags, n_wo_seed):
        q = _f32(n_wo_seed).reshape(-1, 8)
        out = np.zeros((len(q), 8), np.float32)
        self._ck(lib.rtx_debug_bsdf_sample(self._h, mat_id, flags, _ptr(q), len(q), _ptr(out)), "rtx_debug_bsdf_sample")
        return out

    def tea(self, seed, n):
        s = (C.c_uint32 * 2)(*seed)
        out = np.zeros(n, np.float32)
        self._ck(lib.rtx_debug_tea(self._h, s, n, _ptr(out)), "rtx_debug_tea")
        return out, (s[0], s[1])


class Renderer:
    """The headless Renderer facade (host/Renderer.h) through its C entry points."""

    def __init__(self, width, height, name="rtx", device=0):
        self._h = lib.rtxh_renderer_create(width, height, name.encode(), device)
        self.width, self.height = width, height

    def _ck(self, rc, what):
        if rc != RTX_OK:
            raise RtxError(f"{what} failed: {lib.rtxh_last_error().decode()}")

    def set_scene(self, scene):
        self._ck(lib.rtxh_renderer_set_scene(self._h, scene._h), "set_scene")

    @property
    def params(self):
        return lib.rtxh_renderer_params(self._h).contents

    @property
    def restir_params(self):
        return lib.rtxh_renderer_restir_params(self._h).contents

    def set_mode(self, mode):
        """0 = path tracer (rtx_render), 1 = the reference's ReSTIR frame (rtx_render_restir), one frame per on_render"""
        self._ck(lib.rtxh_renderer_set_mode(self._h, int(mode)), "set_mode")

    def set_option(self, opt, value):
        h = lib.rtxh_renderer_context(self._h)
        if not h or lib.rtx_set_option(h, int(opt), int(value)) != RTX_OK:
            raise RtxError("set_option: " + (lib.rtx_last_error(h).decode() if h else "renderer not initialised"))

    def on_init(self):
        self._ck(lib.rtxh_renderer_on_init(self._h), "OnInit")

    def on_update(self):
        self._ck(lib.rtxh_renderer_on_update(self._h), "OnUpdate")

    def set_instance_transform(self, instance, o2w16):
        """Renderer::SetInstanceTransform: takes effect in the next on_update (transform-only commit = GPU refit)"""
        m = _f32(o2w16).reshape(16)
        self._ck(lib.rtxh_renderer_set_instance_transform(self._h, int(instance), _ptr(m)), "SetInstanceTransform")

    def set_instance_visible(self, instance, visible):
        """Renderer::SetInstanceVisible: takes effect in the next on_update (a refit of the resident tree)"""
        self._ck(lib.rtxh_renderer_set_instance_visible(self._h, int(instance), 1 if visible else 0), "SetInstanceVisible")

    def set_mesh_vertices(self, mesh, verts):
        """Renderer::SetMeshVertices: new vertices (n, 7) for a model whose topology stays; takes effect in the next on_update (vertex-changing commit = re-flatten + refit)"""
        v = _f32(verts).reshape(-1, 7)
        self._ck(lib.rtxh_renderer_set_mesh_vertices(self._h, int(mesh), _ptr(v), len(v)), "SetMeshVertices")

    def on_render(self):
        self._ck(lib.rtxh_renderer_on_render(self._h), "OnRender")

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(lib.rtxh_renderer_read_accum(self._h, _ptr(out), out.nbytes), "read_accum")
        return out

    def read_denoised(self, **kw):
        """rtx_denoise over the accumulated image (every default unless Context.denoise's keywords say otherwise) and its read: (H, W, 4) float32, w = 1; the accumulation is left alone"""
        h = lib.rtxh_renderer_context(self._h)
        if not h:
            raise RtxError("read_denoised: renderer not initialised")
        c = Context.__new__(Context)                    # a borrowed view of the renderer's context: never closed from here
        c._h, c.width, c.height = None, self.width, self.height
        try:
            c._h = h
            c.denoise(self.width, self.height, **kw)
            return c.read_denoised()
        finally:
            c._h = None

    def denoise_variance(self, levels=0, sigma_var=0.0, sigma_plane=0.0, normal_power_log2=0, albedo=False, mapped_normals=False):
        """Renderer::DenoiseVariance: rtx_denoise_variance on the renderer's context, whose image must have been sampled by render_adaptive alone -> DenoiseResult"""
        flags = (DENOISE_ALBEDO if albedo else 0) | (DENOISE_MAPPED_NORMALS if mapped_normals else 0)
        vp, res = DenoiseVarParams(int(levels), int(normal_power_log2), float(sigma_var), float(sigma_plane), flags), DenoiseResult()
        rc = lib.rtxh_renderer_denoise_variance(self._h, C.byref(vp), C.byref(res))
        if rc != RTX_OK:
            h = lib.rtxh_renderer_context(self._h)
            raise RtxError(f"DenoiseVariance failed ({rc}): " + (lib.rtx_last_error(h).decode() if h else "renderer not initialised"))
        return res

    def read_output(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._ck(lib.rtxh_renderer_read_output(self._h, _ptr(out), out.nbytes), "read_output")
        return out

    def on_key_up(self, key):
        self._ck(lib.rtxh_renderer_on_key_up(self._h, ord(key) if isinstance(key, str) else key), "OnKeyUp")

    @property
    def display_layer(self):
        return lib.rtxh_renderer_display_layer(self._h)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.rtxh_renderer_destroy(h)

    __del__ = close

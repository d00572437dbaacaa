"""ctypes mirror of the C boundary: include/raytracer.h (the reference's structs,
reference raytracer.h:60-131), include/rt_hip.h (the HIP shim's C-ABI) and
raytracer.c_amd/host/scenes.h.  Plumbing only: no arithmetic happens here.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # raytracer.c_amd/
REPO_ROOT = os.path.dirname(PKG_DIR)
SHIM_PATH = os.environ.get("RT_HIP_SHIM_PATH") or os.path.join(PKG_DIR, "csrc", "librt_hip.so")  # env: dev builds
HOST_PATH = os.path.join(PKG_DIR, "host", "libraytracer_amd.so")

M_DEFAULT, M_REFLECTION, M_REFRACTION, M_CHECKERED = 2, 4, 8, 16
TILE, TILE_PIXELS, TILE_FLOATS = 8, 64, 192
STAT_RAYS, STAT_CASTS, STAT_TESTS, STAT_SAMPLES, NSTATS = 0, 1, 2, 3, 4
FAIL_ALLOC_PARK_WS, FAIL_ALLOC_WIDE_PEND, FAIL_ALLOC_TAIL_WS = 1, 2, 4   # rt_hip_selftest_fail_alloc
FAIL_PEND_SLOT, FAIL_PARK_SLOT = 1, 2             # rt_hip_launch_status
EINVAL = -2                                       # RT_HIP_EINVAL
# render_progressive's per-pass callback: (samples done, budget, kernel seconds of the pass, user)
PASS_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_double, C.c_void_p)


class Vec2(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double)]


class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]

    def tuple(self):
        return (self.x, self.y, self.z)


class Object(C.Structure):  # reference raytracer.h:104-111 == RtHipSphere, 88 B
    _fields_ = [("flags", C.c_uint32), ("radius", C.c_double), ("center", Vec3), ("color", Vec3),
                ("emission", Vec3)]


class Vertex(C.Structure):  # reference raytracer.h:61 == RtHipVertex, 40 B
    _fields_ = [("pos", Vec3), ("tex", Vec2)]


class TriangleMesh(C.Structure):  # reference raytracer.h:77-81
    _fields_ = [("num_triangles", C.c_size_t), ("vertices", C.POINTER(Vertex))]


class MeshObject(C.Structure):  # include/raytracer.h extension
    _fields_ = [("flags", C.c_uint32), ("color", Vec3), ("emission", Vec3), ("mesh", TriangleMesh)]


class Camera(C.Structure):  # reference raytracer.h:121-124 == RtHipCamera, 96 B
    _fields_ = [("position", Vec3), ("horizontal", Vec3), ("vertical", Vec3), ("lower_left_corner", Vec3)]


class Options(C.Structure):  # reference raytracer.h:126-131, 56 B
    _fields_ = [("background", Vec3), ("result", C.c_char_p), ("obj", C.c_char_p), ("width", C.c_int),
                ("height", C.c_int), ("samples", C.c_int)]


class Ray(C.Structure):
    _fields_ = [("origin", Vec3), ("direction", Vec3)]


class Hit(C.Structure):  # reference raytracer.h:113-119, 80 B
    _fields_ = [("t", C.c_double), ("u", C.c_double), ("v", C.c_double), ("point", Vec3), ("normal", Vec3),
                ("object_id", C.c_uint32)]


class RtHipMesh(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("color", C.c_double * 3), ("emission", C.c_double * 3),
                ("num_triangles", C.c_size_t), ("vertices", C.POINTER(Vertex))]


class RtHipSceneOptions(C.Structure):  # rt_hip.h: rt_hip_scene_create_opts' options (rt_hip_scene_options_defaults), 8 B
    _fields_ = [("struct_size", C.c_uint32), ("bvh_builder", C.c_uint32)]


BVH_HOST, BVH_DEVICE = 0, 1  # RtHipSceneOptions.bvh_builder / rt_hip_set_bvh_builder()
BVH_BUILDERS = {"host": BVH_HOST, "device": BVH_DEVICE}
BVH_SRC_DOUBLES = 16         # PT_BVH_SRC_DOUBLES: doubles per fp64 source node (rt_hip_scene_bvh_read)


class RtHipParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("max_depth", C.c_int32),
                ("seed", C.c_uint64), ("tile_first", C.c_uint32), ("tile_stride", C.c_uint32),
                ("tile_count", C.c_uint32), ("integrator", C.c_uint32)]


class RtHipAov(C.Structure):  # rt_hip.h: device (tiles) or host (image) pointers of the first-hit feature buffers; NULL: not wanted
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("object", C.c_void_p), ("hits", C.c_void_p)]


class RtAovImage(C.Structure):  # include/raytracer.h: render_aov's row-major host arrays
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("object_id", C.c_void_p),
                ("hits", C.c_void_p)]


class RtHipDenoiseParams(C.Structure):  # rt_hip.h: the denoiser's parameters (rt_hip_denoise_defaults)
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_uint32), ("normal_power_log2", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_depth", C.c_double)]


class RtHipReprojectParams(C.Structure):  # rt_hip.h: temporal reprojection (rt_hip_reproject_defaults), 32 B
    _fields_ = [("flags", C.c_uint32), ("max_history", C.c_double), ("depth_tol", C.c_double), ("normal_min", C.c_double)]


class RtHipUpsampleParams(C.Structure):  # rt_hip.h: guided upsampling (rt_hip_upsample_defaults), 16 B
    _fields_ = [("flags", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_depth", C.c_double)]


class RtHipAdaptParams(C.Structure):  # rt_hip.h: adaptive sampling (rt_hip_adapt_defaults)
    _fields_ = [("min_samples", C.c_int32), ("dilate", C.c_uint32), ("threshold", C.c_double)]


class RtHipQueryParams(C.Structure):  # rt_hip.h: a ray query (rt_hip_query_defaults), 24 B
    _fields_ = [("source", C.c_uint32), ("flags", C.c_uint32), ("camera", C.POINTER(Camera)), ("origin_radius", C.c_double)]


class RtHipHits(C.Structure):  # rt_hip.h: a query's structure-of-arrays outputs (device or host pointers; NULL: not wanted), 64 B
    _fields_ = [("status", C.c_void_p), ("t", C.c_void_p), ("object", C.c_void_p), ("prim", C.c_void_p), ("point", C.c_void_p),
                ("normal", C.c_void_p), ("bary", C.c_void_p), ("ray", C.c_void_p)]


RAYS_GIVEN, RAYS_CAMERA_UV = 0, 1   # RtHipQueryParams.source
RAYS_NORMALIZE = 1                  # RtHipQueryParams.flags
HIT_FIELDS = ("status", "t", "object", "prim", "point", "normal", "bary", "ray")   # RtHipHits order
HIT_SHAPES = {"status": ("uint32", 1), "t": ("float64", 1), "object": ("uint32", 1), "prim": ("uint32", 1), "point": ("float64", 3),
              "normal": ("float64", 3), "bary": ("float64", 2), "ray": ("float64", 6)}   # dtype, values per ray
NO_HIT = 0xFFFFFFFF                 # object / prim of a miss


class RtHipTraceParams(C.Structure):  # rt_hip.h: a radiance query (rt_hip_trace_defaults), 48 B
    _fields_ = [("source", C.c_uint32), ("flags", C.c_uint32), ("camera", C.POINTER(Camera)), ("origin_radius", C.c_double),
                ("samples", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint64), ("index_first", C.c_uint32),
                ("integrator", C.c_uint32)]


class RtHipRadiance(C.Structure):  # rt_hip.h: a radiance query's structure-of-arrays outputs (NULL: not wanted), 48 B
    _fields_ = [("status", C.c_void_p), ("radiance", C.c_void_p), ("samples", C.c_void_p), ("paths", C.c_void_p),
                ("casts", C.c_void_p), ("ray", C.c_void_p)]


RADIANCE_FIELDS = ("status", "radiance", "samples", "paths", "casts", "ray")   # RtHipRadiance order
RADIANCE_SHAPES = {"status": ("uint32", 1), "radiance": ("float64", 3), "samples": ("float64", 0), "paths": ("uint64", 1),
                   "casts": ("uint64", 1), "ray": ("float64", 6)}   # dtype, values per ray (samples: 3 per sample)

class RtHipLens(C.Structure):  # rt_hip.h: a thin lens (rt_hip_lens_defaults), 24 B
    _fields_ = [("aperture_radius", C.c_double), ("focus_distance", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


PROBE_SPHERE, PROBE_HEMISPHERE = 0, 1   # RtHipProbeParams.mode
PROBE_BASES = {PROBE_SPHERE: 9, PROBE_HEMISPHERE: 1}


class RtHipProbeParams(C.Structure):  # rt_hip.h: a light-probe bake (rt_hip_probe_defaults), 48 B
    _fields_ = [("mode", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint64),
                ("bias", C.c_double), ("origin_radius", C.c_double), ("reserved", C.c_uint64)]


GRID_FACING = 1   # RT_HIP_GRID_FACING


class RtHipProbeGrid(C.Structure):  # rt_hip.h: a regular grid of probes (rt_hip_probe_grid_defaults), 88 B
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("origin", C.c_double * 3), ("step", C.c_double * 3),
                ("count", C.c_uint32 * 3), ("miss_color", C.c_float * 3), ("reserved", C.c_uint32)]


class RtHipProbeVis(C.Structure):  # rt_hip.h: a grid's depth-moment visibility (rt_hip_probe_vis_defaults), 48 B
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("res", C.c_uint32), ("sharp", C.c_uint32), ("d_max", C.c_double),
                ("bias", C.c_double), ("floor", C.c_double), ("reserved", C.c_uint64)]


class RtHipProbeUpdate(C.Structure):  # rt_hip.h: an update round of a grid's state (rt_hip_probe_update_defaults), 48 B
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("stride", C.c_uint32), ("phase", C.c_uint32), ("round", C.c_uint32),
                ("reserved", C.c_uint32), ("hysteresis", C.c_double), ("change", C.c_double), ("fast", C.c_double)]


class RtHipPixelParams(C.Structure):  # rt_hip.h: a pixel refinement's trace (rt_hip_pixel_defaults), 32 B
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("sample_first", C.c_int32),
                ("max_depth", C.c_int32), ("integrator", C.c_uint32), ("seed", C.c_uint64)]


PIXEL_FIELDS = ("status", "radiance", "samples", "paths", "casts")   # what rt_hip_trace_pixels writes of an RtHipRadiance
SELECT_INVERT = 1                                                    # RT_HIP_SELECT_INVERT

ADAPT_CHECKPOINT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_uint32)  # on_checkpoint(user, samples done, live tiles)

DENOISE_DEMODULATE, DENOISE_OBJECT_EDGES = 1, 2   # RT_HIP_DENOISE_*
UPSAMPLE_DEMODULATE, UPSAMPLE_OBJECT_EDGES = 1, 2   # RT_HIP_UPSAMPLE_*

AOV_FIELDS = ("albedo", "normal", "depth", "object", "hits")   # RtHipAov order
AOV_CHANNELS = {"albedo": 3, "normal": 3, "depth": 1, "object": 1, "hits": 1}
AOV_DTYPES = {"albedo": "float32", "normal": "float32", "depth": "float32", "object": "uint32", "hits": "uint32"}   # numpy's names
ENODEV = -1                                                     # RT_HIP_ENODEV


TRACE_PATH, CAST_RAY = 0, 1  # RtHipParams.integrator / rt_set_integrator()
INTEGRATORS = {"path": TRACE_PATH, "whitted": CAST_RAY}


class RtSceneInfo(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("samples", C.c_int), ("max_depth", C.c_int),
                ("cam_pos", C.c_double * 3), ("cam_target", C.c_double * 3), ("n_objects", C.c_size_t),
                ("n_meshes", C.c_size_t), ("n_triangles", C.c_size_t)]


# every symbol include/rt_hip.h declares: name -> (restype, argtypes)
SHIM_SYMBOLS = {
    "rt_hip_device_count": (C.c_int, []),
    "rt_hip_last_error": (C.c_char_p, []),
    "rt_hip_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "rt_hip_scene_create": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "rt_hip_scene_destroy": (None, [C.c_void_p]),
    "rt_hip_scene_options_defaults": (None, [C.POINTER(RtHipSceneOptions)]),
    "rt_hip_scene_create_opts": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.c_int,
                                           C.POINTER(RtHipSceneOptions), C.POINTER(C.c_void_p)]),
    "rt_hip_scene_bvh_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "rt_hip_scene_bvh_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_scene_bvh_build_seconds": (C.c_double, [C.c_void_p]),
    "rt_hip_set_bvh_builder": (C.c_int, [C.c_int]),
    "rt_hip_scene_update_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_update_vertices_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_update_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "rt_hip_scene_read_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_scene_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double * 3), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint32)]),
    "rt_hip_scene_update_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_update_spheres_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_read_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_scene_sphere_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_double * 8), C.POINTER(C.c_double * 8)]),
    "rt_hip_scene_update_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_update_materials_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_hip_scene_read_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_scene_material_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32)]),
    "rt_hip_scene_memory": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_hip_set_material_updates": (None, [C.c_int]),
    "rt_hip_set_scene_updates": (None, [C.c_int]),
    "rt_hip_cache_updates": (C.c_uint64, []),
    "rt_hip_scene_bvh_cost": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rt_hip_bvh_cost_nodes_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "rt_hip_scene_rebuild_bvh": (C.c_int, [C.c_void_p]),
    "rt_hip_scene_rebuild_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rt_hip_scene_maintain_bvh": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "rt_hip_set_bvh_rebuild_ratio": (C.c_int, [C.c_double]),
    "rt_hip_cache_rebuilds": (C.c_uint64, []),
    "rt_hip_scene_device": (C.c_int, [C.c_void_p]),
    "rt_hip_scene_primitives": (C.c_size_t, [C.c_void_p]),
    "rt_hip_scene_hull_facets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_hip_kernel_name": (C.c_char_p, [C.c_void_p, C.c_uint32]),
    "rt_hip_render_tiles": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipParams), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_chunk_workspace_bytes": (C.c_size_t, [C.c_uint32]),
    "rt_hip_suggest_chunks": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_int32]),
    "rt_hip_suggest_chunks_depth": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32]),
    "rt_hip_scene_chunk_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32]),
    "rt_hip_render_tiles_chunked": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipParams), C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_selftest_math": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "rt_hip_selftest_xcc": (C.c_int, [C.c_uint32, C.c_void_p, C.c_int]),
    "rt_hip_selftest_intersect": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int]),
    "rt_hip_accum_create": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipParams), C.POINTER(C.c_void_p)]),
    "rt_hip_accum_add": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_hip_accum_add_host": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "rt_hip_accum_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_accum_read_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_accum_samples": (C.c_int32, [C.c_void_p]),
    "rt_hip_accum_kernel": (C.c_char_p, [C.c_void_p]),
    "rt_hip_accum_destroy": (None, [C.c_void_p]),
    "rt_hip_adapt_defaults": (None, [C.POINTER(RtHipAdaptParams)]),
    "rt_hip_adapt_schedule": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "rt_hip_tile_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p]),
    "rt_hip_accum_freeze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]),
    "rt_hip_accum_freeze_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "rt_hip_accum_tile_samples": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_hip_accum_live_tiles": (C.c_uint32, [C.c_void_p]),
    "rt_hip_accum_run_adaptive": (C.c_int, [C.c_void_p, C.POINTER(RtHipAdaptParams), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                            C.c_void_p, C.c_void_p]),
    "rt_hip_render_adaptive_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera),
                                               C.POINTER(RtHipParams), C.POINTER(RtHipAdaptParams), C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "rt_hip_untile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_set_cancel_flag": (None, [C.c_void_p]),
    "rt_hip_release_cache": (None, []),
    "rt_hip_cache_builds": (C.c_uint64, []),
    "rt_hip_set_device_map": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "rt_hip_last_image_phases": (None, [C.POINTER(C.c_double)]),
    "rt_hip_pool_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "rt_hip_last_launch_kernel": (C.c_char_p, []),
    "rt_hip_kernel_count": (C.c_int, []),
    "rt_hip_kernel_launches": (C.c_char_p, [C.c_int, C.POINTER(C.c_uint64)]),
    "rt_hip_kernel_for_class": (C.c_char_p, [C.c_void_p]),
    "rt_hip_launch_status": (C.c_int, [C.c_int, C.POINTER(C.c_uint32)]),
    "rt_hip_selftest_fail_alloc": (None, [C.c_uint32]),
    "rt_hip_mixed_grid_launches": (C.c_uint64, []),
    "rt_hip_selftest_pool_slots": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_hip_render_aov_tiles": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipParams), C.POINTER(RtHipAov), C.c_void_p]),
    "rt_hip_untile_aov": (C.c_int, [C.POINTER(RtHipAov), C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.POINTER(RtHipAov), C.c_void_p]),
    "rt_hip_render_aov_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera),
                                          C.POINTER(RtHipParams), C.c_int, C.POINTER(RtHipAov)]),
    "rt_hip_aov_kernel_name": (C.c_char_p, [C.c_void_p]),
    "rt_hip_aov_kernel_count": (C.c_int, []),
    "rt_hip_aov_kernel_launches": (C.c_char_p, [C.c_int, C.POINTER(C.c_uint64)]),
    "rt_hip_query_defaults": (None, [C.POINTER(RtHipQueryParams)]),
    "rt_hip_query_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RtHipQueryParams), C.POINTER(RtHipHits),
                                    C.c_void_p]),
    "rt_hip_query_rays_host": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.POINTER(RtHipQueryParams), C.c_int, C.POINTER(RtHipHits)]),
    "rt_hip_query_kernel_name": (C.c_char_p, [C.c_void_p]),
    "rt_hip_query_kernel_count": (C.c_int, []),
    "rt_hip_query_kernel_launches": (C.c_char_p, [C.c_int, C.POINTER(C.c_uint64)]),
    "rt_hip_trace_defaults": (None, [C.POINTER(RtHipTraceParams)]),
    "rt_hip_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RtHipTraceParams), C.POINTER(RtHipRadiance), C.c_void_p,
                                    C.c_void_p]),
    "rt_hip_trace_rays_host": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.c_void_p, C.c_uint64,
                                         C.POINTER(RtHipTraceParams), C.c_int, C.POINTER(RtHipRadiance), C.c_void_p]),
    "rt_hip_trace_kernel_name": (C.c_char_p, [C.c_void_p]),
    "rt_hip_trace_kernel_count": (C.c_int, []),
    "rt_hip_trace_kernel_launches": (C.c_char_p, [C.c_int, C.POINTER(C.c_uint64)]),
    "rt_hip_lens_defaults": (None, [C.POINTER(RtHipLens)]),
    "rt_hip_lens_rays": (C.c_int, [C.POINTER(Camera), C.POINTER(RtHipLens), C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_hip_lens_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_uint32]),
    "rt_hip_render_lens": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipLens), C.POINTER(RtHipParams), C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_lens_resolve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_render_lens_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera),
                                           C.POINTER(RtHipLens), C.POINTER(RtHipParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_defaults": (None, [C.POINTER(RtHipProbeParams)]),
    "rt_hip_probe_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RtHipProbeParams), C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_void_p]),
    "rt_hip_probe_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "rt_hip_bake_probes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RtHipProbeParams), C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_resolve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_irradiance": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rt_hip_bake_probes_host": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.POINTER(RtHipProbeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_grid_defaults": (None, [C.POINTER(RtHipProbeGrid)]),
    "rt_hip_probe_grid_positions": (C.c_int, [C.POINTER(RtHipProbeGrid), C.c_void_p, C.c_void_p]),
    "rt_hip_probe_grid_workspace_bytes": (C.c_size_t, [C.POINTER(RtHipProbeGrid), C.c_uint32]),
    "rt_hip_bake_probe_grid": (C.c_int, [C.c_void_p, C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeParams), C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_shade": (C.c_int, [C.POINTER(RtHipProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_preview_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_hip_probe_preview": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipProbeGrid), C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_preview_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera),
                                             C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeParams), C.c_int32, C.c_int32, C.c_int32, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_preview_scene_image": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeParams), C.c_int32,
                                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_vis_defaults": (None, [C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeGrid)]),
    "rt_hip_probe_depth_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "rt_hip_bake_probe_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeParams), C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_grid_depth_workspace_bytes": (C.c_size_t, [C.POINTER(RtHipProbeGrid), C.c_uint32, C.c_uint32]),
    "rt_hip_bake_probe_grid_depth": (C.c_int, [C.c_void_p, C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeParams),
                                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_shade_vis": (C.c_int, [C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_preview_vis": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rt_hip_probe_preview_vis_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera),
                                                 C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeParams), C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_preview_vis_scene_image": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis),
                                                       C.POINTER(RtHipProbeParams), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_update_defaults": (None, [C.POINTER(RtHipProbeUpdate)]),
    "rt_hip_probe_update_count": (C.c_uint64, [C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeUpdate)]),
    "rt_hip_probe_update_workspace_bytes": (C.c_size_t, [C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeUpdate),
                                                         C.c_uint32]),
    "rt_hip_probe_grid_update": (C.c_int, [C.c_void_p, C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeParams),
                                           C.POINTER(RtHipProbeUpdate), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_blend_coeff": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeUpdate), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_blend_moments": (C.c_int, [C.c_void_p, C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeUpdate),
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_age_step": (C.c_int, [C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeUpdate), C.c_void_p, C.c_void_p]),
    "rt_hip_probe_grid_update_host": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(RtHipProbeGrid),
                                                C.POINTER(RtHipProbeVis), C.POINTER(RtHipProbeParams), C.POINTER(RtHipProbeUpdate), C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_probe_update_preview_scene_image": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RtHipProbeGrid), C.POINTER(RtHipProbeVis),
                                                          C.POINTER(RtHipProbeParams), C.POINTER(RtHipProbeUpdate), C.c_int32, C.c_int32,
                                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_denoise_defaults": (None, [C.POINTER(RtHipDenoiseParams)]),
    "rt_hip_denoise_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rt_hip_denoise": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.c_int32, C.c_int32, C.POINTER(RtHipDenoiseParams), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_denoise_image": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.c_int32, C.c_int32, C.POINTER(RtHipDenoiseParams), C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "rt_hip_reproject_defaults": (None, [C.POINTER(RtHipReprojectParams)]),
    "rt_hip_reproject": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(RtHipAov),
                                   C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(RtHipReprojectParams), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_reproject_image": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(RtHipAov),
                                         C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(RtHipReprojectParams), C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_prev_points": (C.c_int, [C.POINTER(RtHipHits), C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rt_hip_prev_points_host": (C.c_int, [C.POINTER(RtHipHits), C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "rt_hip_prev_points_moved": (C.c_int, [C.POINTER(RtHipHits), C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p]),
    "rt_hip_prev_points_moved_host": (C.c_int, [C.POINTER(RtHipHits), C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_int, C.c_void_p]),
    # rt_hip_reproject's arguments with the previous points after params
    "rt_hip_reproject_points": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(RtHipAov),
                                          C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(RtHipReprojectParams), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_reproject_points_image": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.POINTER(Camera), C.c_void_p, C.c_void_p,
                                                C.POINTER(RtHipAov), C.POINTER(Camera), C.c_int32, C.c_int32,
                                                C.POINTER(RtHipReprojectParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "rt_hip_upsample_defaults": (None, [C.POINTER(RtHipUpsampleParams)]),
    "rt_hip_upsample": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.c_int32, C.c_int32, C.POINTER(RtHipAov), C.c_int32, C.c_int32,
                                  C.POINTER(RtHipUpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_upsample_image": (C.c_int, [C.c_void_p, C.POINTER(RtHipAov), C.c_int32, C.c_int32, C.POINTER(RtHipAov), C.c_int32, C.c_int32,
                                        C.POINTER(RtHipUpsampleParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_select_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rt_hip_select_pixels": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_hip_pixel_defaults": (None, [C.POINTER(RtHipPixelParams)]),
    "rt_hip_trace_pixels": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_uint64, C.POINTER(RtHipPixelParams),
                                      C.POINTER(RtHipRadiance), C.c_void_p, C.c_void_p]),
    "rt_hip_trace_pixels_host": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t, C.POINTER(Camera), C.c_void_p,
                                           C.c_uint64, C.POINTER(RtHipPixelParams), C.c_int, C.POINTER(RtHipRadiance), C.c_void_p]),
    "rt_hip_pixel_kernel_name": (C.c_char_p, [C.c_void_p]),
    "rt_hip_pixel_kernel_count": (C.c_int, []),
    "rt_hip_pixel_kernel_launches": (C.c_char_p, [C.c_int, C.POINTER(C.c_uint64)]),
    "rt_hip_blend_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hip_render_image": (C.c_int, [C.POINTER(Object), C.c_size_t, C.POINTER(RtHipMesh), C.c_size_t,
                                      C.POINTER(Camera), C.POINTER(RtHipParams), C.c_int, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
}

# every function include/raytracer.h declares (+ scenes.h), same idea
HOST_SYMBOLS = {
    "random_double": (C.c_double, []),
    "random_range": (C.c_double, [C.c_double, C.c_double]),
    "point_at": (Vec3, [C.POINTER(Ray), C.c_double]),
    "calculate_surface_normal": (Vec3, [Vec3, Vec3, Vec3]),
    "clamp": (Vec3, [Vec3]),
    "intersect_sphere": (C.c_bool, [C.POINTER(Ray), Vec3, C.c_double, C.POINTER(Hit)]),
    "intersect_triangle": (C.c_bool, [C.POINTER(Ray), Vertex, Vertex, Vertex, C.POINTER(Hit)]),
    "print_v": (None, [C.c_char_p, Vec3]),
    "print_m": (None, [C.POINTER(C.c_double)]),
    "init_camera": (None, [C.POINTER(Camera), Vec3, Vec3, C.POINTER(Options)]),
    "render": (None, [C.c_void_p, C.POINTER(Object), C.c_size_t, C.POINTER(Camera), C.POINTER(Options)]),
    "load_obj": (C.c_bool, [C.c_char_p, C.POINTER(TriangleMesh)]),
    "render_ex": (None, [C.c_void_p, C.c_void_p, C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                         C.POINTER(Camera), C.POINTER(Options)]),
    "rt_set_max_depth": (None, [C.c_int]),
    "rt_set_seed": (None, [C.c_uint64]),
    "rt_set_lens": (None, [C.c_double, C.c_double]),
    "rt_get_lens": (None, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rt_set_probe_grid": (None, [C.c_int, C.c_int, C.c_int]),
    "rt_get_probe_grid": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rt_set_probe_update": (None, [C.c_int, C.c_double]),
    "rt_get_probe_update": (None, [C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "rt_set_probe_visibility": (None, [C.c_int]),
    "rt_get_probe_visibility": (C.c_int, []),
    "rt_set_integrator": (None, [C.c_int]),
    "rt_get_integrator": (C.c_int, []),
    "rt_set_bvh_builder": (None, [C.c_int]),
    "rt_get_bvh_builder": (C.c_int, []),
    "rt_set_scene_updates": (None, [C.c_int]),
    "rt_get_scene_updates": (C.c_int, []),
    "rt_set_material_updates": (None, [C.c_int]),
    "rt_get_material_updates": (C.c_int, []),
    "rt_set_bvh_rebuild_ratio": (None, [C.c_double]),
    "rt_get_bvh_rebuild_ratio": (C.c_double, []),
    "rt_set_devices": (None, [C.c_int]),
    "rt_get_max_depth": (C.c_int, []),
    "rt_get_seed": (C.c_uint64, []),
    "rt_set_cancel_flag": (None, [C.c_void_p]),
    "render_progressive": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                                     C.POINTER(Camera), C.POINTER(Options), C.c_int, C.c_void_p, C.c_void_p]),
    "render_adaptive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                                  C.POINTER(Camera), C.POINTER(Options), C.POINTER(RtHipAdaptParams), C.c_void_p, C.c_void_p]),
    "rt_last_pixel_samples": (C.c_longlong, []),
    "render_aov": (C.c_int, [C.POINTER(RtAovImage), C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                             C.POINTER(Camera), C.POINTER(Options)]),
    "denoise_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtAovImage), C.c_int, C.c_int,
                                C.POINTER(RtHipDenoiseParams)]),
    "reproject_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtAovImage), C.POINTER(Camera),
                                  C.c_void_p, C.c_void_p, C.POINTER(RtAovImage), C.POINTER(Camera), C.c_int, C.c_int,
                                  C.POINTER(RtHipReprojectParams)]),
    "upsample_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtAovImage), C.c_int, C.c_int,
                                 C.POINTER(RtAovImage), C.c_int, C.c_int, C.POINTER(RtHipUpsampleParams)]),
    "intersect_rays": (C.c_int, [C.POINTER(Ray), C.c_size_t, C.c_void_p, C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                                 C.POINTER(Hit), C.c_void_p]),
    "trace_rays": (C.c_int, [C.POINTER(Ray), C.c_size_t, C.c_int, C.POINTER(Object), C.c_size_t, C.POINTER(MeshObject), C.c_size_t,
                             C.POINTER(Vec3), C.c_void_p]),
    "rt_last_render_cancelled": (C.c_int, []),
    "rt_last_render_seconds": (C.c_double, []),
    "rt_last_ray_bounces": (C.c_longlong, []),
    "rt_scene_info": (C.c_int, [C.c_int, C.POINTER(RtSceneInfo)]),
    "rt_scene_build": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(Object), C.POINTER(MeshObject)]),
    "rt_scene_free_meshes": (None, [C.POINTER(MeshObject), C.c_size_t]),
    "rt_mesh_flip_winding": (None, [C.POINTER(TriangleMesh)]),
    "stbi_write_png": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
}
HOST_DATA = ["ray_count", "intersection_test_count"]


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


_shim = None
_host = None


def load_shim():
    """librt_hip.so.  Raises if it is not built: there is no fallback path."""
    global _shim
    if _shim is None:
        # PyTorch-ROCm bundles its own libamdhip64.so.7 / librccl.so.1 / libhsa-runtime64.so.1.
        # The dynamic loader de-duplicates by SONAME only for libraries loaded EARLIER, so
        # torch must come first: the shim then binds to the very runtime instance torch uses
        # (one HIP runtime per process => torch streams and device pointers are valid in the
        # shim).  Loading the shim first would pull in /opt/rocm's copies next to torch's.
        import torch  # noqa: F401
        if not os.path.exists(SHIM_PATH):
            raise RuntimeError(f"{SHIM_PATH} is missing: build it with `make shim` "
                               "(or __graft_entry__.build()); this package has no CPU fallback")
        _shim = _bind(C.CDLL(SHIM_PATH, mode=C.RTLD_GLOBAL), SHIM_SYMBOLS)
    return _shim


def load_host():
    """libraytracer_amd.so: the reference API + scene builders."""
    global _host
    if _host is None:
        load_shim()
        if not os.path.exists(HOST_PATH):
            raise RuntimeError(f"{HOST_PATH} is missing: build it with `make host`")
        _host = _bind(C.CDLL(HOST_PATH), HOST_SYMBOLS)
    return _host


def denoise_params(iterations=None, sigma_color=None, sigma_depth=None, normal_power_log2=None, demodulate=None,
                   object_edges=None):
    """rt_hip_denoise_defaults() with the given fields replaced (None: the default)"""
    p = RtHipDenoiseParams()
    load_shim().rt_hip_denoise_defaults(C.byref(p))
    for f, v in (("iterations", iterations), ("sigma_color", sigma_color), ("sigma_depth", sigma_depth),
                 ("normal_power_log2", normal_power_log2)):
        if v is not None:
            setattr(p, f, v)
    for bit, v in ((DENOISE_DEMODULATE, demodulate), (DENOISE_OBJECT_EDGES, object_edges)):
        if v is not None:
            p.flags = (p.flags | bit) if v else (p.flags & ~bit)
    return p


def lens_params(aperture, focus):
    """an RtHipLens of the given aperture radius and focus distance"""
    lens = RtHipLens()
    load_shim().rt_hip_lens_defaults(C.byref(lens))
    lens.aperture_radius, lens.focus_distance = aperture, focus
    return lens


def probe_params(mode, samples, seed, max_depth=None, bias=0.0, origin_radius=0.0):
    """rt_hip_probe_defaults() with the given fields replaced (max_depth None: the default)"""
    p = RtHipProbeParams()
    load_shim().rt_hip_probe_defaults(C.byref(p))
    p.mode, p.samples, p.seed, p.bias, p.origin_radius = mode, samples, seed, bias, origin_radius
    if max_depth is not None:
        p.max_depth = max_depth
    return p


def probe_grid(origin, step, count, facing=False, miss_color=None):
    """rt_hip_probe_grid_defaults() with the given origin, step and count (three each) replaced; facing: RT_HIP_GRID_FACING;
    miss_color None: the default"""
    g = RtHipProbeGrid()
    load_shim().rt_hip_probe_grid_defaults(C.byref(g))
    for a in range(3):
        g.origin[a], g.step[a], g.count[a] = origin[a], step[a], count[a]
        if miss_color is not None:
            g.miss_color[a] = miss_color[a]
    g.flags = GRID_FACING if facing else 0
    return g


def probe_vis(grid, res=None, sharp=None, d_max=None, bias=None, floor=None):
    """rt_hip_probe_vis_defaults() for `grid` (abi.probe_grid(...), or None) with the given fields replaced (None: the default)"""
    v = RtHipProbeVis()
    load_shim().rt_hip_probe_vis_defaults(C.byref(v), None if grid is None else C.byref(grid))
    for f, x in (("res", res), ("sharp", sharp), ("d_max", d_max), ("bias", bias), ("floor", floor)):
        if x is not None:
            setattr(v, f, x)
    return v


def probe_update(stride=None, phase=None, round=None, hysteresis=None, change=None, fast=None):
    """rt_hip_probe_update_defaults() with the given fields replaced (None: the default)"""
    u = RtHipProbeUpdate()
    load_shim().rt_hip_probe_update_defaults(C.byref(u))
    for f, x in (("stride", stride), ("phase", phase), ("round", round), ("hysteresis", hysteresis), ("change", change), ("fast", fast)):
        if x is not None:
            setattr(u, f, x)
    return u


def reproject_params(max_history=None, depth_tol=None, normal_min=None):
    """rt_hip_reproject_defaults() with the given fields replaced (None: the default)"""
    p = RtHipReprojectParams()
    load_shim().rt_hip_reproject_defaults(C.byref(p))
    for f, v in (("max_history", max_history), ("depth_tol", depth_tol), ("normal_min", normal_min)):
        if v is not None:
            setattr(p, f, v)
    return p


def upsample_params(sigma_depth=None, normal_power_log2=None, demodulate=None, object_edges=None):
    """rt_hip_upsample_defaults() with the given fields replaced (None: the default)"""
    p = RtHipUpsampleParams()
    load_shim().rt_hip_upsample_defaults(C.byref(p))
    for f, v in (("sigma_depth", sigma_depth), ("normal_power_log2", normal_power_log2)):
        if v is not None:
            setattr(p, f, v)
    for bit, v in ((UPSAMPLE_DEMODULATE, demodulate), (UPSAMPLE_OBJECT_EDGES, object_edges)):
        if v is not None:
            p.flags = (p.flags | bit) if v else (p.flags & ~bit)
    return p


def query_params(source=RAYS_GIVEN, normalize=False, camera=None, origin_radius=None):
    """rt_hip_query_defaults() with the given fields replaced (origin_radius None: the default).  The camera is referenced, not
    copied: keep it alive until the call that takes the params has returned."""
    p = RtHipQueryParams()
    load_shim().rt_hip_query_defaults(C.byref(p))
    p.source = source
    p.flags = RAYS_NORMALIZE if normalize else 0
    if camera is not None:
        p.camera = C.pointer(camera)
    if origin_radius is not None:
        p.origin_radius = origin_radius
    return p


def trace_params(samples, seed, max_depth=None, source=RAYS_GIVEN, normalize=False, camera=None, origin_radius=None, index_first=0):
    """rt_hip_trace_defaults() with the given fields replaced (max_depth, origin_radius None: the defaults).  The camera is
    referenced, not copied: keep it alive until the call that takes the params has returned."""
    p = RtHipTraceParams()
    load_shim().rt_hip_trace_defaults(C.byref(p))
    p.source = source
    p.flags = RAYS_NORMALIZE if normalize else 0
    p.samples, p.seed, p.index_first = samples, seed, index_first
    if max_depth is not None:
        p.max_depth = max_depth
    if camera is not None:
        p.camera = C.pointer(camera)
    if origin_radius is not None:
        p.origin_radius = origin_radius
    return p


def pixel_params(width, height, samples, seed, sample_first=0, max_depth=None):
    """rt_hip_pixel_defaults() with the given fields replaced (max_depth None: the default)"""
    p = RtHipPixelParams()
    load_shim().rt_hip_pixel_defaults(C.byref(p))
    p.width, p.height, p.samples, p.sample_first, p.seed = width, height, samples, sample_first, seed
    if max_depth is not None:
        p.max_depth = max_depth
    return p


def adapt_params(min_samples=None, threshold=None, dilate=None):
    """rt_hip_adapt_defaults() with the given fields replaced (None: the default)"""
    p = RtHipAdaptParams()
    load_shim().rt_hip_adapt_defaults(C.byref(p))
    for f, v in (("min_samples", min_samples), ("threshold", threshold), ("dilate", dilate)):
        if v is not None:
            setattr(p, f, v)
    return p


def adapt_schedule(budget, min_samples):
    """rt_hip_adapt_schedule(): the sample counts the passes of an adaptive render end at (no device needed)"""
    buf = (C.c_int32 * 32)()
    n = load_shim().rt_hip_adapt_schedule(budget, min_samples, buf, 32)
    return [int(buf[k]) for k in range(n)]

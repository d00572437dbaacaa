"""The refusals of the ray front end, each form walked in its own order: the device forms and the host forms of the ray query, the
radiance query, the pixel refinement, the lens frame and the probe bake.  A case breaks one argument -- or two, where the point is
which refusal is reported first -- and asks for the code and the whole text of rt_hip_last_error().  None needs a device: the checks
come before the lookup, and what passes them ends at the lookup (logical device 99) or, in a device form, at an empty input.  The
texts and the workspace sizes below were recorded from the build before the sliced job and the shared prologue were folded."""
import ctypes as C

import numpy as np
import pytest

from rt_amd import abi, scene as S

OK, ENODEV, EINVAL = 0, abi.ENODEV, abi.EINVAL
FAKE = 0x1000            # an aligned address nothing dereferences: every call below returns before a launch
INF = float("inf")
NO_DEVICE = "no HIP device is available (this library has no CPU path)"
NO_DEVICE_99 = ("no HIP device 99", "logical device 99: the device map has ")   # where there are devices


class Env:
    def __init__(self):
        self.shim = abi.load_shim()
        self.sc = S.build_scene(1, 16, 16, 1)
        self.cam = self.sc.camera
        self.rays = np.zeros((4, 6))
        self.pixels = np.zeros(4, np.uint32)
        self.status = np.zeros(4, np.uint32)
        self.positions = np.zeros((4, 3))
        self.normals = np.tile([0.0, 0.0, 1.0], (4, 1))
        self.coeff = np.zeros((4, 9, 3))
        self.rgb = np.zeros((5 * 3, 3), np.float32)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.sc.free()


def _set(p, fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _ptr(v):
    return None if v is None else C.c_void_p(v)


def _hits(status):
    h = abi.RtHipHits()
    h.status = status
    return h


def _radiance(status, ray=None):
    r = abi.RtHipRadiance()
    r.status, r.ray = status, ray
    return r


def _frame(**fields):
    p = abi.RtHipParams()
    p.width, p.height, p.samples, p.max_depth, p.seed, p.tile_stride = 5, 3, 3, 4, 7, 1
    return _set(p, fields)


# ---- the forms: a valid call each, one keyword per argument a case may break ---------------------------------------------------------------
def query_device(e, scene=FAKE, rays=FAKE, n=4, params=True, out=FAKE, **fields):
    p = _set(abi.query_params(camera=e.cam), fields)
    return e.shim.rt_hip_query_rays(_ptr(scene), _ptr(rays), None, n, C.byref(p) if params else None, C.byref(_hits(out)), None)


def query_host(e, rays=True, n=4, params=True, out=True, **fields):
    p = _set(abi.query_params(camera=e.cam), fields)
    return e.shim.rt_hip_query_rays_host(e.sc.objects, e.sc.n_objects, None, 0, e.rays.ctypes.data if rays else None, None, n,
                                         C.byref(p) if params else None, 99, C.byref(_hits(e.status.ctypes.data if out else None)))


def trace_device(e, scene=FAKE, rays=FAKE, n=4, params=True, out=FAKE, **fields):
    p = _set(abi.trace_params(2, 7, camera=e.cam), fields)
    return e.shim.rt_hip_trace_rays(_ptr(scene), _ptr(rays), n, C.byref(p) if params else None, C.byref(_radiance(out)), None, None)


def trace_host(e, rays=True, n=4, params=True, out=True, **fields):
    p = _set(abi.trace_params(2, 7, camera=e.cam), fields)
    return e.shim.rt_hip_trace_rays_host(e.sc.objects, e.sc.n_objects, None, 0, e.rays.ctypes.data if rays else None, n,
                                         C.byref(p) if params else None, 99, C.byref(_radiance(e.status.ctypes.data if out else None)), None)


def pixels_device(e, scene=FAKE, camera=True, pixels=FAKE, n=4, params=True, out=FAKE, ray=None, **fields):
    p = _set(abi.pixel_params(8, 8, 2, 7), fields)
    return e.shim.rt_hip_trace_pixels(_ptr(scene), C.byref(e.cam) if camera else None, _ptr(pixels), n, C.byref(p) if params else None,
                                      C.byref(_radiance(out, ray)), None, None)


def pixels_host(e, camera=True, pixels=True, n=4, params=True, out=True, ray=None, **fields):
    p = _set(abi.pixel_params(8, 8, 2, 7), fields)
    return e.shim.rt_hip_trace_pixels_host(e.sc.objects, e.sc.n_objects, None, 0, C.byref(e.cam) if camera else None,
                                           e.pixels.ctypes.data if pixels else None, n, C.byref(p) if params else None, 99,
                                           C.byref(_radiance(e.status.ctypes.data if out else None, ray)), None)


def lens_device(e, scene=FAKE, camera=True, lens=True, params=True, slice_pixels=4, ws=FAKE, d_sum=FAKE, aperture=0.5, focus=2.0,
                lens_flags=0, lens_reserved=0, **fields):
    p, l = _frame(**fields), abi.lens_params(aperture, focus)
    l.flags, l.reserved = lens_flags, lens_reserved
    return e.shim.rt_hip_render_lens(_ptr(scene), C.byref(e.cam) if camera else None, C.byref(l) if lens else None,
                                     C.byref(p) if params else None, slice_pixels, _ptr(ws), _ptr(d_sum), None, None, None, None)


def lens_host(e, camera=True, lens=True, params=True, out=True, aperture=0.5, focus=2.0, lens_flags=0, lens_reserved=0, **fields):
    p, l = _frame(**fields), abi.lens_params(aperture, focus)
    l.flags, l.reserved = lens_flags, lens_reserved
    return e.shim.rt_hip_render_lens_image(e.sc.objects, e.sc.n_objects, None, 0, C.byref(e.cam) if camera else None,
                                           C.byref(l) if lens else None, C.byref(p) if params else None, 99,
                                           e.rgb.ctypes.data if out else None, None, None)


def bake_device(e, scene=FAKE, positions=FAKE, normals=None, n_probes=4, params=True, slice_rays=4, ws=FAKE, d_sum=None, coeff=FAKE,
                **fields):
    p = _set(abi.probe_params(abi.PROBE_SPHERE, 5, 7, 4), fields)
    return e.shim.rt_hip_bake_probes(_ptr(scene), _ptr(positions), _ptr(normals), n_probes, C.byref(p) if params else None, slice_rays,
                                     _ptr(ws), _ptr(d_sum), _ptr(coeff), None, None, None, None)


def bake_host(e, positions=True, normals=False, n_probes=4, params=True, out=True, **fields):
    p = _set(abi.probe_params(abi.PROBE_SPHERE, 5, 7, 4), fields)
    return e.shim.rt_hip_bake_probes_host(e.sc.objects, e.sc.n_objects, None, 0, e.positions.ctypes.data if positions else None,
                                          e.normals.ctypes.data if normals else None, n_probes, C.byref(p) if params else None, 99,
                                          e.coeff.ctypes.data if out else None, None, None, None)


# ---- the refusals, in each form's order: (what is broken, code, text) ----------------------------------------------------------------------
T_PARAMS = "params is required"
T_SAMPLES0 = "samples = 0 must be >= 1"
T_DEPTH = "max_depth out of range"
T_ORIGIN = "origin_radius -1 must be finite and >= 0"
T_N_QUERY = "n = 4294967296: a query takes fewer than 2^32 rays"
T_SOURCE = "source 2 is neither RT_HIP_RAYS_GIVEN nor RT_HIP_RAYS_CAMERA_UV"
T_CAMERA_UV = "RT_HIP_RAYS_CAMERA_UV needs params->camera"
T_HITS = "hits: at least one output array is required"
T_RADIANCE = "radiance: at least one output array is required"
T_INTEGRATOR = "integrator 1: %s traces paths (RT_HIP_TRACE_PATH) only"
T_N_TRACE = "n = %d, index_first = %d: a radiance query takes fewer than 2^32 rays with stream indices below 2^32"
T_PIXEL_SAMPLES = "samples = %d, sample_first = %d: samples >= 1, sample_first >= 0, sample_first + samples <= 2^31"
T_FRAME2 = "width and height must be in [2, 2^20] with fewer than 2^32 pixels"
T_TILES = "a lens frame is the whole frame: the tile fields must describe it or be 0"
T_WS16 = "d_workspace must be 16-byte aligned"
T_SUM8 = "d_sum must be 8-byte aligned"
T_MODE = "mode 2 is neither RT_HIP_PROBE_SPHERE nor RT_HIP_PROBE_HEMISPHERE"
T_PROBE_FLAGS = "probe flags and reserved must be 0"
NULL_CAMERA = C.POINTER(abi.Camera)()

RAYS_CASES = [   # check_rays: the tail of a ray query's and a radiance query's checks
    (dict(n=2 ** 32), EINVAL, T_N_QUERY),
    (dict(source=2), EINVAL, T_SOURCE),
    (dict(source=2, flags=2), EINVAL, T_SOURCE),
    (dict(flags=2), EINVAL, "unknown flags 0x2"),
    (dict(flags=2, origin_radius=-1.0), EINVAL, "unknown flags 0x2"),
    (dict(origin_radius=-1.0), EINVAL, T_ORIGIN),
    (dict(origin_radius=INF), EINVAL, "origin_radius inf must be finite and >= 0"),
    (dict(origin_radius=-1.0, source=abi.RAYS_CAMERA_UV, camera=NULL_CAMERA), EINVAL, T_ORIGIN),
    (dict(source=abi.RAYS_CAMERA_UV, camera=NULL_CAMERA), EINVAL, T_CAMERA_UV),
    (dict(source=abi.RAYS_CAMERA_UV, camera=NULL_CAMERA, rays=None), EINVAL, T_CAMERA_UV),
    (dict(rays=None), EINVAL, "rays is required"),
]
TRACE_HEAD = [   # check_trace up to check_rays
    (dict(params=False), EINVAL, T_PARAMS),
    (dict(out=None), EINVAL, T_RADIANCE),
    (dict(out=None, integrator=abi.CAST_RAY), EINVAL, T_RADIANCE),
    (dict(integrator=abi.CAST_RAY), EINVAL, T_INTEGRATOR % "a radiance query"),
    (dict(integrator=abi.CAST_RAY, samples=0), EINVAL, T_INTEGRATOR % "a radiance query"),
    (dict(samples=0), EINVAL, T_SAMPLES0),
    (dict(samples=0, max_depth=-1), EINVAL, T_SAMPLES0),
    (dict(max_depth=-1), EINVAL, T_DEPTH),
    (dict(max_depth=1000001), EINVAL, T_DEPTH),
    (dict(max_depth=-1, n=2 ** 32), EINVAL, T_DEPTH),
    (dict(n=2 ** 32), EINVAL, T_N_TRACE % (2 ** 32, 0)),
    (dict(index_first=2 ** 32 - 3), EINVAL, T_N_TRACE % (4, 2 ** 32 - 3)),
    (dict(index_first=2 ** 32 - 3, source=2), EINVAL, T_N_TRACE % (4, 2 ** 32 - 3)),
]
PIXEL_CASES = [  # check_pixels
    (dict(params=False), EINVAL, T_PARAMS),
    (dict(out=None), EINVAL, T_RADIANCE),
    (dict(out=None, ray=FAKE), EINVAL, T_RADIANCE),
    (dict(ray=FAKE), EINVAL, "radiance: ray must be NULL (an entry's samples have a camera ray each)"),
    (dict(ray=FAKE, integrator=abi.CAST_RAY), EINVAL, "radiance: ray must be NULL (an entry's samples have a camera ray each)"),
    (dict(integrator=abi.CAST_RAY), EINVAL, T_INTEGRATOR % "a pixel refinement"),
    (dict(integrator=abi.CAST_RAY, samples=0), EINVAL, T_INTEGRATOR % "a pixel refinement"),
    (dict(samples=0), EINVAL, T_PIXEL_SAMPLES % (0, 0)),
    (dict(sample_first=-1), EINVAL, T_PIXEL_SAMPLES % (2, -1)),
    (dict(samples=2 ** 30, sample_first=2 ** 30 + 1), EINVAL, T_PIXEL_SAMPLES % (2 ** 30, 2 ** 30 + 1)),
    (dict(samples=0, max_depth=-1), EINVAL, T_PIXEL_SAMPLES % (0, 0)),
    (dict(max_depth=-1), EINVAL, T_DEPTH),
    (dict(max_depth=1000001, width=1), EINVAL, T_DEPTH),
    (dict(width=1), EINVAL, T_FRAME2),
    (dict(height=2 ** 20 + 1, n=2 ** 32), EINVAL, T_FRAME2),
    (dict(n=2 ** 32), EINVAL, "n = 4294967296: a call takes fewer than 2^32 entries"),
    (dict(n=2 ** 32, camera=False), EINVAL, "n = 4294967296: a call takes fewer than 2^32 entries"),
    (dict(camera=False), EINVAL, "camera is required"),
    (dict(camera=False, pixels=None), EINVAL, "camera is required"),
    (dict(pixels=None), EINVAL, "pixels is required"),
]
LENS_CASES = [   # check_render_lens (check_lens inside it)
    (dict(params=False), EINVAL, T_PARAMS),
    (dict(params=False, camera=False), EINVAL, T_PARAMS),
    (dict(camera=False), EINVAL, "camera and lens are required"),
    (dict(lens=False), EINVAL, "camera and lens are required"),
    (dict(lens=False, width=1), EINVAL, "camera and lens are required"),
    (dict(aperture=-1.0), EINVAL, "aperture_radius -1 must be finite and >= 0"),
    (dict(aperture=INF, focus=0.0), EINVAL, "aperture_radius inf must be finite and >= 0"),
    (dict(focus=0.0), EINVAL, "focus_distance 0 must be finite and > 0"),
    (dict(focus=INF, lens_flags=1), EINVAL, "focus_distance inf must be finite and > 0"),
    (dict(lens_flags=1), EINVAL, "lens flags and reserved must be 0"),
    (dict(lens_reserved=1, width=1), EINVAL, "lens flags and reserved must be 0"),
    (dict(width=1), EINVAL, T_FRAME2),
    (dict(height=2 ** 20 + 1, integrator=abi.CAST_RAY), EINVAL, T_FRAME2),
    (dict(integrator=abi.CAST_RAY), EINVAL, T_INTEGRATOR % "a lens frame"),
    (dict(integrator=abi.CAST_RAY, samples=0), EINVAL, T_INTEGRATOR % "a lens frame"),
    (dict(samples=0), EINVAL, T_SAMPLES0),
    (dict(samples=0, max_depth=-1), EINVAL, T_SAMPLES0),
    (dict(max_depth=-1), EINVAL, T_DEPTH),
    (dict(max_depth=1000001, tile_first=1), EINVAL, T_DEPTH),
    (dict(width=2 ** 16, height=2 ** 15, samples=3), EINVAL,
     "samples x pixels = 3 x 2147483648 exceeds 2^32: a lens sample is a ray index of rt_hip_trace_rays"),
    (dict(tile_first=1), EINVAL, T_TILES),
    (dict(tile_stride=2), EINVAL, T_TILES),
    (dict(tile_count=3), EINVAL, T_TILES),
]
PROBE_CASES = [  # check_probe
    (dict(params=False), EINVAL, T_PARAMS),
    (dict(mode=2), EINVAL, T_MODE),
    (dict(mode=2, flags=1), EINVAL, T_MODE),
    (dict(flags=1), EINVAL, T_PROBE_FLAGS),
    (dict(reserved=1, samples=0), EINVAL, T_PROBE_FLAGS),
    (dict(samples=0), EINVAL, T_SAMPLES0),
    (dict(samples=0, bias=-1.0), EINVAL, T_SAMPLES0),
    (dict(samples=0, max_depth=-1), EINVAL, T_SAMPLES0),
    (dict(n_probes=2 ** 16 + 1, samples=2 ** 16), EINVAL,
     "probes x samples = 65537 x 65536 exceeds 2^32: a probe sample is a ray index of rt_hip_trace_rays"),
    (dict(n_probes=2 ** 32 + 1, samples=1, bias=-1.0), EINVAL,
     "probes x samples = 4294967297 x 1 exceeds 2^32: a probe sample is a ray index of rt_hip_trace_rays"),
    (dict(bias=-1.0), EINVAL, "bias -1 must be finite and >= 0"),
    (dict(bias=INF, origin_radius=-1.0), EINVAL, "bias inf must be finite and >= 0"),
    (dict(bias=-1.0, max_depth=-1), EINVAL, "bias -1 must be finite and >= 0"),
    (dict(origin_radius=-1.0), EINVAL, T_ORIGIN),
    (dict(origin_radius=INF, max_depth=-1), EINVAL, "origin_radius inf must be finite and >= 0"),
    (dict(max_depth=-1), EINVAL, T_DEPTH),
    (dict(max_depth=1000001, mode=abi.PROBE_HEMISPHERE), EINVAL, T_DEPTH),
    (dict(mode=abi.PROBE_HEMISPHERE), EINVAL, "RT_HIP_PROBE_HEMISPHERE needs normals"),
]

FORMS = {
    "query_rays": (query_device, [
        (dict(scene=None), EINVAL, "scene is required"),
        (dict(scene=None, params=False), EINVAL, "scene is required"),
        (dict(params=False), EINVAL, T_PARAMS),
        (dict(params=False, out=None), EINVAL, T_PARAMS),
        (dict(out=None), EINVAL, T_HITS),
        (dict(out=None, n=2 ** 32), EINVAL, T_HITS),
        *RAYS_CASES,
        (dict(rays=None, n=0), OK, None),
        (dict(rays=FAKE + 8), EINVAL, "d_rays must be 16-byte aligned"),
        (dict(rays=FAKE + 8, n=0), EINVAL, "d_rays must be 16-byte aligned"),
        (dict(n=0), OK, None),
    ]),
    "query_rays_host": (query_host, [
        (dict(params=False), EINVAL, T_PARAMS),
        (dict(params=False, out=False), EINVAL, T_PARAMS),
        (dict(out=False), EINVAL, T_HITS),
        (dict(out=False, n=2 ** 32), EINVAL, T_HITS),
        *RAYS_CASES,
        (dict(n=0, rays=None), ENODEV, None),     # the device is looked up before an empty query returns
        (dict(), ENODEV, None),
    ]),
    "trace_rays": (trace_device, [
        *TRACE_HEAD,
        *RAYS_CASES[1:],
        (dict(rays=FAKE + 8), EINVAL, "d_rays must be 16-byte aligned"),
        (dict(rays=FAKE + 8, scene=None), EINVAL, "d_rays must be 16-byte aligned"),
        (dict(scene=None), EINVAL, "scene is required"),
        (dict(scene=None, n=0), EINVAL, "scene is required"),
        (dict(n=0, rays=None), OK, None),
    ]),
    "trace_rays_host": (trace_host, [
        *TRACE_HEAD,
        *RAYS_CASES[1:],
        (dict(n=0, rays=None), OK, None),         # no ray: nothing to do, on any device or none
        (dict(n=0, samples=0), EINVAL, T_SAMPLES0),
        (dict(), ENODEV, None),
    ]),
    "trace_pixels": (pixels_device, [
        *PIXEL_CASES,
        (dict(pixels=None, scene=None), EINVAL, "pixels is required"),
        (dict(scene=None), EINVAL, "scene is required"),
        (dict(scene=None, n=0), EINVAL, "scene is required"),
        (dict(n=0, pixels=None), OK, None),
    ]),
    "trace_pixels_host": (pixels_host, [
        *PIXEL_CASES,
        (dict(n=0, pixels=None), OK, None),
        (dict(n=0, width=1), EINVAL, T_FRAME2),
        (dict(), ENODEV, None),
    ]),
    "render_lens": (lens_device, [
        *LENS_CASES[:13],
        (dict(d_sum=None), EINVAL, "at least one of sum, rgb and rgb8 is required"),
        (dict(d_sum=None, integrator=abi.CAST_RAY), EINVAL, "at least one of sum, rgb and rgb8 is required"),
        *LENS_CASES[13:20],
        (dict(slice_pixels=0), EINVAL, "slice_pixels must be >= 1"),
        (dict(slice_pixels=0, tile_first=1), EINVAL, "slice_pixels must be >= 1"),
        *LENS_CASES[20:],
        (dict(tile_count=3, scene=None), EINVAL, T_TILES),
        (dict(scene=None), EINVAL, "scene and d_workspace are required"),
        (dict(ws=None), EINVAL, "scene and d_workspace are required"),
        (dict(scene=None, ws=FAKE + 8), EINVAL, "scene and d_workspace are required"),
        (dict(ws=FAKE + 8), EINVAL, T_WS16),
        (dict(ws=FAKE + 8, d_sum=FAKE + 4), EINVAL, T_WS16),
        (dict(d_sum=FAKE + 4), EINVAL, T_SUM8),
    ]),
    "render_lens_image": (lens_host, [
        *LENS_CASES[:13],
        (dict(out=False), EINVAL, "at least one of sum, rgb and rgb8 is required"),
        (dict(out=False, integrator=abi.CAST_RAY), EINVAL, "at least one of sum, rgb and rgb8 is required"),
        *LENS_CASES[13:],
        (dict(), ENODEV, None),
    ]),
    "bake_probes": (bake_device, [
        *PROBE_CASES,
        (dict(mode=abi.PROBE_HEMISPHERE, slice_rays=0), EINVAL, "RT_HIP_PROBE_HEMISPHERE needs normals"),
        (dict(slice_rays=0), EINVAL, "slice_rays must be >= 1"),
        (dict(slice_rays=0, ws=FAKE + 8), EINVAL, "slice_rays must be >= 1"),
        (dict(ws=FAKE + 8), EINVAL, T_WS16),
        (dict(ws=FAKE + 8, d_sum=FAKE + 4), EINVAL, T_WS16),
        (dict(d_sum=FAKE + 4), EINVAL, T_SUM8),
        (dict(d_sum=FAKE + 4, n_probes=0), EINVAL, T_SUM8),            # the alignment is asked for before an empty bake returns
        (dict(ws=FAKE + 8, scene=None), EINVAL, T_WS16),               # ... and before the null checks
        (dict(n_probes=0, scene=None, ws=None, coeff=None, positions=None), OK, None),
        (dict(n_probes=0, mode=abi.PROBE_HEMISPHERE), OK, None),       # (no probe needs no normal)
        (dict(scene=None), EINVAL, "scene, d_positions, d_workspace and d_coeff are required"),
        (dict(positions=None), EINVAL, "scene, d_positions, d_workspace and d_coeff are required"),
        (dict(ws=None), EINVAL, "scene, d_positions, d_workspace and d_coeff are required"),
        (dict(coeff=None), EINVAL, "scene, d_positions, d_workspace and d_coeff are required"),
    ]),
    "bake_probes_host": (bake_host, [
        *PROBE_CASES,
        (dict(n_probes=0, positions=False, out=False), OK, None),      # no probe: nothing to do, on any device or none
        (dict(n_probes=0, samples=0), EINVAL, T_SAMPLES0),
        (dict(positions=False), EINVAL, "h_positions and h_coeff are required"),
        (dict(out=False), EINVAL, "h_positions and h_coeff are required"),
        (dict(mode=abi.PROBE_HEMISPHERE, normals=True, positions=False), EINVAL, "h_positions and h_coeff are required"),
        (dict(mode=abi.PROBE_HEMISPHERE, normals=True, bias=0.5), ENODEV, None),
        (dict(), ENODEV, None),
    ]),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_refusals_in_order(env, form):
    call, cases = FORMS[form]
    for broken, code, text in cases:
        got = call(env, **broken)
        said = env.shim.rt_hip_last_error().decode()
        assert got == code, (form, broken, got, said)
        if code == EINVAL:
            assert said == text, (form, broken)
        elif code == ENODEV and env.shim.rt_hip_device_count() == 0:
            assert said == NO_DEVICE, (form, broken)
        elif code == ENODEV:
            assert said.startswith(NO_DEVICE_99), (form, broken)
    print(f"{form}: {len(cases)} cases")


# ---- the workspace sizes ---------------------------------------------------------------------------------------------------------------------
def _align(n):
    return (n + 255) // 256 * 256


LENS_WORKSPACE = {   # (width, height, slice_pixels) -> bytes
    (2, 2, 1): 1024, (2, 2, 7): 1024, (2, 2, 4): 1024, (2, 2, 5): 1024,
    (5, 3, 1): 1280, (5, 3, 7): 1536, (5, 3, 15): 2048, (5, 3, 16): 2048,
    (64, 64, 1): 99072, (64, 64, 7): 99328, (64, 64, 4096): 409600, (64, 64, 4097): 409600,
}
PROBE_WORKSPACE = {  # (n_probes, mode, slice_rays) -> bytes
    (0, 0, 1): 768, (0, 0, 7): 1024, (0, 0, 4): 768, (0, 0, 5): 768, (0, 0, 15): 1536, (0, 0, 16): 1536, (0, 0, 4096): 311296, (0, 0, 4097): 312064,
    (0, 1, 1): 768, (0, 1, 7): 1024, (0, 1, 4): 768, (0, 1, 5): 768, (0, 1, 15): 1536, (0, 1, 16): 1536, (0, 1, 4096): 311296, (0, 1, 4097): 312064,
    (1, 0, 1): 1024, (1, 0, 7): 1280, (1, 0, 4): 1024, (1, 0, 5): 1024, (1, 0, 15): 1792, (1, 0, 16): 1792, (1, 0, 4096): 311552, (1, 0, 4097): 312320,
    (1, 1, 1): 1024, (1, 1, 7): 1280, (1, 1, 4): 1024, (1, 1, 5): 1024, (1, 1, 15): 1792, (1, 1, 16): 1792, (1, 1, 4096): 311552, (1, 1, 4097): 312320,
    (5, 0, 1): 2048, (5, 0, 7): 2304, (5, 0, 4): 2048, (5, 0, 5): 2048, (5, 0, 15): 2816, (5, 0, 16): 2816, (5, 0, 4096): 312576, (5, 0, 4097): 313344,
    (5, 1, 1): 1024, (5, 1, 7): 1280, (5, 1, 4): 1024, (5, 1, 5): 1024, (5, 1, 15): 1792, (5, 1, 16): 1792, (5, 1, 4096): 311552, (5, 1, 4097): 312320,
}


def test_workspace_bytes_are_the_recorded_ones(env):
    shim = env.shim
    assert len(LENS_WORKSPACE) == 3 * 4 and len(PROBE_WORKSPACE) == 3 * 2 * 8
    for (w, h, s), want in LENS_WORKSPACE.items():
        assert shim.rt_hip_lens_workspace_bytes(w, h, s) == want, (w, h, s)
        m = min(s, w * h)      # the lens query clamps the slice to the frame
        assert want == _align(48 * m) + _align(4 * m) + _align(24 * m) + _align(24 * w * h), (w, h, s)
    for (n, mode, s), want in PROBE_WORKSPACE.items():
        assert shim.rt_hip_probe_workspace_bytes(n, mode, s) == want, (n, mode, s)
        assert want == _align(48 * s) + _align(4 * s) + _align(24 * s) + _align(24 * abi.PROBE_BASES[mode] * n), (n, mode, s)   # no clamp
    # the 0 answers
    for w, h, s in ((1, 4, 4), (4, 1, 4), (2 ** 20 + 1, 2, 4), (2 ** 16, 2 ** 16, 4), (0, 0, 1), (5, 3, 0)):
        assert shim.rt_hip_lens_workspace_bytes(w, h, s) == 0, (w, h, s)
    for n, mode, s in ((5, 2, 4), (5, 0, 0), (5, 1, 0), (2 ** 32 + 1, 0, 4), (0, 0, 0)):
        assert shim.rt_hip_probe_workspace_bytes(n, mode, s) == 0, (n, mode, s)
    assert shim.rt_hip_probe_workspace_bytes(2 ** 32, 1, 1) == 3 * 256 + 24 * 2 ** 32

"""The host-array entry points (rt_hip_denoise_image, _reproject_image, _upsample_image, _render_aov_image, _query_rays_host,
_trace_rays_host, _trace_pixels_host) stage their arrays in one device allocation.  Here each of them is called with every output,
with each optional output left out and -- the ray forms and the AOV image -- with each output alone, at sizes whose parts are no
multiple of the 256-byte alignment (9 x 7 and 5 x 3 pixels; 1 and 65 rays of 3 samples), and its answer is compared BIT FOR BIT
with the device-pointer form of the same call.  A part staged at a wrong offset, with a wrong size or not at all shows as a
difference or as a sentinel that went missing.  Counters given in non-zero come back increased, never overwritten."""
import ctypes as C

import numpy as np
import pytest

import query_expected as Q
import reproject_expected as RE
import upsample_expected as UE
import util

pytestmark = pytest.mark.gpu

SEED = 1666943821
W, H, WL, HL = 9, 7, 5, 3
COUNTS = (1, 65)
SPP = 3
STATS0 = (5, 1 << 40, 7, 11)   # what h_stats holds before a call


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


@pytest.fixture(autouse=True)
def _no_device_failure(gpu):
    yield
    flags = C.c_uint32(7)
    assert gpu.abi.load_shim().rt_hip_launch_status(0, C.byref(flags)) == 0 and flags.value == 0


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.nbytes == exp.nbytes and got.tobytes() == exp.tobytes(), f"{what}: the host form differs from the device form"


def _aov_struct(abi, aov, fields, keep):
    """an RtHipAov of host pointers to the `fields` of `aov`"""
    a = abi.RtHipAov()
    for f in fields:
        arr = np.ascontiguousarray(aov[f], dtype=np.float32 if f in ("albedo", "normal", "depth") else np.uint32)
        keep.append(arr)
        setattr(a, f, arr.ctypes.data)
    return a


def _aov_fields(demodulate, object_edges):
    return ("normal", "depth", "hits") + (("albedo",) if demodulate else ()) + (("object",) if object_edges else ())


def _outputs(shapes, drop):
    """sentinel-filled host arrays for every output but `drop`, and the pointer of each (None for the dropped one)"""
    out = {f: np.full(shape, 7, dtype) for f, (shape, dtype) in shapes.items() if f != drop}
    return out, {f: (out[f].ctypes.data if f in out else None) for f in shapes}


# ---- the image forms -----------------------------------------------------------------------------------------------------------
def _denoise_inputs():
    rng = np.random.default_rng(97)
    rgb = (rng.random((H, W, 3)) * rng.choice([0.1, 1.0, 30.0], (H, W, 1))).astype(np.float32)
    hits = rng.integers(0, 4, (H, W)).astype(np.uint32)
    obj = rng.integers(0, 3, (H, W)).astype(np.uint32)
    obj[hits == 0] = 0xFFFFFFFF
    return rgb, dict(albedo=rng.random((H, W, 3)).astype(np.float32), normal=(rng.random((H, W, 3)) * 2 - 1).astype(np.float32),
                     depth=(rng.random((H, W)) * 20).astype(np.float32), hits=hits, object=obj)


@pytest.mark.parametrize("demodulate,object_edges", [(False, False), (True, False), (False, True), (True, True)])
def test_denoise_image(gpu, demodulate, object_edges):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    rgb, aov = _denoise_inputs()
    fields = _aov_fields(demodulate, object_edges)
    kw = dict(demodulate=demodulate, object_edges=object_edges, iterations=3)
    exp, exp8 = gpu.denoise(_dev(rgb), {f: _dev(aov[f]) for f in fields}, W, H, **kw)
    exp, exp8 = _np(exp), _np(exp8)
    assert np.isfinite(exp).all() and (exp != rgb).any()
    p = abi.denoise_params(**kw)
    for drop in (None, "rgb8", "rgb"):   # both outputs, floats alone, bytes alone
        keep = []
        out, ptr = _outputs(dict(rgb=((H, W, 3), np.float32), rgb8=((H, W, 3), np.uint8)), drop)
        before = rgb.copy()
        assert shim.rt_hip_denoise_image(rgb.ctypes.data, C.byref(_aov_struct(abi, aov, fields, keep)), W, H, C.byref(p), 0, ptr["rgb"],
                                         ptr["rgb8"]) == 0, shim.rt_hip_last_error()
        _same(rgb, before, "the input colour")
        for f, e in (("rgb", exp), ("rgb8", exp8)):
            if f in out:
                _same(out[f], e, f"denoise {fields} without {drop}: {f}")


@pytest.mark.parametrize("with_history", [False, True])
def test_reproject_image(gpu, with_history):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    rgb, aov, cam, hist, _ = RE.edge_case(W, H, "small", seed=97)
    if not with_history:
        hist = None
    p = RE.params(0)
    cam_c = RE.to_camera(RE.cam_array(cam))
    d_hist = None
    if hist is not None:
        d_hist = dict(rgb=_dev(hist["rgb"]), len=_dev(hist["len"]), aov={f: _dev(hist["aov"][f]) for f in gpu.REPROJECT_AOV},
                      camera=RE.to_camera(RE.cam_array(hist["camera"])))
    exp = gpu.reproject(_dev(rgb), {f: _dev(aov[f]) for f in gpu.REPROJECT_AOV}, cam_c, hist=d_hist, **p)
    exp = {f: _np(t) for f, t in exp.items()}
    if hist is not None:
        assert (exp["len"] > 1).any()   # the history is used: a history part staged wrongly would show
    pp = abi.reproject_params(**p)
    shapes = dict(rgb=((H, W, 3), np.float32), rgb8=((H, W, 3), np.uint8), len=((H, W), np.float32), motion=((H, W, 2), np.float32))
    for drop in (None, "rgb8", "motion"):
        keep = []
        out, ptr = _outputs(shapes, drop)
        h_rgb = h_len = h_aov = h_cam = None
        if hist is not None:
            hr, hl = np.ascontiguousarray(hist["rgb"], np.float32), np.ascontiguousarray(hist["len"], np.float32)
            keep += [hr, hl]
            h_rgb, h_len = hr.ctypes.data, hl.ctypes.data
            h_aov, h_cam = C.byref(_aov_struct(abi, hist["aov"], gpu.REPROJECT_AOV, keep)), C.byref(d_hist["camera"])
        src = np.ascontiguousarray(rgb, np.float32)
        assert shim.rt_hip_reproject_image(src.ctypes.data, C.byref(_aov_struct(abi, aov, gpu.REPROJECT_AOV, keep)), C.byref(cam_c), h_rgb,
                                           h_len, h_aov, h_cam, W, H, C.byref(pp), 0, ptr["rgb"], ptr["rgb8"], ptr["len"],
                                           ptr["motion"]) == 0, shim.rt_hip_last_error()
        for f in out:
            _same(out[f], exp[f], f"reproject history {with_history} without {drop}: {f}")


@pytest.mark.parametrize("demodulate,object_edges", [(False, False), (True, False), (False, True), (True, True)])
def test_upsample_image(gpu, demodulate, object_edges):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    low_rgb, low_aov, aov, _ = UE.edge_case(((W, H), (WL, HL)), 97)
    fields = _aov_fields(demodulate, object_edges)
    kw = dict(demodulate=demodulate, object_edges=object_edges)
    exp = gpu.upsample(_dev(low_rgb), {f: _dev(low_aov[f]) for f in fields}, WL, HL, {f: _dev(aov[f]) for f in fields}, W, H, **kw)
    exp = {f: _np(t) for f, t in exp.items()}
    assert (exp["conf"] > 0).any()      # guided pixels: the low frame's parts are read
    p = abi.upsample_params(**kw)
    shapes = dict(rgb=((H, W, 3), np.float32), rgb8=((H, W, 3), np.uint8), conf=((H, W), np.float32))
    for drop in (None, "rgb8", "conf"):
        keep = []
        out, ptr = _outputs(shapes, drop)
        src = np.ascontiguousarray(low_rgb, np.float32)
        assert shim.rt_hip_upsample_image(src.ctypes.data, C.byref(_aov_struct(abi, low_aov, fields, keep)), WL, HL,
                                          C.byref(_aov_struct(abi, aov, fields, keep)), W, H, C.byref(p), 0, ptr["rgb"], ptr["rgb8"],
                                          ptr["conf"]) == 0, shim.rt_hip_last_error()
        for f in out:
            _same(out[f], exp[f], f"upsample {fields} without {drop}: {f}")


def test_aov_image(gpu):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    sc = util.class_scene(n_packed=4, tris=40, width=W, height=H)
    gs = gpu.GpuScene(sc)
    exp = gs.aov_image(SEED, SPP)
    assert (exp["hits"] != 0).any()
    p = abi.RtHipParams()
    p.width, p.height, p.samples, p.seed = W, H, SPP, SEED
    meshes = sc.hip_meshes()
    for want in (abi.AOV_FIELDS,) + tuple((f,) for f in abi.AOV_FIELDS):
        out, a = {}, abi.RtHipAov()
        for f in want:
            out[f] = np.full((H, W, 3) if abi.AOV_CHANNELS[f] == 3 else (H, W), 7, np.float32 if f in ("albedo", "normal", "depth") else np.uint32)
            setattr(a, f, out[f].ctypes.data)
        assert shim.rt_hip_render_aov_image(sc.objects, sc.n_objects, meshes, sc.n_meshes, C.byref(sc.camera), C.byref(p), 0,
                                            C.byref(a)) == 0, shim.rt_hip_last_error()
        for f in want:
            _same(out[f], exp[f], f"AOV image, want {want}: {f}")
    gs.close()
    sc.free()


# ---- the ray forms -------------------------------------------------------------------------------------------------------------
SCENES = {"spheres": lambda: util.class_scene(n_packed=4), "mesh": lambda: util.class_scene(n_packed=4, tris=40)}


def _host_words(t):
    a = _np(t)
    return a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_query_rays_host(gpu, name):
    sc = SCENES[name]()
    gs = gpu.GpuScene(sc)
    rays = Q.ray_set(sc, n=max(COUNTS))
    for n in COUNTS:
        for limited in (False, True):
            t_max = np.linspace(0.5, 40.0, n) if limited else None
            exp = {f: _host_words(t) for f, t in gs.query_rays(rays[:n], t_max=t_max).items()}
            if n > 1:
                assert (exp["status"] == 1).any() and (not limited or (exp["status"] == 0).any())
            for want in (gpu.abi.HIT_FIELDS,) + tuple((f,) for f in gpu.abi.HIT_FIELDS):
                got = gpu.query_rays_host(sc, rays[:n], t_max=t_max, want=want)
                for f in want:
                    _same(got[f], exp[f], f"query {name} n={n} t_max {limited}, want {want}: {f}")
    assert gs.launch_status() == 0
    gs.close()
    sc.free()


def _radiance(abi, n, want):
    out, rad = {}, abi.RtHipRadiance()
    for f in want:
        dtype, k = abi.RADIANCE_SHAPES[f]
        out[f] = np.full((n, SPP, 3) if f == "samples" else ((n, k) if k > 1 else (n,)), 7, dtype=dtype)
        setattr(rad, f, out[f].ctypes.data)
    return out, rad


def _counted(exp_stats, stats):
    """h_stats came back as what it held plus the call's counts (the device form's, counted from zero)"""
    assert [int(s) for s in stats] == [a + int(b) for a, b in zip(STATS0, exp_stats)], (list(stats), exp_stats)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_trace_rays_host(gpu, name):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    sc = SCENES[name]()
    gs = gpu.GpuScene(sc)
    rays = np.ascontiguousarray(Q.ray_set(sc, n=max(COUNTS)))
    meshes = sc.hip_meshes()
    p = abi.trace_params(SPP, SEED, sc.max_depth)
    for n in COUNTS:
        exp = {f: _host_words(t) for f, t in gs.trace_rays(rays[:n], SPP, SEED, want=abi.RADIANCE_FIELDS).items()}
        assert exp["stats"][3] == n * SPP and (n == 1 or (exp["radiance"] != 0).any())
        for want in (abi.RADIANCE_FIELDS,) + tuple((f,) for f in abi.RADIANCE_FIELDS):
            out, rad = _radiance(abi, n, want)
            stats = (C.c_uint64 * abi.NSTATS)(*STATS0)
            assert shim.rt_hip_trace_rays_host(sc.objects, sc.n_objects, meshes, sc.n_meshes, rays.ctypes.data, n, C.byref(p), 0, C.byref(rad),
                                               stats) == 0, shim.rt_hip_last_error()
            for f in want:
                _same(out[f], exp[f], f"trace {name} n={n}, want {want}: {f}")
            _counted(exp["stats"], stats)
    assert gs.launch_status() == 0
    gs.close()
    sc.free()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_trace_pixels_host(gpu, name):
    abi, shim = gpu.abi, gpu.abi.load_shim()
    sc = SCENES[name]()
    gs = gpu.GpuScene(sc)
    pixels = np.ascontiguousarray(np.random.default_rng(97).permutation(sc.width * sc.height)[:max(COUNTS)].astype(np.uint32))
    meshes = sc.hip_meshes()
    p = abi.pixel_params(sc.width, sc.height, SPP, SEED, 2, sc.max_depth)
    for n in COUNTS:
        exp = {f: _host_words(t) for f, t in gs.trace_pixels(pixels[:n], SPP, SEED, sample_first=2, want=abi.PIXEL_FIELDS).items()}
        assert exp["stats"][3] == n * SPP and (n == 1 or (exp["radiance"] != 0).any())
        for want in (abi.PIXEL_FIELDS,) + tuple((f,) for f in abi.PIXEL_FIELDS):
            out, rad = _radiance(abi, n, want)
            stats = (C.c_uint64 * abi.NSTATS)(*STATS0)
            assert shim.rt_hip_trace_pixels_host(sc.objects, sc.n_objects, meshes, sc.n_meshes, C.byref(sc.camera), pixels.ctypes.data, n,
                                                 C.byref(p), 0, C.byref(rad), stats) == 0, shim.rt_hip_last_error()
            for f in want:
                _same(out[f], exp[f], f"pixels {name} n={n}, want {want}: {f}")
            _counted(exp["stats"], stats)
    assert gs.launch_status() == 0
    gs.close()
    sc.free()

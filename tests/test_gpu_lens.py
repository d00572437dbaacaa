"""The thin-lens camera on the GPU (include/rt_hip.h, "thin-lens camera"): the generator's rays equal the restatement
(tests/lens_expected.py) bit for bit; the frame is the stated composition of rt_hip_trace_rays calls, whatever the slices, in the
device form and the host form; per ray the compiled reference's paths and casts; the resolve's edges; every refusal before the first
launch; autofocus; the C host and the CLI.

The compiled reference and the restated rays.  The reference forms a ray from a camera (tests/trace_expected.py: position o,
lower_left_corner q, no extent: the ray is (o, vec3_normalize(o - q))).  It is given o = L and q = L - E 2^200 with E = F - L, the
restated ray's own difference: 2^200 |E_c| is beyond 2^54 |L_c| in every nonzero component, so L - q rounds to E 2^200 exactly, and
vec3_normalize does not see a power of two (its square root, reciprocal and products scale exactly): the reference traces the restated
ray to the bit, which the test asserts."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lens_expected as L
import trace_expected as T
import util

pytestmark = pytest.mark.gpu

W, H, S, DEPTH = 17, 9, 3, 4
NP = W * H
APERTURE, FOCUS = 0.5, 40.0
SCENES = {"room": dict(n_packed=4), "glass": dict(n_packed=4, refr=True), "mesh": dict(n_packed=4, tris=40)}
_CACHE = {}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _stats(a):
    a = np.asarray(a).reshape(-1)
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


def _scene(gpu, name):
    """scene, GpuScene and, once, the composition the frame is stated as: per pass the restated rays and what trace_rays returns"""
    if name not in _CACHE:
        sc = util.class_scene(width=W, height=H, depth=DEPTH, samples=S, **SCENES[name])
        gs = gpu.GpuScene(sc)
        cam = L.camera_tuple(sc.camera)
        passes = []
        for s in range(S):
            rays, info = L.lens_rays(cam, W, H, APERTURE, FOCUS, L.SEED, s, info=True)
            out = gs.trace_rays(rays, 1, L.SEED, index_first=s * NP, want=("status", "radiance", "samples", "paths", "casts", "ray"))
            got = {f: _host(t) for f, t in out.items()}
            got["status"] = got["status"].view(np.uint32)
            passes.append(dict(rays=rays, E=info["F"] - rays[:, :3], **got))
        _CACHE[name] = (sc, gs, passes)
    return _CACHE[name]


def _launches():
    from rt_amd import abi
    shim, total = abi.load_shim(), 0
    for count, each in ((shim.rt_hip_kernel_count, shim.rt_hip_kernel_launches), (shim.rt_hip_trace_kernel_count, shim.rt_hip_trace_kernel_launches)):
        for k in range(count()):
            n = C.c_uint64(0)
            each(k, C.byref(n))
            total += n.value
    return total


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cameras():
    base = util.class_scene(n_packed=4, width=W, height=H)
    out = {"own": base.camera}
    keep = [base]
    for name in ("far", "sheared"):
        sc = util.view_variant(base, name)
        out[name] = sc.camera
        keep.append(sc)
    yield out
    for sc in keep:
        sc.free()


@pytest.mark.parametrize("w,h", L.FRAMES)
def test_rays_equal_the_restatement(gpu, cameras, w, h):
    n_cases = 0
    for sample in L.SAMPLES:
        for name, cam in cameras.items():
            for R in L.APERTURES:
                for f in L.FOCUSES:
                    if (R, f) not in ((0.5, 1.0), (0.0, 1e-3), (2.0 ** -10, 1e3)) and (w, h, name) != (17, 9, "own"):
                        continue   # (the cross product tests/test_lens_cpu.py walks)
                    want = L.lens_rays(L.camera_tuple(cam), w, h, R, f, L.SEED, sample)
                    got = _host(gpu.lens_rays(cam, w, h, R, f, L.SEED, sample))
                    assert (_bits(got) == _bits(want)).all(), (w, h, sample, name, R, f, np.nonzero(_bits(got) != _bits(want))[0][:4])
                    n_cases += 1
    cam = cameras["own"]
    whole = L.lens_rays(L.camera_tuple(cam), w, h, 0.5, 1.0, L.SEED, 1)
    for first, n in L.sub_ranges(w * h):
        got = _host(gpu.lens_rays(cam, w, h, 0.5, 1.0, L.SEED, 1, first, n))
        assert got.shape == (n, 6) and (_bits(got) == _bits(whole[first:first + n])).all(), (w, h, first, n)
    print(f"{w} x {h}: {n_cases} cases and {len(L.sub_ranges(w * h))} sub-ranges equal the restatement bit for bit")


def test_a_sub_range_writes_nothing_outside_itself(gpu, cameras):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    buf = torch.full((65 * 3 + 8, 6), -7.0, dtype=torch.float64, device="cuda")
    lens = abi.lens_params(0.5, 1.0)
    rc = shim.rt_hip_lens_rays(C.byref(cameras["own"]), C.byref(lens), 65, 3, L.SEED, 1, 7, 64, C.c_void_p(buf[4:].data_ptr()), None)
    assert rc == 0
    got = _host(buf)
    want = L.lens_rays(L.camera_tuple(cameras["own"]), 65, 3, 0.5, 1.0, L.SEED, 1, 7, 64)
    assert (got[:4] == -7.0).all() and (got[68:] == -7.0).all() and (_bits(got[4:68]) == _bits(want)).all()


# ---- 2. the composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_frame_is_the_stated_composition(gpu, name):
    sc, gs, passes = _scene(gpu, name)
    for p in passes:
        assert (p["status"] == 1).all() and (_bits(p["ray"]) == _bits(p["rays"])).all()
    total = L.accumulate([p["radiance"] for p in passes], [p["status"] for p in passes])
    want_stats = {k: sum(_stats(p["stats"])[k] for p in passes) for k in ("rays", "casts", "tests", "samples")}
    frames = {}
    for slice_pixels in (1, 64, 100, NP):
        rgb, rgb8, tot, st = gs.render_lens(APERTURE, FOCUS, S, L.SEED, slice_pixels=slice_pixels)
        frames[slice_pixels] = (_host(rgb), _host(rgb8), _host(tot), _stats(_host(st)))
        assert gs.launch_status() == 0
    rgb, rgb8, tot, st = frames[NP]
    assert (_bits(tot.reshape(-1, 3)) == _bits(total)).all(), f"{name}: (c) sum is not the ascending vec3_add of the samples"
    mean = L.mean_of(tot, S)
    assert (_bits(rgb) == _bits(L.float_of(mean))).all(), f"{name}: (c) rgb is not float(sum * (1 / S))"
    differ, at_boundary = L.bytes_agree(rgb8, mean)
    print(f"{name}: {differ} of {rgb8.size} bytes differ from the host's tonemap of the same mean")
    assert at_boundary, f"{name}: a byte differs away from a byte boundary"
    assert st == want_stats, (name, st, want_stats)
    for slice_pixels, other in frames.items():                                           # (d)
        for a, b in zip(other[:3], frames[NP][:3]):
            assert (_bits(a) == _bits(b)).all(), f"{name}: slice_pixels = {slice_pixels} changes the frame"
        assert other[3] == st
    # the host form, on the HIP device and on a logical one
    from rt_amd import abi
    shim = abi.load_shim()
    h_rgb, h_rgb8, h_st = gpu.render_lens_host(sc, APERTURE, FOCUS, S, L.SEED)
    assert (_bits(h_rgb) == _bits(rgb)).all() and (h_rgb8 == rgb8).all() and h_st == st
    assert shim.rt_hip_set_device_map((C.c_int * 3)(0, 0, 0), 3) == 0
    try:
        m_rgb, m_rgb8, m_st = gpu.render_lens_host(sc, APERTURE, FOCUS, S, L.SEED, device=2)
        with pytest.raises(gpu.ShimError):
            gpu.render_lens_host(sc, APERTURE, FOCUS, S, L.SEED, device=3)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    assert (_bits(m_rgb) == _bits(rgb)).all() and (m_rgb8 == rgb8).all() and m_st == st


def test_slices_end_at_every_sample_pass(gpu):
    """5 x 3 pixels, 3 samples: a slice that does not divide the pass (4), one short of it (14), the pass (15) and slices larger than
    it (16, 2^31) give the whole-frame call's outputs and counters bit for bit, and that frame is the composition over the passes'
    own rays -- lens_rays(sample = s), traced at index_first = s * 15 -- which a slice running on into the next pass would break"""
    w, h, s_count = 5, 3, 3
    sc = util.class_scene(width=w, height=h, depth=DEPTH, samples=s_count, n_packed=4)
    gs = gpu.GpuScene(sc)
    radiance, status = [], []
    for s in range(s_count):
        rays = L.lens_rays(L.camera_tuple(sc.camera), w, h, APERTURE, FOCUS, L.SEED, s)
        assert (_bits(_host(gpu.lens_rays(sc.camera, w, h, APERTURE, FOCUS, L.SEED, s))) == _bits(rays)).all(), s
        out = gs.trace_rays(rays, 1, L.SEED, index_first=s * w * h)
        radiance.append(_host(out["radiance"]))
        status.append(_host(out["status"]).view(np.uint32))
    whole = [_host(t) for t in gs.render_lens(APERTURE, FOCUS, s_count, L.SEED)]
    assert (_bits(whole[2].reshape(-1, 3)) == _bits(L.accumulate(radiance, status))).all()
    for slice_pixels in (1, 4, 14, 15, 16, 2 ** 31):
        got = [_host(t) for t in gs.render_lens(APERTURE, FOCUS, s_count, L.SEED, slice_pixels=slice_pixels)]
        assert gs.launch_status() == 0
        for a, b in zip(got, whole):   # rgb, rgb8, sum, counters
            assert (_bits(a) == _bits(b)).all(), f"slice_pixels = {slice_pixels} changes the frame"
    gs.close()
    sc.free()


# ---- 3. the compiled reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_paths_casts_and_values_equal_the_reference(gpu, ref_mesh, pt, name):
    sc, gs, passes = _scene(gpu, name)
    glass = name == "glass"
    ref_mean = np.zeros((NP, 3))
    for s, p in enumerate(passes):
        o = p["rays"][:, :3]
        ref = T.reference_samples(ref_mesh(DEPTH), sc, o, o - p["E"] * 2.0 ** 200, 1, L.SEED, s * NP, casts_oracle=pt)
        assert (_bits(ref["rays"]) == _bits(p["rays"])).all(), "the reference's ray is not the restated ray"
        assert (p["paths"].view(np.uint64) == ref["paths"]).all(), f"{name} pass {s}: paths differ"
        assert (p["casts"].view(np.uint64) == ref["casts"]).all(), f"{name} pass {s}: casts differ"
        err, bar = np.abs(p["samples"] - ref["samples"]), T.value_bar(ref["samples"], glass)
        assert (err <= bar).all(), f"{name} pass {s}: {(err > bar).sum()} values beyond 2^-40"
        ref_mean = ref_mean + ref["samples"][:, 0]
    ref_mean = ref_mean * (1.0 / S)
    _, rgb8, _, _ = gs.render_lens(APERTURE, FOCUS, S, L.SEED)
    rgb8 = _host(rgb8).reshape(-1, 3)
    want8, scaled = L.tonemap(ref_mean)
    differ = rgb8 != want8
    print(f"{name}: {int(differ.sum())} of {rgb8.size} bytes differ from the tonemap of the oracle's mean")
    assert (np.abs(rgb8.astype(int) - want8.astype(int)) <= 1).all()
    assert (np.abs(scaled - np.round(scaled))[differ] <= 2.0 ** -30 * np.maximum(scaled[differ], 1.0)).all(), \
        f"{name}: a byte differs at a mean that is not within 2^-30 of a byte boundary"


# ---- 4. the resolve's edges -----------------------------------------------------------------------------------------------------------
def test_resolve_edges(gpu):
    """NaN, negative, zeros, above 1, denormal, infinite sums through rt_hip_lens_resolve: the float is float(sum * (1 / S)) to the bit,
    the byte the accumulation resolve's rule -- (uint8)(255 MAX(0, MIN(pow(mean, 1 / 5), 1))) with a NaN power reading 1 -> 255"""
    import torch
    vals = np.array([np.nan, -np.nan, -1.0, -0.0, 0.0, 5e-324, 2.2e-308, 1e-300, 1e-12, 0.25, 0.999999, 1.0, 1.0000001, 3.0, 7.5, 1e300,
                     np.inf, -np.inf, -5e-324, 2.0 ** -30, 0.5, 1.5, 2.9999, 1e-5])
    total = np.resize(vals, (3, 8, 3)).astype(np.float64)
    for samples in (1, 3, 64):
        rgb, rgb8 = gpu.lens_resolve(torch.as_tensor(total, device="cuda"), samples)
        rgb, rgb8 = _host(rgb), _host(rgb8)
        mean = L.mean_of(total, samples)
        want = L.float_of(mean)
        both_nan = np.isnan(rgb) & np.isnan(want)
        assert ((_bits(rgb) == _bits(want)) | both_nan).all()
        differ, at_boundary = L.bytes_agree(rgb8, mean)
        assert at_boundary, samples
        nan, neg = np.isnan(mean), mean < 0
        assert (rgb8[nan] == 255).all() and (rgb8[neg] == 255).all(), "pow of a negative mean is NaN, and NaN reads 1 (MIN's comparison is false)"
        assert (rgb8[mean == 0] == 0).all() and (rgb8[mean >= 1] == 255).all()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs, _ = _scene(gpu, "room")
    glass_sc, glass, _ = _scene(gpu, "glass")
    ws = torch.full((shim.rt_hip_lens_workspace_bytes(W, H, NP),), 0x5A, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (24 * NP, 12 * NP, 3 * NP, 32)]
    torch.cuda.synchronize()
    before = _launches()

    def frame(handle=gs.handle, cam=sc.camera, R=APERTURE, f=FOCUS, w=W, h=H, samples=S, depth=DEPTH, integrator="path", slice_pixels=NP,
              workspace=ws, lens=True, params=True, tiles=(0, 0, 0), outputs=True, flags=0, ws_offset=0, sum_offset=0):
        p = abi.RtHipParams()
        p.width, p.height, p.samples, p.max_depth, p.seed = w, h, samples, depth, L.SEED
        p.integrator = abi.INTEGRATORS[integrator]
        p.tile_first, p.tile_stride, p.tile_count = tiles
        ln = abi.lens_params(R, f)
        ln.flags = flags
        ptr = [C.c_void_p(t.data_ptr()) if outputs else None for t in outs]
        return shim.rt_hip_render_lens(handle, C.byref(cam) if cam is not None else None, C.byref(ln) if lens else None,
                                       C.byref(p) if params else None, slice_pixels, C.c_void_p(workspace.data_ptr() + ws_offset) if workspace is not None else None,
                                       C.c_void_p(outs[0].data_ptr() + sum_offset) if outputs else None, ptr[1], ptr[2], ptr[3] if outputs else None, None)

    EINVAL, ELIMIT = -2, -5
    cases = {
        "aperture < 0": (dict(R=-1e-9), EINVAL), "aperture NaN": (dict(R=float("nan")), EINVAL), "aperture inf": (dict(R=float("inf")), EINVAL),
        "focus 0": (dict(f=0.0), EINVAL), "focus < 0": (dict(f=-1.0), EINVAL), "focus NaN": (dict(f=float("nan")), EINVAL),
        "focus inf": (dict(f=float("inf")), EINVAL), "width 1": (dict(w=1), EINVAL), "height 1": (dict(h=1), EINVAL),
        "samples 0": (dict(samples=0), EINVAL), "samples x pixels > 2^32": (dict(w=2 ** 16, h=2 ** 15, samples=3), EINVAL),
        "slice_pixels 0": (dict(slice_pixels=0), EINVAL), "cast_ray": (dict(integrator="whitted"), EINVAL),
        "part of the frame": (dict(tiles=(1, 1, 1)), EINVAL), "lens flags": (dict(flags=1), EINVAL), "max_depth < 0": (dict(depth=-1), EINVAL),
        "no scene": (dict(handle=None), EINVAL), "no camera": (dict(cam=None), EINVAL), "no lens": (dict(lens=False), EINVAL),
        "no params": (dict(params=False), EINVAL), "no workspace": (dict(workspace=None), EINVAL), "no output": (dict(outputs=False), EINVAL),
        "workspace not 16-byte aligned": (dict(ws_offset=8), EINVAL), "sum not 8-byte aligned": (dict(sum_offset=4), EINVAL),
        "glass beyond depth 32": (dict(handle=glass.handle, depth=33), ELIMIT),
    }
    for what, (kw, code) in cases.items():
        assert frame(**kw) == code, (what, shim.rt_hip_last_error())
    # the generator and the resolve
    rays = torch.full((NP + 1, 6), -7.0, dtype=torch.float64, device="cuda")
    ln = abi.lens_params(APERTURE, FOCUS)
    gen = lambda w=W, h=H, sample=0, first=0, n=NP, ptr=rays.data_ptr(), lens=ln: shim.rt_hip_lens_rays(
        C.byref(sc.camera), C.byref(lens), w, h, L.SEED, sample, first, n, C.c_void_p(ptr), None)
    assert gen(first=1) == EINVAL and gen(n=NP + 1) == EINVAL and gen(ptr=rays.data_ptr() + 8) == EINVAL and gen(ptr=None) == EINVAL
    assert gen(sample=2 ** 32 // NP) == EINVAL and gen(w=1) == EINVAL and gen(lens=abi.lens_params(-1.0, 1.0)) == EINVAL
    assert gen(n=0, ptr=None) == 0
    assert shim.rt_hip_lens_resolve(None, W, H, 1, C.c_void_p(outs[1].data_ptr()), None, None) == EINVAL
    assert shim.rt_hip_lens_resolve(C.c_void_p(outs[0].data_ptr()), W, H, 0, C.c_void_p(outs[1].data_ptr()), None, None) == EINVAL
    # the host form: arguments before the device is looked for -- device 99 does not exist (RT_HIP_ENODEV with good arguments), and a
    # bad argument is reported first (RT_HIP_EINVAL, naming it)
    p = abi.RtHipParams()
    p.width, p.height, p.samples, p.max_depth, p.seed = W, H, 0, DEPTH, L.SEED
    img = np.full((H, W, 3), 7, dtype=np.uint8)
    host_form = lambda: shim.rt_hip_render_lens_image(sc.objects, sc.n_objects, sc.hip_meshes(), sc.n_meshes, C.byref(sc.camera), C.byref(ln),
                                                      C.byref(p), 99, None, img.ctypes.data, None)
    assert host_form() == EINVAL and b"samples" in shim.rt_hip_last_error()
    p.samples = S
    assert host_form() == -1 and b"samples" not in shim.rt_hip_last_error()   # RT_HIP_ENODEV
    assert (img == 7).all()
    torch.cuda.synchronize()
    assert _launches() == before, "a refusal launched a render or radiance-query kernel"
    for t in outs + [ws]:
        assert bool((t == 0x5A).all()), "a refusal wrote into an output or the workspace"
    assert bool((rays == -7.0).all())
    assert gs.launch_status() == 0


# ---- 6. autofocus -------------------------------------------------------------------------------------------------------------------------
def test_focus_at(gpu):
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=2.0, center=(0.3, -0.2, 1.0), color=(0.8, 0.7, 0.6), emission=(0.0, 0.0, 0.0))]
    sc = S.custom_scene(objs, W, H, 1, DEPTH, (1.0, 2.0, 12.0), (0.3, -0.2, 1.0))
    gs = gpu.GpuScene(sc)
    x, y = W // 2, H // 2
    f = gs.focus_at(x, y)
    hit = gs.pick(x, y)
    assert f is not None and hit["status"] == 1
    pos, hor, ver, llc = (np.array(c) for c in L.camera_tuple(sc.camera))
    u, v = (x + 0.5) / (W - 1.0), (y + 0.5) / (H - 1.0)
    d = pos - (llc + (hor * u + ver * v))
    point = np.array(hit["point"])
    assert np.linalg.norm(pos + d * f - point) <= 2.0 ** -40 * np.linalg.norm(point), (f, point)
    assert gs.focus_at(0, 0) is None and gs.pick(0, 0)["status"] == 0
    gs.close()
    sc.free()


# ---- 7. the C host and the CLI ---------------------------------------------------------------------------------------------------------
def _png_rgb(path):
    """the pixels of an 8-bit RGB PNG without interlace (what stbi_write_png writes) -> uint8 [h, w, 3]"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, w, h = 8, b"", 0, 0
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, interlace) == (8, 2, 0)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), dtype=np.int64)
    for r in range(h):
        kind, line = int(raw[r, 0]), raw[r, 1:].astype(np.int64)
        up = out[r - 1] if r else np.zeros(3 * w, dtype=np.int64)
        for i in range(3 * w):
            a = out[r, i - 3] if i >= 3 else 0
            c = up[i - 3] if i >= 3 else 0
            b = up[i]
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[r, i] = (line[i] + (0, a, b, (a + b) // 2, paeth)[kind]) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


def test_c_host_and_cli(gpu, tmp_path):
    from rt_amd import abi, scene as S
    host = abi.load_host()
    seed, focus = 20261021, 3.0
    sc = S.build_scene(1, W, H, S_CLI, DEPTH)
    opt = abi.Options()
    opt.width, opt.height, opt.samples = W, H, S_CLI
    depth0, seed0 = host.rt_get_max_depth(), host.rt_get_seed()
    host.rt_set_max_depth(DEPTH)
    host.rt_set_seed(seed)

    def render():
        fb = np.zeros((H, W, 3), dtype=np.uint8)
        host.render(fb.ctypes.data, sc.objects, sc.n_objects, C.byref(sc.camera), C.byref(opt))
        return fb
    try:
        a, f = C.c_double(-1), C.c_double(-1)
        host.rt_get_lens(C.byref(a), C.byref(f))
        assert (a.value, f.value) == (0.0, 1.0)
        pinhole = render()
        host.rt_set_lens(0.05, focus)
        host.rt_get_lens(C.byref(a), C.byref(f))
        assert (a.value, f.value) == (0.05, focus)
        with_lens = render()
        host.rt_set_lens(0.0, focus)
        assert (render() == pinhole).all(), "aperture 0 must leave render() on the pinhole path"
    finally:
        host.rt_set_lens(0.0, 1.0)
        host.rt_set_max_depth(depth0)
        host.rt_set_seed(seed0)
    _, want8, _ = gpu.render_lens_host(sc, 0.05, focus, S_CLI, seed, max_depth=DEPTH)
    assert (with_lens == want8).all() and (with_lens != pinhole).any()
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    out = tmp_path / "lens.png"
    r = subprocess.run([cli, "-w", str(W), "-h", str(H), "-s", str(S_CLI), "-c", "1", "-d", str(DEPTH), "-r", str(seed), "-l", f"0.05,{focus:g}",
                        "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (_png_rgb(out) == want8).all()
    for bad in ("0.05", "-1,3", "0.05,0", "x,3"):
        r = subprocess.run([cli, "-w", str(W), "-h", str(H), "-s", "1", "-l", bad, "-o", os.devnull], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stderr, bad
    sc.free()


# ---- invalid rays: status 2 makes the pixel NaN -------------------------------------------------------------------------------------------
def test_invalid_rays_make_their_pixels_nan(gpu):
    """A camera whose vertical is 1.9e154 long: for v > 0.71 the square of F - L overflows, vec3_normalize gives a zero direction and
    rt_hip_trace_rays calls the ray invalid (status 2); above that the rays are ordinary.  The frame's sum is NaN in all three
    channels at exactly the pixels a pass found invalid -- rows of the frame, so a status word read at the wrong index would show --
    and the stated sum everywhere else; the byte of a NaN mean is 255."""
    sc, gs, _ = _scene(gpu, "room")
    pos, hor, ver, llc = util.camera_arrays(sc.camera)
    cam = util.hand_camera(pos, hor, (0.0, 1.9e154, 0.0), (llc[0], 0.0, llc[2]))
    passes, statuses = [], []
    for s in range(S):
        rays = L.lens_rays(L.camera_tuple(cam), W, H, APERTURE, 1.0, L.SEED, s)
        assert (_bits(_host(gpu.lens_rays(cam, W, H, APERTURE, 1.0, L.SEED, s))) == _bits(rays)).all()
        out = gs.trace_rays(rays, 1, L.SEED, index_first=s * NP, want=("status", "radiance"))
        statuses.append(_host(out["status"]).view(np.uint32))
        passes.append(_host(out["radiance"]))
    bad = np.any([st == 2 for st in statuses], axis=0)
    assert 0 < bad.sum() < NP and not bad[:3 * W].any() and bad[-2 * W:].all(), bad.reshape(H, W).sum(axis=1)
    assert any(0 < n < W for st in statuses for n in (st == 2).reshape(H, W).sum(axis=1)), "no pass splits a row: the jitter should"
    want = L.accumulate(passes, statuses)
    for slice_pixels in (NP, 100):
        _, rgb8, tot, _ = gs.render_lens(APERTURE, 1.0, S, L.SEED, camera=cam, slice_pixels=slice_pixels)
        tot, rgb8 = _host(tot).reshape(-1, 3), _host(rgb8).reshape(-1, 3)
        assert (np.isnan(tot) == bad[:, None]).all()
        assert (_bits(tot[~bad]) == _bits(want[~bad])).all() and (_bits(tot[bad]) == 0x7FF8000000000000).all()
        assert (rgb8[bad] == 255).all()
    gs.launch_status()


# ---- 8. the optics ----------------------------------------------------------------------------------------------------------------------------
def test_defocus_spreads_a_sphere_over_more_pixels(gpu):
    """33 x 17, 64 samples, a black room and one emitter: on the focal plane (1.5 ahead, radius 0.15), or twice as far and twice as
    large (the same pinhole footprint).  A pixel is lit when a channel of its sum is above 0.  The CPU run with the restated rays
    (tests/test_lens_cpu.py, lens_expected.OPTICS_LIT) gave 12 and 12 lit pixels at aperture 0 and 12 and 24 at aperture 0.25: the
    defocused sphere must light strictly more, and at aperture 0 the two counts are equal."""
    o = L.OPTICS
    lit = {}
    for k in (1, 2):
        sc = L.optics_scene(k)
        gs = gpu.GpuScene(sc)
        for R in (0.0, o["aperture"]):
            _, _, tot, _ = gs.render_lens(R, o["focus"], o["samples"], L.SEED)
            tot = _host(tot).reshape(-1, 3)
            assert np.isfinite(tot).all()
            lit[(R, k)] = int((tot > 0).any(axis=1).sum())
        assert gs.launch_status() == 0
        gs.close()
        sc.free()
    print("lit pixels (aperture, k):", lit, "-- the CPU run:", L.OPTICS_LIT)
    assert lit[(o["aperture"], 2)] > lit[(o["aperture"], 1)]
    assert lit[(0.0, 1)] == lit[(0.0, 2)]
    assert lit == L.OPTICS_LIT, "the device lights other pixels than the restated rays do"


S_CLI = 4


def test_zz_close(gpu):
    for sc, gs, _ in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

"""The denoiser (rt_hip_denoise) over the rest of its accepted range: the late iterations whose taps lie 64 .. 1,024 pixels away
(every one outside most images, and inside a 1,100-wide one), the normal weight squared 8 .. 10 times (fp64 overflow, and
underflow through denormals to 0), sigmas at the ends of what the arguments check accepts, images one pixel wide or high and
around the 16 x 16 workgroup's edges, the largest accepted side, buffers that hold FLT_MAX, float32 denormals, -0.0, negative
values, an albedo of exactly -2^-10, depths of FLT_MAX, -inf and 0 (denoise_expected._edge_inputs), real frames under the view and
placement variants of util.py, and a logical device of a device map.  As in tests/test_gpu_denoise.py the floats equal the numpy
restatement (tests/denoise_expected.py, itself pinned against a scalar restatement at these edges by tests/test_denoise_cpu.py)
BIT FOR BIT, NaN equal to NaN, and the bytes are within 1 LSB of the oracle's tonemap of those floats."""
import ctypes as C
import math

import numpy as np
import pytest

from denoise_expected import COLD, HOT, _edge_inputs, denoise_aov
from test_gpu_denoise import _check, _expected_kw, _kw, _random_inputs, _to_dev
from util import VARIANTS, aov_view_scene

pytestmark = pytest.mark.gpu

SEED = 1666943821
# sigma_color: S2 = (sigma_color * 2^-i)^2 must stay finite and non-zero for every i < 10: from the first double above
# 2^-528.5 (S2 rounds to 2^-1074, the smallest fp64 denormal, at i = 9; one double lower it rounds to 0) up to the double below
# 2^512 (S2 just below 2^1024 at i = 0).  sigma_depth: any finite double > 0.
SIGMA_COLOR_MIN, SIGMA_COLOR_MAX = float.fromhex("0x1.6a09e667f3bcdp-529"), math.nextafter(2.0 ** 512, 0.0)
SIGMA_DEPTH_MIN, SIGMA_DEPTH_MAX = 5e-324, 1.7976931348623157e308
SIGMAS = ((0.5, 1.0), (1e-6, 1e6), (1e6, 1e-6), (SIGMA_COLOR_MIN, SIGMA_DEPTH_MAX), (SIGMA_COLOR_MAX, SIGMA_DEPTH_MIN),
          (SIGMA_COLOR_MIN, SIGMA_DEPTH_MIN), (SIGMA_COLOR_MAX, SIGMA_DEPTH_MAX))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_shim().rt_hip_set_device_map(None, 0)


def test_the_sigma_ends_are_the_ends():
    sq = lambda x: x * x
    assert sq(SIGMA_COLOR_MIN * 2.0 ** -9) == 5e-324 and sq(math.nextafter(SIGMA_COLOR_MIN, 0.0) * 2.0 ** -9) == 0.0
    assert math.isfinite(sq(SIGMA_COLOR_MAX)) and math.isinf(sq(2.0 ** 512))
    assert math.nextafter(SIGMA_DEPTH_MIN, 0.0) == 0.0 and math.isinf(math.nextafter(SIGMA_DEPTH_MAX, math.inf))


def _near_parallel_normals(aov, rng, overflow):
    """normals for which the late squarings matter: most within a few degrees of one direction and of length about 1 (g in
    0.98 .. 1.02: g^1024 spans 1e-9 .. 1e9, and g^512 is another number), columns of (0, 0, 0.6974) (g = 2^-1.04: g^1024 =
    2^-1065, an fp64 denormal) and of (0, 0, 0.5) (g = 1/4: 2^-1024 at k = 9, 0 at 10); overflow: a tenth of length 1e2 (g^256
    is inf; a weight of inf makes the pixel NaN, and within ten iterations every pixel)"""
    h, w = aov["depth"].shape
    n = np.float32([0.3, 0.2, 0.93]) + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32)
    n = n / np.linalg.norm(n.astype(np.float64), axis=2, keepdims=True) * (1 + rng.normal(0, 0.004, (h, w, 1)))
    n = n.astype(np.float32)
    if overflow:
        n[rng.random((h, w)) < 0.1] *= np.float32(1e2)
    n[:, 3::11] = np.float32([0, 0, 0.6974])
    n[:, 4::11] = np.float32([0, 0, 0.6974])
    n[:, 7::11] = np.float32([0, 0, 0.5])
    n[:, 8::11] = np.float32([0, 0, 0.5])
    n[aov["hits"] == 0] = 0
    aov["normal"] = n
    return aov


def _late_inputs(w, h, flags, kind):
    """clean: ordinary values only (_edge_inputs with nothing planted) -- nothing non-finite arises at moderate sigmas, so the
    comparison is one of numbers; rough: _random_inputs (NaN / inf colours, NaN normals, inf depths on hits) with overflowing
    normal weights -- ten iterations carry a NaN everywhere, and the comparison is one of which pixels pass through"""
    rng = np.random.default_rng(w * 131 + h * 7 + flags)
    if kind == "clean":
        rgb, aov, _ = _edge_inputs(w, h, rng, hot_band=0.0, share=0.0)
    else:
        rgb, aov = _random_inputs(w, h, rng)
    return rgb, _near_parallel_normals(aov, rng, overflow=kind == "rough")


@pytest.mark.parametrize("kind", ["clean", "rough"])
@pytest.mark.parametrize("size", [(37, 21), (1100, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_late_iterations_and_high_normal_powers(gpu, size, flags, kind):
    """L in {7, 8, 9, 10} x k in {8, 9, 10}: at 37 x 21 every tap of the iterations from step 64 on lies outside (the pixel keeps
    float((9/64 e) / (9/64))); at 1,100 x 12 the step-512 taps at +-512 and +-1,024 land inside for part of the pixels.  The
    sigma pairs go round SIGMAS; at the first three (the moderate ones) the clean inputs' expectation is finite throughout"""
    import torch
    w, h = size
    rgb, aov = _late_inputs(w, h, flags, kind)
    d_rgb, d_aov = torch.from_numpy(rgb).cuda(), _to_dev(aov)
    n = 0
    for L in (7, 8, 9, 10):
        for k in (8, 9, 10):
            sc, sz = SIGMAS[n % len(SIGMAS)]
            kw = _kw(flags, iterations=L, normal_power_log2=k, sigma_color=sc, sigma_depth=sz)
            exp = denoise_aov(rgb, aov, **_expected_kw(kw))
            if kind == "clean" and n % len(SIGMAS) < 3:
                assert np.isfinite(exp).all(), f"{w}x{h} flags {flags} L {L} k {k} sigma {sc} {sz}: the expectation is not finite"
            n += 1
            out, out8 = gpu.denoise(d_rgb, d_aov, w, h, **kw)
            torch.cuda.synchronize()
            _check(out, out8, exp, f"{kind} {w}x{h} flags {flags} L {L} k {k} sigma {sc} {sz}")


def test_the_normal_power_and_the_far_taps_show_in_the_expectation():
    """the clean cases above can tell k = 10 from k = 9, and a tap 512 or 1,024 pixels away from none: on the restatement alone"""
    w, h = 1100, 12
    rgb, aov = _late_inputs(w, h, 0, "clean")
    p = dict(iterations=10, flags=0, sigma_color=1e6, sigma_depth=1e6)
    a = denoise_aov(rgb, aov, normal_power_log2=10, **p)
    b = denoise_aov(rgb, aov, normal_power_log2=9, **p)
    assert np.isfinite(a).all() and (a.view(np.uint32) != b.view(np.uint32)).mean() > 0.2
    c = denoise_aov(rgb[:, :500], {f: v[:, :500] for f, v in aov.items()}, normal_power_log2=10, **p)
    assert (a[:, :500].view(np.uint32) != c.view(np.uint32)).mean() > 0.2   # columns < 500 see columns >= 512 only through far taps
    # 37 x 21: from step 64 on nothing is inside -- the late iterations change nothing but must still run
    rgb, aov = _late_inputs(37, 21, 0, "clean")
    p = dict(flags=0, sigma_color=0.5, sigma_depth=1.0, normal_power_log2=8)
    assert np.array_equal(denoise_aov(rgb, aov, iterations=10, **p), denoise_aov(rgb, aov, iterations=6, **p))


SHAPES = [(1, n) for n in range(1, 41)] + [(n, 1) for n in range(2, 41)] + \
         [(n, 21) for n in (15, 16, 17, 31, 32, 33)] + [(37, n) for n in (15, 16, 17, 31, 32, 33)] + [(16, 16), (17, 33), (33, 17)]


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_thin_images_and_workgroup_edges(gpu, size):
    import torch
    from rt_amd import abi
    w, h = size
    assert abi.load_shim().rt_hip_denoise_workspace_bytes(w, h) >= 56 * w * h
    rng = np.random.default_rng(w * 4099 + h)
    rgb, aov, _ = _edge_inputs(w, h, rng, hot_band=0.0)
    d_rgb, d_aov = torch.from_numpy(rgb).cuda(), _to_dev(aov)
    for flags, L in ((3, 6), ((w + h) % 4, 3), (0, 1)):
        kw = _kw(flags, iterations=L)
        out, out8 = gpu.denoise(d_rgb, d_aov, w, h, **kw)
        torch.cuda.synchronize()
        _check(out, out8, denoise_aov(rgb, aov, **_expected_kw(kw)), f"{w}x{h} flags {flags} L {L}")


@pytest.mark.parametrize("size", [(1 << 20, 1), (1, 1 << 20)], ids=["2^20x1", "1x2^20"])
def test_the_largest_accepted_side(gpu, size):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    w, h = size
    assert shim.rt_hip_denoise_workspace_bytes(w, h) >= 56 * w * h
    assert shim.rt_hip_denoise_workspace_bytes(w + (h == 1), h + (w == 1)) == 0   # 2^20 + 1
    rgb, aov = _random_inputs(w, h, np.random.default_rng(20))
    kw = _kw(3, iterations=3)
    out, out8 = gpu.denoise(torch.from_numpy(rgb).cuda(), _to_dev(aov), w, h, **kw)
    torch.cuda.synchronize()
    _check(out, out8, denoise_aov(rgb, aov, **_expected_kw(kw)), f"{w}x{h}")


EDGE_SIZE = (320, 200)   # the hot values live in x < 40; five iterations carry a non-finite signal 62 pixels: x < 102 of 320


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_edge_values(gpu, flags):
    """every value of denoise_expected.COLD and HOT, L in {1, 5}.  A valid pixel may come out inf or NaN: that is the contract.
    So that NaN == NaN cannot hide everything, the EXPECTATION has at most half of its valid pixels non-finite after L = 5"""
    import torch
    w, h = EDGE_SIZE
    rgb, aov, planted = _edge_inputs(w, h, np.random.default_rng(99))
    assert all(len(planted[c]) >= 100 for c in COLD + HOT), {c: len(v) for c, v in planted.items()}
    valid = np.isfinite(rgb).all(axis=2)
    d_rgb, d_aov = torch.from_numpy(rgb).cuda(), _to_dev(aov)
    for L in (1, 5):
        kw = _kw(flags, iterations=L)
        exp = denoise_aov(rgb, aov, **_expected_kw(kw))
        bad = float((~np.isfinite(exp).all(axis=2) & valid).sum()) / float(valid.sum())
        print(f"flags {flags} L {L}: {bad:.3f} of the valid pixels are non-finite in the expectation")
        assert bad <= 0.5
        out, out8 = gpu.denoise(d_rgb, d_aov, w, h, **kw)
        torch.cuda.synchronize()
        _check(out, out8, exp, f"edge values flags {flags} L {L}")


# three classes as the denoiser's users have them, and one without its back wall: misses (depth +inf, no object) next to hits
FRAME_CLASSES = [dict(n_packed=4), dict(n_packed=4, tris=40, mesh_chk=True), dict(n_packed=4, wide=True, chk=True),
                 dict(n_packed=4, chk=True, open_back=True)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cls", FRAME_CLASSES, ids=["spheres", "flat_mesh_chk", "wide_chk", "open_chk"])
def test_real_frames_under_the_variants(gpu, cls, variant):
    """render_image's floats and aov_image's buffers of the same scene, seed and samples, denoised with flags 1 and 3 at the
    default L: depths 2e7 out, of size 1e-3 and 1e5, a floor of radius 1e19, a telephoto frame of almost constant guidance"""
    sc = aov_view_scene(cls, variant, width=48, height=32, samples=4)
    gs = gpu.GpuScene(sc)
    image, _, _ = gs.render_image(SEED, 4)
    rgb, aov = image.cpu().numpy(), gs.aov_image(SEED, 4)
    assert (aov["hits"] == 4).any()
    for flags in (1, 3):
        kw = _kw(flags)
        noisy, den, den8 = gs.denoised_image(SEED, 4, **kw)
        assert np.array_equal(noisy.view(np.uint32), rgb.view(np.uint32))
        exp = denoise_aov(rgb, aov, **_expected_kw(kw))
        assert np.isfinite(exp).all() and (exp.view(np.uint32) != rgb.view(np.uint32)).any()
        _check(den, den8, exp, f"{cls} {variant} flags {flags}")
    gs.close()
    sc.free()


def test_the_image_entry_point_on_a_logical_device(gpu):
    """rt_hip_denoise_image(..., device=2, ...) under the device map (0, 0, 0): device 0's output, and the restatement's"""
    from rt_amd import abi
    shim = abi.load_shim()
    w, h = 45, 30
    rgb, aov, _ = _edge_inputs(w, h, np.random.default_rng(45), hot_band=0.0)
    a = abi.RtHipAov()
    for f, v in aov.items():
        setattr(a, f, v.ctypes.data)
    kw = _kw(3, iterations=4)
    p = abi.denoise_params(**kw)

    def run(device):
        out, out8 = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.uint8)
        rc = shim.rt_hip_denoise_image(rgb.ctypes.data, C.byref(a), w, h, C.byref(p), device, out.ctypes.data, out8.ctypes.data)
        return rc, out, out8
    assert shim.rt_hip_set_device_map(None, 0) == 0
    rc, zero, zero8 = run(0)
    assert rc == 0, shim.rt_hip_last_error()
    arr = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(arr, 3) == 0, shim.rt_hip_last_error()
    try:
        rc, two, two8 = run(2)
        assert rc == 0, shim.rt_hip_last_error()
        assert run(3)[0] == abi.ENODEV   # beyond the map
    finally:
        shim.rt_hip_set_device_map(None, 0)
    assert np.array_equal(two.view(np.uint32), zero.view(np.uint32)) and np.array_equal(two8, zero8)
    _check(two, two8, denoise_aov(rgb, aov, **_expected_kw(kw)), "logical device 2")

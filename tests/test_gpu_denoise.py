"""The denoiser on the GPU (rt_hip_denoise): its output equals the numpy restatement of the contract (tests/denoise_expected.py)
BIT FOR BIT in floats (NaN equal to NaN), and its bytes are within 1 LSB of the oracle's tonemap of those floats -- on seeded random
buffers (any contents: the contract is total), on real frames and their first-hit buffers, on a progressive accumulation after
passes; in place, with one output, on a second stream; through the host library and the CLI's -n.  And it does what it is for: a
16-spp frame of the 38-sphere room moves closer to the 1024-spp frame."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from denoise_expected import denoise_aov, same_floats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1666943821
FLAGS = {0: {}, 1: dict(demodulate=True), 2: dict(demodulate=False, object_edges=True), 3: dict(demodulate=True, object_edges=True)}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _kw(flags, **p):
    kw = dict(FLAGS[flags])
    kw.setdefault("demodulate", False)
    kw.setdefault("object_edges", False)
    kw.update(p)
    return kw


def _expected_kw(kw):
    """abi.denoise_params' keywords -> denoise_expected's"""
    from rt_amd import abi
    p = abi.denoise_params(**kw)
    return dict(iterations=p.iterations, sigma_color=p.sigma_color, normal_power_log2=p.normal_power_log2, sigma_depth=p.sigma_depth,
                flags=p.flags)


def _to_dev(aov):
    import torch
    out = {}
    for f, a in aov.items():
        a = np.ascontiguousarray(a)
        out[f] = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    return out


def _check(gpu_rgb, gpu_rgb8, exp, what):
    from oracle_py import PtOracle
    g = gpu_rgb.cpu().numpy() if hasattr(gpu_rgb, "cpu") else gpu_rgb
    assert same_floats(g, exp), f"{what}: {int((~((g.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(g) & np.isnan(exp)))).sum())} floats differ"
    if gpu_rgb8 is not None:
        g8 = gpu_rgb8.cpu().numpy() if hasattr(gpu_rgb8, "cpu") else gpu_rgb8
        want8 = PtOracle().tonemap(exp.reshape(-1, 3).astype(np.float64)).reshape(exp.shape)
        d = np.abs(g8.astype(int) - want8.astype(int)).max()
        assert d <= 1, f"{what}: bytes differ by {d} LSB"


def _random_inputs(w, h, rng):
    """any contents: NaN / inf colours, zero albedo, normals that are not unit (and some NaN), depth with 0 hits, hits 0 with a
    depth, objects of a few ids"""
    rgb = (rng.random((h, w, 3)) * rng.choice([0.1, 1.0, 30.0], (h, w, 1))).astype(np.float32)
    bad = rng.random((h, w)) < 0.03
    rgb[bad, rng.integers(0, 3, bad.sum())] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), bad.sum())
    albedo = rng.random((h, w, 3)).astype(np.float32)
    albedo[rng.random((h, w)) < 0.05] = 0
    normal = (rng.random((h, w, 3)) * 2 - 1).astype(np.float32)
    normal[rng.random((h, w)) < 0.01] = np.nan
    depth = (rng.random((h, w)) * 20).astype(np.float32)
    depth[rng.random((h, w)) < 0.02] = np.inf
    depth[rng.random((h, w)) < 0.02] = 0
    hits = rng.integers(0, 4, (h, w)).astype(np.uint32)
    obj = rng.integers(0, 3, (h, w)).astype(np.uint32)
    obj[hits == 0] = 0xFFFFFFFF
    return rgb, dict(albedo=albedo, normal=normal, depth=depth, hits=hits, object=obj)


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (9, 10), (37, 21), (257, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_random_buffers_equal_the_restatement(gpu, size, flags):
    """L = 0 .. 6, k in {0, 3, 7}, sigma from 1e-6 to 1e6"""
    import torch
    w, h = size
    rng = np.random.default_rng(w * 7919 + h * 31 + flags)
    rgb, aov = _random_inputs(w, h, rng)
    d_rgb, d_aov = torch.from_numpy(rgb).cuda(), _to_dev(aov)
    for L in range(7):
        k = (0, 3, 7)[L % 3]
        sc, sz = ((0.5, 1.0), (1e-6, 1e6), (1e6, 1e-6), (2.0, 0.25))[L % 4]
        kw = _kw(flags, iterations=L, normal_power_log2=k, sigma_color=sc, sigma_depth=sz)
        out, out8 = gpu.denoise(d_rgb, d_aov, w, h, **kw)
        torch.cuda.synchronize()
        _check(out, out8, denoise_aov(rgb, aov, **_expected_kw(kw)), f"{w}x{h} flags {flags} L {L} k {k} sigma {sc} {sz}")


def test_full_hd_random_buffers(gpu):
    import torch
    w, h = 1920, 1080
    rgb, aov = _random_inputs(w, h, np.random.default_rng(1080))
    kw = _kw(3, iterations=5)
    out, out8 = gpu.denoise(torch.from_numpy(rgb).cuda(), _to_dev(aov), w, h, **kw)
    torch.cuda.synchronize()
    _check(out, out8, denoise_aov(rgb, aov, **_expected_kw(kw)), "1920x1080")


def _frame(gs, samples, seed=SEED):
    image, _, _ = gs.render_image(seed, samples)
    return image.cpu().numpy(), gs.aov_image(seed, samples)


@pytest.mark.parametrize("what", ["config4", "mesh_checker"])
def test_real_frames_equal_the_restatement(gpu, what):
    """colour from render_tiles, first-hit buffers from render_aov of the same seed and samples"""
    from rt_amd import scene as S
    from util import class_scene
    sc = S.build_scene(4, 96, 54, 8) if what == "config4" else class_scene(n_packed=4, tris=40, mesh_chk=True, width=64, height=40)
    gs = gpu.GpuScene(sc)
    rgb, aov = _frame(gs, 8)
    for flags in (1, 3):
        for L in (1, 5):
            kw = _kw(flags, iterations=L)
            noisy, den, den8 = gs.denoised_image(SEED, 8, **kw)
            assert same_floats(noisy, rgb)
            _check(den, den8, denoise_aov(rgb, aov, **_expected_kw(kw)), f"{what} flags {flags} L {L}")
    gs.close()
    sc.free()


def test_progressive_preview_after_passes(gpu):
    """Accumulation.denoised after passes of 1, 3 and 16 samples: the denoise of the resolved mean with the first-hit buffers of
    the samples done"""
    import torch
    from rt_amd import scene as S
    sc = S.build_scene(4, 64, 40, 20)
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, 20)
    for n in (1, 3, 16):
        acc.add(n)
        rgb, rgb8 = acc.denoised()
        tiles, tiles8 = acc.resolve()
        image, _ = gs.untile(tiles, tiles8, 0, 1, gpu.n_tiles(64, 40))
        torch.cuda.synchronize()
        exp = denoise_aov(image.cpu().numpy(), gs.aov_image(SEED, acc.samples), **_expected_kw(_kw(1, iterations=5)))
        _check(rgb, rgb8, exp, f"after {acc.samples} samples")
    acc.close()
    part = gs.accumulate(SEED, 4, first=1, stride=2, count=3)
    part.add(4)
    with pytest.raises(ValueError):
        part.denoised()
    part.close()
    gs.close()
    sc.free()


def test_in_place_one_output_and_a_second_stream(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    w, h = 45, 30
    rgb, aov = _random_inputs(w, h, np.random.default_rng(3))
    kw = _kw(3, iterations=4)
    exp = denoise_aov(rgb, aov, **_expected_kw(kw))
    d_aov = _to_dev(aov)
    # in place
    d_rgb = torch.from_numpy(rgb).cuda()
    out, out8 = gpu.denoise(d_rgb, d_aov, w, h, out=d_rgb, **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == d_rgb.data_ptr()
    _check(d_rgb, out8, exp, "in place")
    # one output, then the other (NULL for the other)
    d_rgb = torch.from_numpy(rgb).cuda()
    a = abi.RtHipAov()
    for f, t in d_aov.items():
        setattr(a, f, t.data_ptr())
    p = abi.denoise_params(**kw)
    ws = torch.empty(shim.rt_hip_denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    o = torch.full((h, w, 3), 7.0, device="cuda")
    o8 = torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda")
    assert shim.rt_hip_denoise(d_rgb.data_ptr(), C.byref(a), w, h, C.byref(p), ws.data_ptr(), o.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    _check(o, None, exp, "rgb only")
    assert (o8 == 7).all()
    assert shim.rt_hip_denoise(d_rgb.data_ptr(), C.byref(a), w, h, C.byref(p), ws.data_ptr(), None, o8.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _check(exp, o8, exp, "bytes only")
    # a second stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, out8 = gpu.denoise(d_rgb, d_aov, w, h, **kw)
    s.synchronize()
    _check(out, out8, exp, "second stream")
    # a host pointer is refused, not launched on
    assert shim.rt_hip_denoise(rgb.ctypes.data, C.byref(a), w, h, C.byref(p), ws.data_ptr(), o.data_ptr(), None, None) == abi.EINVAL


# the quality bounds: the sweep in DESIGN ("Denoiser") measured the defaults at 320 x 180, 16 spp, against 1024 spp of another seed
QUALITY_BYTES, QUALITY_LINEAR = 0.25, 0.6   # measured 0.166x and 0.477x


def quality(noisy, noisy8, den, den8, ref, ref8):
    """(byte RMS, clipped linear RMS) of the noisy and the denoised frame against the reference"""
    rms = lambda a, b: float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))
    clip = lambda a: np.clip(np.nan_to_num(np.asarray(a, np.float64), nan=1.0), 0, 1)
    return (rms(noisy8, ref8), rms(clip(noisy), clip(ref))), (rms(den8, ref8), rms(clip(den), clip(ref)))


def test_quality_on_the_room(gpu):
    from rt_amd import scene as S
    sc = S.build_scene(4, 320, 180, 16)
    gs = gpu.GpuScene(sc)
    ref, ref8, _ = gs.render_image(SEED + 1, 1024)
    noisy, noisy8, _ = gs.render_image(SEED, 16)
    same, n, den8 = gs.denoised_image(SEED, 16)
    assert same_floats(same, noisy.cpu().numpy())
    (b0, l0), (b1, l1) = quality(noisy.cpu().numpy(), noisy8.cpu().numpy(), n, den8, ref.cpu().numpy(), ref8.cpu().numpy())
    print(f"\nbytes RMS {b0:.2f} -> {b1:.2f} LSB ({b1 / b0:.3f}x), clipped linear RMS {l0:.4f} -> {l1:.4f} ({l1 / l0:.3f}x)")
    assert b1 <= QUALITY_BYTES * b0 and l1 <= QUALITY_LINEAR * l0
    gs.close()
    sc.free()


def _read_png(path):
    """the project's PNG writer: one IDAT, filter 0 on every row"""
    data = open(path, "rb").read()
    pos, chunks = 8, {}
    while pos < len(data):
        (n,), typ = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        chunks[typ] = data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h = struct.unpack(">II", chunks[b"IHDR"][:8])
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), dtype=np.uint8).reshape(h, 1 + w * 3)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_host_library_and_cli_equal_the_python_path(gpu, tmp_path):
    from rt_amd import abi, scene as S
    w, h, spp = 48, 30, 4
    sc = S.build_scene(4, w, h, spp)
    gs = gpu.GpuScene(sc)
    noisy, den, den8 = gs.denoised_image(SEED, spp, iterations=3)
    aov = gs.aov_image(SEED, spp)
    host = abi.load_host()
    img = abi.RtAovImage()
    img.albedo, img.normal, img.depth = aov["albedo"].ctypes.data, aov["normal"].ctypes.data, aov["depth"].ctypes.data
    img.object_id, img.hits = aov["object"].ctypes.data, aov["hits"].ctypes.data
    p = abi.denoise_params(iterations=3)
    out, out8 = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.uint8)
    assert host.denoise_frame(out8.ctypes.data, out.ctypes.data, noisy.ctypes.data, C.byref(img), w, h, C.byref(p)) == 0
    assert same_floats(out, den) and np.array_equal(out8, den8)
    # in place, default parameters (NULL)
    buf = noisy.copy()
    assert host.denoise_frame(None, buf.ctypes.data, buf.ctypes.data, C.byref(img), w, h, None) == 0
    assert same_floats(buf, gs.denoised_image(SEED, spp)[1])
    cli = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")
    png = tmp_path / "frame.png"
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "-s", str(spp), "-d", str(sc.max_depth), "-c", "4", "-r", str(SEED),
                        "-o", str(png), "-n", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, noisy8_py, _ = gs.render_image(SEED, spp)
    assert np.array_equal(_read_png(tmp_path / "frame.noisy.png"), noisy8_py.cpu().numpy())
    assert np.array_equal(_read_png(png), den8)
    gs.close()
    sc.free()

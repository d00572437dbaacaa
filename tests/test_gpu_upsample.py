"""Guided upsampling on the GPU (rt_hip_upsample): rgb, conf and the bytes equal the numpy restatement of the contract
(tests/upsample_expected.py) BIT FOR BIT (NaN colours equal to NaN) -- on the edge inputs the restatement is pinned on, in every
call form, on real frames, at 1920 x 1080 from 960 x 540; Preview, the driver, equals the pipeline step by step; and the result
does what it is for: closer to the converged frame than plain bilinear of the same low frame."""
import ctypes as C

import numpy as np
import pytest

import upsample_expected as UE
from upsample_expected import PARAMS, SIZE_PAIRS, edge_case, mismatch, tonemap8, upsample

pytestmark = pytest.mark.gpu

SEED = 1666943821
FIELDS = ("albedo", "normal", "depth", "object", "hits")


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _dev_aov(aov):
    return {f: _dev(aov[f]) for f in FIELDS}


def _host_aov(aov):
    out = {f: t.cpu().numpy() for f, t in aov.items()}
    for f in ("object", "hits"):
        out[f] = out[f].view(np.uint32)
    return out


def _host(res):
    return {f: (t.cpu().numpy() if hasattr(t, "cpu") else t) for f, t in res.items() if f in ("rgb", "conf", "rgb8")}


def _check(got, exp, what):
    """floats against the restatement, bytes against the tonemap of the restatement's floats: all of it bit for bit"""
    got = _host(got)
    got.setdefault("conf", exp["conf"])          # (an output the call was not given)
    msg = mismatch(got, exp)
    assert not msg, f"{what}: {msg}"
    if "rgb8" in got:
        want8 = tonemap8(exp["rgb"])
        bad = np.argwhere(got["rgb8"] != want8)
        assert not len(bad), f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {got['rgb8'][tuple(bad[0])]} != {want8[tuple(bad[0])]}"


def _run(G, low_rgb, low_aov, aov, **p):
    import torch
    hl, wl = low_rgb.shape[:2]
    h, w = aov["depth"].shape
    res = G.upsample(_dev(low_rgb), _dev_aov(low_aov), wl, hl, _dev_aov(aov), w, h, **p)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=UE.pair_id)
def test_edge_inputs_equal_the_restatement(gpu, pair):
    """every parameter row of PARAMS (both flags in both states, k 0 and 10, sigma_depth 2^-40 and DBL_MAX) on the planted colours,
    albedos, normals, depths, hits and object ids: tests/test_upsample_cpu.py shows that they reach every branch"""
    low_rgb, low_aov, aov, _ = edge_case(pair, UE.case_seed(pair))
    for k in range(len(PARAMS)):
        _check(_run(gpu, low_rgb, low_aov, aov, **UE.params(k)), upsample(low_rgb, low_aov, aov, **UE.params(k)),
               f"{UE.pair_id(pair)} {UE.params(k)}")


def test_call_forms(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    pair = ((45, 30), (23, 14))
    (w, h), (wl, hl) = pair
    low_rgb, low_aov, aov, _ = edge_case(pair, 4530)
    p = UE.params(2)     # both flags
    exp = upsample(low_rgb, low_aov, aov, **p)
    d_low, d_laov, d_aov = _dev(low_rgb), _dev_aov(low_aov), _dev_aov(aov)
    pp = abi.upsample_params(**p)
    la, a = gpu._upsample_aov(d_laov, wl * hl, d_low.device, pp, "low"), gpu._upsample_aov(d_aov, w * h, d_low.device, pp, "full")
    # each optional output NULL, through the C-ABI
    for drop in ("rgb8", "conf", None):
        o = dict(rgb=torch.full((h, w, 3), 7.0, device="cuda"), conf=torch.full((h, w), 7.0, device="cuda"),
                 rgb8=torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda"))
        ptr = lambda f: None if f == drop else C.c_void_p(o[f].data_ptr())
        assert shim.rt_hip_upsample(d_low.data_ptr(), C.byref(la), wl, hl, C.byref(a), w, h, C.byref(pp), ptr("rgb"), ptr("rgb8"),
                                    ptr("conf"), None) == 0
        torch.cuda.synchronize()
        if drop:
            assert (o[drop] == 7).all()
        _check({f: t for f, t in o.items() if f != drop}, exp, f"without {drop}")
    res = gpu.upsample(d_low, d_laov, wl, hl, d_aov, w, h, out=dict(rgb8=None, conf=None), **p)   # ... and through gpu.upsample
    torch.cuda.synchronize()
    assert set(res) == {"rgb"}
    _check(res, exp, "without bytes and conf")
    # given output tensors are written in place
    res = gpu.upsample(d_low, d_laov, wl, hl, d_aov, w, h, out=dict(rgb=o["rgb"].zero_()), **p)
    torch.cuda.synchronize()
    assert res["rgb"].data_ptr() == o["rgb"].data_ptr()
    _check(res, exp, "given out")
    # a second stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = gpu.upsample(d_low, d_laov, wl, hl, d_aov, w, h, **p)
    s.synchronize()
    _check(res, exp, "second stream")
    # a host pointer is refused, not launched on; an output that is an input likewise
    assert shim.rt_hip_upsample(low_rgb.ctypes.data, C.byref(la), wl, hl, C.byref(a), w, h, C.byref(pp), o["rgb"].data_ptr(), None, None,
                                None) == abi.EINVAL
    with pytest.raises(gpu.ShimError):
        gpu.upsample(d_low, d_laov, wl, hl, d_aov, w, h, out=dict(conf=d_aov["depth"]), **p)
    # the host-array form, on the device and on a logical device of a (0, 0, 0) map
    _check(gpu.upsample_image_host(low_rgb, low_aov, aov, **p), exp, "image form")
    plain = dict(p, demodulate=False, object_edges=False)
    bare = lambda b: {f: b[f] for f in ("normal", "depth", "hits")}
    _check(gpu.upsample_image_host(low_rgb, bare(low_aov), bare(aov), **plain), upsample(low_rgb, low_aov, aov, **plain), "image form, no flags")
    m = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(m, 3) == 0
    try:
        _check(gpu.upsample_image_host(low_rgb, low_aov, aov, device=2, **p), exp, "logical device 2 of (0, 0, 0)")
        with pytest.raises(gpu.ShimError):
            gpu.upsample_image_host(low_rgb, low_aov, aov, device=3, **p)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0


def _render(gs, seed, spp, aov_samples):
    """the frame's linear mean and its first-hit buffers of `aov_samples` samples of the same seed, as numpy"""
    import torch
    from rt_amd import gpu as G
    total = G.n_tiles(gs.scene.width, gs.scene.height)
    tiles, tiles8, _ = gs.render_tiles(seed, 0, 1, total, samples=spp, chunks=gs.suggest_chunks(total, spp))
    image, _ = gs.untile(tiles, tiles8, 0, 1, total)
    aov = gs.untile_aov(gs.render_aov(seed, aov_samples, 0, 1, total), 0, 1, total)
    torch.cuda.synchronize()
    gs.launch_status()
    return image.cpu().numpy(), _host_aov(aov)


def _low_scene(G, gs, wl, hl):
    """the same objects and camera at another size, as Preview makes it"""
    import dataclasses
    return G.GpuScene(dataclasses.replace(gs.scene, width=wl, height=hl), device=gs.device)


@pytest.mark.parametrize("config, low, full", [(4, (96, 54), (192, 108)), (3, (40, 30), (120, 90))], ids=["room", "cube"])
def test_real_frames_equal_the_restatement(gpu, config, low, full):
    """4 spp for the low colour, first-hit buffers of S = 4 at both sizes; the defaults and both flags with k = 0"""
    from rt_amd import scene as S
    sc = S.build_scene(config, full[0], full[1], 4)
    gs = gpu.GpuScene(sc)
    lo = _low_scene(gpu, gs, *low)
    low_rgb, low_aov = _render(lo, SEED, 4, 4)
    _, aov = _render(gs, SEED, 1, 4)
    for p in (UE.DEFAULTS, dict(sigma_depth=0.2, normal_power_log2=0, demodulate=True, object_edges=True)):
        info = {}
        exp = upsample(low_rgb, low_aov, aov, info=info, **p)
        assert info["guided"] > 0.5 * full[0] * full[1] and info["accepted"] > 0 and info["hits"] + info["normal"] + info["object"] > 0, info
        _check(_run(gpu, low_rgb, low_aov, aov, **p), exp, f"config {config} {p}")
    lo.close()
    gs.close()
    sc.free()


def test_full_hd_frame(gpu):
    """config 4 at 1920 x 1080 from 960 x 540, 1 spp: the block and pixel arithmetic at the workload's size"""
    from rt_amd import scene as S
    sc = S.build_scene(4, 1920, 1080, 1)
    gs = gpu.GpuScene(sc)
    lo = _low_scene(gpu, gs, 960, 540)
    low_rgb, low_aov = _render(lo, SEED, 1, 1)
    _, aov = _render(gs, SEED, 1, 1)
    _check(_run(gpu, low_rgb, low_aov, aov), upsample(low_rgb, low_aov, aov, **UE.DEFAULTS), "1920x1080 from 960x540")
    lo.close()
    gs.close()
    sc.free()


@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoised"])
def test_preview_frame_equals_the_pipeline(gpu, denoise):
    """Preview.frame = render low (+ denoise) -> first-hit buffers at both sizes -> upsample, step by step; scale 3 of 100 x 55
    gives a low frame of 34 x 19 (ceil), whose aspect is not the full frame's"""
    import torch
    from rt_amd import scene as S
    w, h, spp = 100, 55, 4
    sc = S.build_scene(4, w, h, spp)
    gs = gpu.GpuScene(sc)
    pv = gs.preview(3, sigma_depth=0.1)
    assert (pv.low_width, pv.low_height) == (34, 19)
    res = pv.frame(SEED, spp, denoise=denoise, iterations=2)
    torch.cuda.synchronize()
    assert set(res) == {"rgb", "rgb8", "conf", "aov", "low"}
    low_rgb, low_aov = _render(pv.low, SEED, spp, spp)
    _, aov = _render(gs, SEED, 1, spp)
    assert UE.same_floats(res["low"]["noisy"].cpu().numpy(), low_rgb)
    for f in FIELDS:
        assert np.array_equal(_host_aov(res["aov"])[f].view(np.uint32), aov[f].view(np.uint32)), f
    if denoise:
        den, _ = gpu.denoise(_dev(low_rgb), _dev_aov(low_aov), 34, 19, iterations=2)
        low_rgb = den.cpu().numpy()
        assert not UE.same_floats(low_rgb, res["low"]["noisy"].cpu().numpy())
    assert UE.same_floats(res["low"]["rgb"].cpu().numpy(), low_rgb)
    _check(res, upsample(low_rgb, low_aov, aov, **dict(UE.DEFAULTS, sigma_depth=0.1)), f"Preview.frame, denoise={denoise}")
    pv.close()
    gs.close()
    sc.free()


# DESIGN, "`pt_upsample`", profiles/r09_upsample_bench.txt: (a) / (b) of test_guided_beats_plain_bilinear measured on an MI355X with
# this test's seed.  Over three seeds (SEED, SEED + 1, SEED + 2) it is 0.878, 0.912, 0.894: a spread of +-2 %, which the 15 % margin
# of the bar covers
GUIDED_RATIO = 0.878


def checkered_room(w, h, spp):
    """config 4's room with a checkered floor (M_CHECKERED on the floor's wall sphere, object 0)"""
    from rt_amd import abi, scene as S
    sc = S.build_scene(4, w, h, spp)
    sc.objects[0].flags |= abi.M_CHECKERED
    return sc


def test_guided_beats_plain_bilinear(gpu):
    """the checkered room: the low frame at 96 x 54 with 16 spp, upsampled to 192 x 108 under first-hit buffers of 16 samples,
    against R = 1024 spp at 192 x 108 of another seed, in clipped linear RMS: (a) guided with the defaults, (b) plain bilinear of the
    same low frame, (c) a 192 x 108 frame of 4 spp (the same number of path samples).  (a) < (b): the checker's edges and the
    silhouettes exist at full resolution in (a) only.  (a) / (c) is printed, not asserted"""
    import torch
    w, h, wl, hl = 192, 108, 96, 54
    sc = checkered_room(w, h, 16)
    gs = gpu.GpuScene(sc)
    ref = gs.render_image(SEED + 100, 1024)[0].cpu().numpy()
    pv = gs.preview(2)
    res = pv.frame(SEED, 16)
    torch.cuda.synchronize()
    low_rgb, low_aov, aov = res["low"]["rgb"].cpu().numpy(), _host_aov(res["low"]["aov"]), _host_aov(res["aov"])
    floor = aov["albedo"][(aov["object"] == 0) & (aov["hits"] == 16)]
    assert len(floor) and (floor.max(axis=0) - floor.min(axis=0) > 0.25).all(), "the floor shows no checker"
    a = UE.clip_rms(res["rgb"].cpu().numpy(), ref)
    b = UE.clip_rms(upsample(low_rgb, low_aov, aov, guided=False, demodulate=False)["rgb"], ref)
    c = UE.clip_rms(gs.render_image(SEED, 4)[0].cpu().numpy(), ref)
    print(f"\nclipped linear RMS against 1024 spp: guided {a:.4f}, plain bilinear {b:.4f}, 4 spp at full size {c:.4f}; "
          f"(a)/(b) {a / b:.3f}, (a)/(c) {a / c:.3f}; conf < 0.5 on {float((res['conf'] < 0.5).float().mean()):.4f} of the frame")
    assert a < b
    if GUIDED_RATIO is not None:
        assert a / b <= GUIDED_RATIO * 1.15
    pv.close()
    gs.close()
    sc.free()


def test_cli_preview_writes_both_frames(gpu, tmp_path):
    """the CLI's -u 3 of 100 x 55 with -n 2: the full-size PNG at -o and the 34 x 19 low frame next to it"""
    import os
    import struct
    import subprocess
    from rt_amd import abi
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    out = tmp_path / "frame.png"
    r = subprocess.run([cli, "-w", "100", "-h", "55", "-s", "4", "-u", "3", "-n", "2", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "100 x 55 (5500) pixels from 34 x 19" in r.stdout
    size = lambda path: struct.unpack(">II", open(path, "rb").read(24)[16:24])
    assert size(out) == (100, 55) and size(tmp_path / "frame.low.png") == (34, 19)

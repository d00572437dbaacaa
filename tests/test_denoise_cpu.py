"""The denoiser without a GPU: the numpy restatement of the contract (tests/denoise_expected.py) on hand-built cases whose answer is
known, and the C-ABI, host library and CLI entry points checked for their arguments and for failing loudly without a device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from denoise_expected import DEMODULATE, OBJECT_EDGES, denoise, same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")


def _flat(h, w, rgb=None, depth=1.0, hits=4, obj=0):
    """a flat, facing wall: normal (0, 0, 1), one depth, every pixel hit"""
    rng = np.random.default_rng(h * 1000 + w)
    c = rng.random((h, w, 3), dtype=np.float32) if rgb is None else np.asarray(rgb, np.float32)
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = 1
    return dict(rgb=c, albedo=np.full((h, w, 3), 0.5, np.float32), normal=n, depth=np.full((h, w), depth, np.float32),
                hits=np.full((h, w), hits, np.uint32), obj=np.full((h, w), obj, np.uint32))


def _run(b, **p):
    return denoise(b["rgb"], b["albedo"], b["normal"], b["depth"], b["hits"], b["obj"], **p)


def test_zero_iterations_is_the_identity():
    b = _flat(7, 9)
    assert same_floats(_run(b, iterations=0, flags=0), b["rgb"])
    assert same_floats(_run(b, iterations=0, flags=OBJECT_EDGES), b["rgb"])
    # with DEMODULATE the colour goes through c / (a + eps) and back: at most one rounding away
    np.testing.assert_allclose(_run(b, iterations=0, flags=DEMODULATE), b["rgb"], rtol=2.0 ** -23, atol=0)


def test_hand_computed_three_by_three():
    """one white pixel in the middle of black, a flat wall, sigma_color 1, k 0, one iteration (s = 1, S2 = 1): a neighbour q of
    different colour has dc = 3 and weight h5 h5 / 4; equal colours weigh h5 h5.  Worked by hand:
      centre: W = 9/64 + (49/64 - 9/64) / 4 = 19/64, A = 9/64           -> 9/19
      corner: W = 36/256 + 69/256 + 4/256 = 109/256, A = 4/256          -> 4/109
      edge (x 1, y 0): W = 36/256 + 94/256 + 6/256 = 136/256, A = 6/256 -> 3/68"""
    c = np.zeros((3, 3, 3), np.float32)
    c[1, 1] = 1.0
    out = _run(_flat(3, 3, c), iterations=1, sigma_color=1.0, normal_power_log2=0, flags=0)
    assert np.all(out[1, 1] == np.float32(9 / 19))
    assert np.all(out[1, 1] == np.float32(0.47368421))
    for y, x in ((0, 0), (0, 2), (2, 0), (2, 2)):
        assert np.all(out[y, x] == np.float32(4 / 109)) and abs(float(out[y, x, 0]) - 0.0366972) < 1e-7
    for y, x in ((0, 1), (1, 0), (1, 2), (2, 1)):
        assert np.all(out[y, x] == np.float32(3 / 68)) and abs(float(out[y, x, 0]) - 0.0441176) < 1e-7


def test_invalid_pixels_pass_through_and_are_never_neighbours():
    b = _flat(9, 11)
    b["rgb"][4, 5] = [np.nan, 0.5, 0.5]
    b["rgb"][0, 0] = [np.inf, 0.1, 0.1]
    b["rgb"][8, 10, 2] = -np.inf
    out = _run(b, iterations=3, flags=0)
    for y, x in ((4, 5), (0, 0), (8, 10)):
        assert same_floats(out[y, x], b["rgb"][y, x])
    assert np.isfinite(np.delete(out.reshape(-1, 3), [4 * 11 + 5, 0, 8 * 11 + 10], axis=0)).all()
    # the same image with other garbage in the invalid pixels' other channels: the valid pixels do not change
    b2 = {k: v.copy() for k, v in b.items()}
    b2["rgb"][4, 5] = [np.nan, 1e30, -7.0]
    out2 = _run(b2, iterations=3, flags=0)
    mask = np.isfinite(b["rgb"]).all(axis=2)
    assert same_floats(out2[mask], out[mask])


def test_edge_taps_are_dropped():
    """a 1 x 1 image: every tap but the centre lies outside, so the pixel keeps its colour; a 1 x 5 row: what a pixel sees does
    not depend on what lies beyond the image (a pixel's result equals the same pixels cut from a wider image's edge only if
    nothing outside is read -- the restatement never reads outside)"""
    b = _flat(1, 1)
    assert same_floats(_run(b, iterations=6, flags=0), b["rgb"])
    row = _flat(1, 5, np.float32([[[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]]]))
    out = _run(row, iterations=1, sigma_color=1.0, normal_power_log2=0, flags=0)
    # pixel 0: taps dx 0, 1, 2 of row dy 0 only; q = 1 differs (dc 3): w = (1/4 * 3/8) / 4; q = 2: w = 1/16 * 3/8
    W = 9 / 64 + (3 / 32) / 4 + 3 / 128
    assert np.all(out[0, 0] == np.float32(((3 / 32) / 4) / W))


def test_object_edges_keep_two_flat_objects_apart():
    b = _flat(8, 8)
    b["rgb"][:, :4] = 0.2
    b["rgb"][:, 4:] = 0.9
    b["obj"][:, 4:] = 7
    out = _run(b, iterations=5, sigma_color=1e6, flags=OBJECT_EDGES)
    assert same_floats(out[:, :4], b["rgb"][:, :4]) and same_floats(out[:, 4:], b["rgb"][:, 4:])
    mixed = _run(b, iterations=5, sigma_color=1e6, flags=0)
    assert (mixed[:, 3] > 0.25).all()   # without the flag they mix


def test_background_next_to_a_hit_is_never_mixed_in():
    b = _flat(6, 10)
    b["rgb"][:, 5:] = 10 / 255
    b["hits"][:, 5:] = 0
    b["depth"][:, 5:] = np.inf
    b["normal"][:, 5:] = 0
    out = _run(b, iterations=4, sigma_color=1e6, flags=0)
    assert same_floats(out[:, 5:], b["rgb"][:, 5:])       # background among background: equal colours stay
    left = _run({k: v[:, :5].copy() for k, v in b.items()}, iterations=4, sigma_color=1e6, flags=0)
    assert same_floats(out[:, :5], left)                   # the hits never see the background


def test_total_on_inconsistent_inputs():
    """NaN normals, finite depth with 0 hits, zero albedo, sigma at the extremes: defined, and deterministic"""
    rng = np.random.default_rng(5)
    b = _flat(9, 10)
    b["normal"][2, 3] = np.nan
    b["hits"] = rng.integers(0, 3, (9, 10)).astype(np.uint32)
    b["albedo"][4] = 0
    b["depth"][1] = 0
    for s in (1e-6, 1e6):
        a = _run(b, iterations=4, sigma_color=s, sigma_depth=s, flags=DEMODULATE | OBJECT_EDGES)
        assert same_floats(a, _run(b, iterations=4, sigma_color=s, sigma_depth=s, flags=DEMODULATE | OBJECT_EDGES))


# ---- the entry points without a device -------------------------------------------------------------------------------------

def _no_gpu():
    from rt_amd import abi
    return abi.load_shim().rt_hip_device_count() == 0


def _bufs(w=8, h=6):
    b = _flat(h, w)
    b["out"] = np.full((h, w, 3), 7.0, np.float32)
    b["out8"] = np.full((h, w, 3), 7, np.uint8)
    return b


def _aov(b, albedo=True, obj=True):
    from rt_amd import abi
    a = abi.RtHipAov()
    a.normal, a.depth, a.hits = b["normal"].ctypes.data, b["depth"].ctypes.data, b["hits"].ctypes.data
    if albedo:
        a.albedo = b["albedo"].ctypes.data
    if obj:
        a.object = b["obj"].ctypes.data
    return a


def test_defaults():
    from rt_amd import abi
    p = abi.denoise_params()
    assert (p.iterations, p.flags, p.normal_power_log2, p.sigma_color, p.sigma_depth) == (5, abi.DENOISE_DEMODULATE, 3, 0.5, 1.0)
    assert C.sizeof(abi.RtHipDenoiseParams) == 32
    q = abi.denoise_params(iterations=2, demodulate=False, object_edges=True)
    assert (q.iterations, q.flags) == (2, abi.DENOISE_OBJECT_EDGES)


def test_workspace_bytes():
    from rt_amd import abi
    shim = abi.load_shim()
    assert shim.rt_hip_denoise_workspace_bytes(1920, 1080) >= 56 * 1920 * 1080
    assert shim.rt_hip_denoise_workspace_bytes(0, 10) == 0 and shim.rt_hip_denoise_workspace_bytes(10, -1) == 0
    assert shim.rt_hip_denoise_workspace_bytes((1 << 20) + 1, 1) == 0
    assert shim.rt_hip_denoise_workspace_bytes(1 << 20, 1 << 12) == 0   # 2^32 pixels


def _bad_params():
    from rt_amd import abi
    out = []
    for f, v in (("iterations", -1), ("iterations", 11), ("normal_power_log2", 11), ("sigma_color", 0.0), ("sigma_color", -1.0),
                 ("sigma_color", math.inf), ("sigma_color", math.nan), ("sigma_depth", 0.0), ("sigma_depth", -0.5),
                 ("sigma_depth", math.inf), ("sigma_depth", math.nan), ("flags", 4)):
        p = abi.denoise_params()
        setattr(p, f, v)
        out.append((f"{f}={v}", p))
    return out


def test_bad_arguments_rejected():
    """EINVAL for every bad argument, before a device is looked for (the same on a machine with or without a GPU)"""
    from rt_amd import abi
    shim = abi.load_shim()
    b = _bufs()
    ws = np.zeros(shim.rt_hip_denoise_workspace_bytes(8, 6), np.uint8)
    good = abi.denoise_params(object_edges=True)
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(rgb=ptr(b["rgb"]), aov=None, w=8, h=6, p=good, work=ptr(ws), out=ptr(b["out"]), out8=ptr(b["out8"])):
        return shim.rt_hip_denoise(rgb, C.byref(aov if aov is not None else _aov(b)), w, h, C.byref(p) if p is not None else None,
                                   work, out, out8, None)

    def call_image(rgb=ptr(b["rgb"]), aov=None, w=8, h=6, p=good, out=ptr(b["out"]), out8=ptr(b["out8"])):
        return shim.rt_hip_denoise_image(rgb, C.byref(aov if aov is not None else _aov(b)), w, h,
                                         C.byref(p) if p is not None else None, 0, out, out8)

    for fn in (call, call_image):
        for w, h in ((0, 6), (8, 0), (-1, 6), ((1 << 20) + 1, 1), (1 << 20, 1 << 12)):
            assert fn(w=w, h=h) == abi.EINVAL, (fn.__name__, w, h)
        for what, p in _bad_params():
            assert fn(p=p) == abi.EINVAL, (fn.__name__, what)
        assert fn(p=None) == abi.EINVAL
        assert fn(rgb=None) == abi.EINVAL
        assert fn(out=None, out8=None) == abi.EINVAL
        for f in ("normal", "depth", "hits"):
            a = _aov(b)
            setattr(a, f, None)
            assert fn(aov=a) == abi.EINVAL, (fn.__name__, f)
        assert fn(aov=_aov(b, albedo=False)) == abi.EINVAL                             # DEMODULATE needs the albedo
        assert fn(aov=_aov(b, obj=False)) == abi.EINVAL                                # OBJECT_EDGES needs the object ids
    assert call(work=None) == abi.EINVAL
    assert shim.rt_hip_denoise(ptr(b["rgb"]), None, 8, 6, C.byref(good), ptr(ws), ptr(b["out"]), None, None) == abi.EINVAL
    assert (b["out"] == 7.0).all() and (b["out8"] == 7).all()


def test_no_device_is_an_error_not_a_fallback():
    from rt_amd import abi
    if not _no_gpu():
        pytest.skip("a GPU is visible")
    shim = abi.load_shim()
    b = _bufs()
    ws = np.zeros(shim.rt_hip_denoise_workspace_bytes(8, 6), np.uint8)
    p = abi.denoise_params(object_edges=True)
    assert shim.rt_hip_denoise(b["rgb"].ctypes.data, C.byref(_aov(b)), 8, 6, C.byref(p), ws.ctypes.data, b["out"].ctypes.data, None,
                               None) == abi.ENODEV
    assert b"no HIP device" in shim.rt_hip_last_error()
    assert shim.rt_hip_denoise_image(b["rgb"].ctypes.data, C.byref(_aov(b)), 8, 6, C.byref(p), 0, b["out"].ctypes.data,
                                     b["out8"].ctypes.data) == abi.ENODEV
    host = abi.load_host()
    img = abi.RtAovImage()
    img.albedo, img.normal, img.depth = b["albedo"].ctypes.data, b["normal"].ctypes.data, b["depth"].ctypes.data
    img.object_id, img.hits = b["obj"].ctypes.data, b["hits"].ctypes.data
    assert host.denoise_frame(b["out8"].ctypes.data, b["out"].ctypes.data, b["rgb"].ctypes.data, C.byref(img), 8, 6, None) == abi.ENODEV
    assert host.denoise_frame(b["out8"].ctypes.data, None, b["rgb"].ctypes.data, None, 8, 6, None) == abi.EINVAL
    assert (b["out"] == 7.0).all() and (b["out8"] == 7).all()


def test_cli_denoise_without_gpu_exits_loudly(tmp_path):
    if not _no_gpu():
        pytest.skip("a GPU is visible")
    r = subprocess.run([CLI, "-w", "16", "-h", "12", "-s", "2", "-c", "1", "-o", str(tmp_path / "f.png"), "-n", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert not list(tmp_path.glob("*.png"))


def test_cli_lists_the_flag_and_rejects_bad_values(tmp_path):
    r = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-n <denoise iterations" in r.stderr
    for bad in ("11", "-1", "x"):
        r = subprocess.run([CLI, "-w", "16", "-h", "12", "-s", "1", "-o", str(tmp_path / "f.png"), "-n", bad], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stderr, bad
        assert not list(tmp_path.glob("*.png"))

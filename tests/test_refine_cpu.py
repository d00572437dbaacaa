"""The pixel refinement without a GPU: the numpy restatements of the select and of the blend (tests/refine_expected.py) equal
their scalar loops on inputs that reach every branch; expected_pixels is the oracle's trace_sample under the contract's reduction;
the C-ABI refuses bad arguments before it looks for a device; and the end-to-end GPU test's input is meaningful -- on the oracle's
first-hit buffers the upsampling restatement leaves at least one pixel and at most a quarter of the frame at conf <= 0."""
import ctypes as C

import numpy as np
import pytest

import aov_expected as A
import refine_expected as R
import trace_expected as T
import upsample_expected as UE

SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 0.5, 2.0 ** -149, -(2.0 ** -149), R.FLT_MAX, -R.FLT_MAX], dtype=np.float32)
BOUNDS = [(0.0, 1.0), (-np.inf, 0.0), (0.0, np.inf), (-np.inf, np.inf), (1.0, 0.0), (0.5, 0.5), (-0.0, 0.0), (2.0 ** -150, 1.0),
          (-1e300, 1e300)]


def test_select_restatement_equals_the_scalar_loop():
    rng = np.random.default_rng(1)
    values = np.concatenate([SPECIAL, rng.uniform(-2, 2, 200).astype(np.float32)]).reshape(4, 53)
    seen = set()
    for lo, hi in BOUNDS:
        for invert in (False, True):
            a, b = R.select(values, lo, hi, invert), R.select_scalar(values, lo, hi, invert)
            assert a.shape == values.shape and (a == b).all(), (lo, hi, invert)
            seen.add(int(a.sum()))
            nan = np.isnan(values)
            assert (a[nan] == invert).all()                                  # a NaN value: under INVERT only
    assert 0 in seen and values.size in seen                                  # lo > hi: nothing, everything under INVERT
    zero = np.array([0.0, -0.0], dtype=np.float32)
    assert R.select(zero, 0.0, 0.0).all() and R.select(zero, -0.0, -0.0).all()   # -0.0 equals 0.0
    idx, count = R.selected(values, 0.0, 1.0)
    assert count == len(idx) and (np.diff(idx.astype(np.int64)) > 0).all() and idx.dtype == np.uint32


def test_blend_restatement_equals_the_scalar_loop():
    for seed, (nw, ps, with_prior) in enumerate([(4.0, 0.0, True), (4.0, 4.0, True), (16.0, 1.0, False), (1.0, 2.0 ** 100, True),
                                                 (3.0, np.inf, True), (2.0, 0.0, False)]):
        case = R.blend_case(seed)
        prior = case["prior"] if with_prior else None
        a = R.blend(case["pixels"], case["status"], case["radiance"], case["rgb"], nw, ps, prior)
        b = R.blend_scalar(case["pixels"], case["status"], case["radiance"], case["rgb"], nw, ps, prior)
        assert (a["touched"] == b["touched"]).all()
        assert UE.same_floats(a["rgb"], b["rgb"]) and UE.same_floats(a["weight"], b["weight"]), (nw, ps)
        t = a["touched"]
        assert 40 <= t.sum() <= 60 - 7                  # status 2 and 0, three non-finite radiances, two indices out of range
        assert (a["rgb"].reshape(-1, 3)[~t].view(np.uint32) == case["rgb"].reshape(-1, 3)[~t].view(np.uint32)).all()
        if ps == 0.0:
            assert (a["weight"][t] == np.float32(nw)).all()      # replacement everywhere
        if (nw, ps) == (4.0, 4.0):
            w = a["weight"][t].astype(np.float64)
            assert (w == 4.0).sum() >= 7 and (w > 4.0).sum() >= 30   # both branches


def test_expected_pixels_is_trace_sample_under_the_reduction(pt):
    from rt_amd import scene as S
    sc = S.build_scene(1, 16, 12, 1, 4)
    pixels = R.pixel_list(16, 12)
    assert len(pixels) == 39 and pixels.max() == 0xFFFFFFFF and (pixels == 16 * 12).sum() == 1
    exp = R.expected_pixels(pt, sc, pixels, 5, 3, R.SEED)
    assert exp["status"].tolist().count(2) == 2 and (exp["samples"][exp["status"] == 2] == 0).all()
    i = 6                                                       # an entry of the descending run
    p = int(pixels[i])
    for k in range(5):
        rgb, st = pt.trace_sample(sc, p % 16, p // 16, 3 + k, R.SEED)
        assert (exp["samples"][i, k] == rgb).all()
    assert (exp["radiance"].view(np.uint64) == T.reduce_samples_scalar(exp["samples"]).view(np.uint64)).all()
    dup = np.flatnonzero(pixels == pixels[4])
    assert len(dup) == 2 and (exp["samples"][dup[0]] == exp["samples"][dup[1]]).all()
    sc.free()


def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    from rt_amd import abi
    shim = abi.load_shim()
    one = C.c_void_p(16)                                       # (never dereferenced: the checks come first)
    nan = float("nan")
    assert shim.rt_hip_select_workspace_bytes(0, 4) == 0 and shim.rt_hip_select_workspace_bytes(4, (1 << 20) + 1) == 0
    assert shim.rt_hip_select_workspace_bytes(1 << 16, 1 << 16) == 0
    assert shim.rt_hip_select_workspace_bytes(1, 1) == 256
    # 2^32 - 1 pixels: 2^24 counts, 2^14 sums, 16 sums of sums, one total, each level on a 256-byte boundary
    assert shim.rt_hip_select_workspace_bytes(65537, 65535) == 4 * (2 ** 24 + 2 ** 14) + 256 + 256
    for args in [(None, 4, 4, 0.0, 1.0, 0, one, one, 16, one), (one, 0, 4, 0.0, 1.0, 0, one, one, 16, one),
                 (one, 4, 4, nan, 1.0, 0, one, one, 16, one), (one, 4, 4, 0.0, nan, 0, one, one, 16, one),
                 (one, 4, 4, 0.0, 1.0, 2, one, one, 16, one), (one, 4, 4, 0.0, 1.0, 0, None, one, 16, one),
                 (one, 4, 4, 0.0, 1.0, 0, one, None, 16, one), (one, 4, 4, 0.0, 1.0, 0, one, one, 16, None)]:
        assert shim.rt_hip_select_pixels(*args, None) == abi.EINVAL, args
    cam = abi.Camera()
    rad = abi.RtHipRadiance()
    rad.status = 16

    def params(**kw):
        p = abi.pixel_params(8, 8, 1, 0)
        for f, v in kw.items():
            setattr(p, f, v)
        return p
    bad = [params(width=1), params(height=(1 << 20) + 1), params(samples=0), params(sample_first=-1),
           params(samples=2 ** 30, sample_first=2 ** 30 + 1), params(max_depth=-1), params(integrator=abi.CAST_RAY)]
    for p in bad:
        assert shim.rt_hip_trace_pixels(one, C.byref(cam), one, 4, C.byref(p), C.byref(rad), None, None) == abi.EINVAL
    ok = params()
    assert shim.rt_hip_trace_pixels(one, None, one, 4, C.byref(ok), C.byref(rad), None, None) == abi.EINVAL        # no camera
    assert shim.rt_hip_trace_pixels(one, C.byref(cam), None, 4, C.byref(ok), C.byref(rad), None, None) == abi.EINVAL
    assert shim.rt_hip_trace_pixels(None, C.byref(cam), one, 4, C.byref(ok), C.byref(rad), None, None) == abi.EINVAL     # no scene
    assert shim.rt_hip_trace_pixels(one, C.byref(cam), one, 4, C.byref(ok), C.byref(abi.RtHipRadiance()), None, None) == abi.EINVAL
    with_ray = abi.RtHipRadiance()
    with_ray.status, with_ray.ray = 16, 16
    assert shim.rt_hip_trace_pixels(one, C.byref(cam), one, 4, C.byref(ok), C.byref(with_ray), None, None) == abi.EINVAL
    assert shim.rt_hip_trace_pixels(one, C.byref(cam), one, 2 ** 32, C.byref(ok), C.byref(rad), None, None) == abi.EINVAL
    # the order of the host form's steps: the arguments, then nothing to do for no entry, then the device (99: there is none such)
    sc = R.checkered_room(8, 8, 1)
    idx = np.zeros(4, np.uint32)
    status = np.zeros(4, np.uint32)
    rad.status = status.ctypes.data

    def host_form(n, p, device):
        return shim.rt_hip_trace_pixels_host(sc.objects, sc.n_objects, None, 0, C.byref(cam), idx.ctypes.data, n, C.byref(p), device,
                                             C.byref(rad), None)
    for device in (0, 99):
        assert host_form(4, bad[0], device) == abi.EINVAL
        assert host_form(0, bad[0], device) == abi.EINVAL
        assert host_form(0, ok, device) == 0
    assert host_form(4, ok, 99) == abi.ENODEV
    assert host_form(4, ok, 0) == (abi.ENODEV if shim.rt_hip_device_count() == 0 else 0)
    rad.status = 16
    sc.free()
    for args in [(one, one, one, 4, 0, 4, 1.0, 0.0, None, one, None, None), (one, one, one, 4, 4, 4, 0.0, 0.0, None, one, None, None),
                 (one, one, one, 4, 4, 4, float("inf"), 0.0, None, one, None, None), (one, one, one, 4, 4, 4, 1.0, -1.0, None, one, None, None),
                 (one, one, one, 4, 4, 4, 1.0, nan, None, one, None, None), (one, one, one, 4, 4, 4, 1.0, 0.0, None, None, None, None),
                 (None, one, one, 4, 4, 4, 1.0, 0.0, None, one, None, None), (one, None, one, 4, 4, 4, 1.0, 0.0, None, one, None, None),
                 (one, one, None, 4, 4, 4, 1.0, 0.0, None, one, None, None), (one, one, one, 2 ** 32, 4, 4, 1.0, 0.0, None, one, None, None)]:
        assert shim.rt_hip_blend_pixels(*args, None) == abi.EINVAL, args
    names = [shim.rt_hip_pixel_kernel_launches(k, None).decode() for k in range(shim.rt_hip_pixel_kernel_count())]
    assert names == ["pt_trace_pixels", "pt_trace_pixels_big", "pt_trace_pixels_tri", "pt_trace_pixels_tri_big", "pt_trace_pixels_mem"]
    assert shim.rt_hip_pixel_kernel_launches(5, None) is None
    family = [shim.rt_hip_kernel_launches(k, None).decode() for k in range(shim.rt_hip_kernel_count())]
    assert not set(names) & set(family)                        # not members of the family


def test_the_end_to_end_input_is_meaningful(pt):
    """the checkered room at 48 x 32 from 24 x 16, 4 spp, OBJECT_EDGES: over the oracle's first-hit buffers of both sizes and the oracle's low
    frame, the restatement's conf <= 0 selects at least one pixel and at most a quarter of the frame"""
    (w, h), (wl, hl) = R.FULL, R.LOW
    assert (wl, hl) == (-(-w // R.SCALE), -(-h // R.SCALE))
    sc = R.checkered_room(w, h, R.E2E_SPP)
    lo = R.low_scene(sc, wl, hl)
    aov = A.expected_image(pt, sc, R.E2E_SEED, R.E2E_SPP)
    low_aov = A.expected_image(pt, lo, R.E2E_SEED, R.E2E_SPP)
    mean, _, _ = pt.render_pixels(lo, R.E2E_SEED, spp=R.E2E_SPP, want_rgb8=False)
    low_rgb = mean.reshape(hl, wl, 3).astype(np.float32)
    exp = UE.upsample(low_rgb, low_aov, aov, **dict(UE.DEFAULTS, **R.E2E_PARAMS))
    idx, count = R.selected(exp["conf"], -np.inf, 0.0)
    print(f"conf <= 0 on {count} of {w * h} pixels; conf == -1 on {(exp['conf'] == -1).sum()}")
    assert 1 <= count <= w * h // 4
    sc.free()

"""Temporal reprojection without a GPU: the numpy restatement of the contract (tests/reproject_expected.py) against a scalar one
on the edge inputs the GPU test runs, its ray against the compiled reference's get_camera_ray, what identical cameras must give,
the C-ABI's argument checks, and that the real-frame pairs of the GPU test exercise every way a pixel can lose its history."""
import ctypes as C
import math

import numpy as np
import pytest

import reproject_expected as RE
from reproject_expected import (CAMERAS, PARAMS, PLANTED, REAL_PAIRS, REAL_SEEDS, REAL_SIZE, REAL_SPP, REASONS, SIZES, edge_case, mismatch,
                                reproject, scalar_reproject)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_restatement_equals_the_scalar_one_at_the_edges(size):
    w, h = size
    for kind in CAMERAS:
        rgb, aov, cam, hist, planted = edge_case(w, h, kind, seed=RE.case_seed(w, h, kind))
        if w * h >= 2 * len(PLANTED):
            assert all(len(planted[c]) for c in PLANTED)
        for k in [k for kd, k in RE.CASES if kd == kind]:
            info = {}
            vec = reproject(rgb, aov, cam, hist, info=info, **RE.params(k))
            with np.errstate(all="ignore"):
                sca = scalar_reproject(rgb, aov, cam, hist, **RE.params(k))
            assert not mismatch(vec, sca), f"{w}x{h} {kind} params {RE.params(k)}: {mismatch(vec, sca)}"
            if kind in ("behind", "zero_horizontal", "nan_history", "nan_current"):
                assert not info["ok"].any(), kind
        first = reproject(rgb, aov, cam, None)
        assert not mismatch(first, scalar_reproject(rgb, aov, cam, None))
        zero = reproject(rgb, aov, cam, RE.zero_history(w, h))
        assert not mismatch(zero, first), "a zero-filled history is no history"


def test_every_parameter_set_decides_something_on_the_edge_inputs():
    """what the GPU test's runs exercise, counted with the restatement over all sizes: under the small and under the large move
    every parameter set of PARAMS has pixels that pass step 4 and pixels that blend, and the sets at the ends of the ranges do
    what they are there for -- max_history 1 and 2^20 cut lengths (2^20: where a len' of 2^24 was planted), depth_tol 0 rejects
    every tap on its depth (a float32 depth is not the fp64 distance) where DBL_MAX rejects only a NaN difference, normal_min -2 rejects fewer taps than 0.5 (only a NaN dot fails it), normal_min 2 rejects taps of
    unit normals and still blends where a normal of length 1e19 was planted"""
    keys = ("ok", "blended", "capped", "normal", "depth")
    for kind in ("small", "large"):
        count = {}
        for k in range(len(PARAMS)):
            tot = dict.fromkeys(keys, 0)
            at_cap = 0
            for w, h in SIZES:
                rgb, aov, cam, hist, _ = edge_case(w, h, kind, seed=RE.case_seed(w, h, kind))
                info = {}
                res = reproject(rgb, aov, cam, hist, info=info, **RE.params(k))
                for f in keys:
                    tot[f] += int(info[f].sum())
                at_cap += int((info["capped"] & (res["len"] == np.float32(PARAMS[k][0]))).sum())
            count[k] = tot
            print(f"\n{kind} {RE.params(k)}: " + ", ".join(f"{f} {tot[f]}" for f in keys))
            assert tot["ok"] > 0 and (tot["blended"] > 0) == (PARAMS[k][1] != 0.0), (kind, k, tot)
            assert at_cap == tot["capped"]
            if PARAMS[k][0] in (1.0, 2.0 ** 20):
                assert tot["capped"] > 0, (kind, k, tot)
        c = count
        assert c[1]["capped"] == c[1]["blended"]                                     # max_history 1: every blend is cut to 1
        assert c[3]["depth"] > c[4]["depth"] and c[3]["blended"] == 0 < c[4]["blended"]   # depth_tol 0 against DBL_MAX
        assert c[5]["normal"] < c[0]["normal"] and c[5]["blended"] > c[6]["blended"]  # normal_min -2 against 0.9 and 2
        assert c[6]["normal"] > c[0]["normal"] and c[6]["blended"] > 0               # normal_min 2: only the 1e19 normals pass


def test_scalar_restatement_on_a_hand_computed_pixel():
    """identical cameras, a 2 x 2 floor: every pixel reprojects onto itself (motion 0 to rounding); history 4 frames long of
    colour 1, the frame's colour 0 -> out = 1 + (0 - 1) / 5 = 0.8, len 5; with max_history 2 -> 0.5, len 2"""
    from oracle_py import PtOracle
    cam = RE.cam_array(PtOracle().init_camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), 2, 2))
    aov = RE.floor_frame(cam, 2, 2)
    assert (aov["hits"] > 0).all()
    hist = dict(rgb=np.ones((2, 2, 3), np.float32), len=np.full((2, 2), 4, np.float32), aov=aov, camera=cam)
    rgb = np.zeros((2, 2, 3), np.float32)
    for fn in (reproject, scalar_reproject):
        r = fn(rgb, aov, cam, hist, max_history=32.0, depth_tol=1e-6, normal_min=0.99)
        assert np.abs(r["motion"]).max() < 2.0 ** -30
        np.testing.assert_allclose(r["rgb"], 0.8, rtol=2.0 ** -22)
        np.testing.assert_allclose(r["len"], 5.0, rtol=2.0 ** -22)
        r = fn(rgb, aov, cam, hist, max_history=2.0, depth_tol=1e-6, normal_min=0.99)
        assert (r["rgb"] == 0.5).all() and (r["len"] == 2.0).all()
    assert RE.f32(1e39) == math.inf and RE.f32(2.0 ** -150) == 0.0 and math.isnan(RE._div(0.0, 0.0)) and RE._div(-1.0, 0.0) == -math.inf


def test_the_ray_is_the_compiled_reference_s(ref):
    """step 3's ray = get_camera_ray of the compiled reference, bit for bit: init_camera cameras and raw random ones"""
    r = ref(5)
    rng = np.random.default_rng(11)
    cams = [RE.cam_array(r.init_camera((0.0, 0.0, 50.0), (0.0, 0.0, 0.0), 37, 21)),
            RE.cam_array(r.init_camera((16.0, 9.0, 42.0), (0.0, 0.0, 0.0), 37, 21)),
            RE.cam_array(r.init_camera((-3.0, 7.5, 0.25), (1.0, -2.0, 9.0), 37, 21))] + [rng.normal(size=(4, 3)) * s for s in (1.0, 30.0, 1e-3)]
    for cam in cams:
        w, h = 37, 21
        u, v, d = RE.camera_ray_dirs(cam, w, h)
        c = RE.to_camera(cam)
        for y, x in [(0, 0), (h - 1, w - 1), (3, 17), (20, 1), (10, 36)] + [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(40)]:
            ray = r.camera_ray(c, float(u[y, x]), float(v[y, x]))
            assert np.array_equal(ray[:3], cam[0])
            assert np.array_equal(ray[3:].view(np.uint64), np.ascontiguousarray(d[y, x]).view(np.uint64)), (cam, x, y)


@pytest.fixture(scope="module")
def full_hd_floor():
    from oracle_py import PtOracle
    w, h = 1920, 1080
    cam = RE.cam_array(PtOracle().init_camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), w, h))
    return cam, RE.floor_frame(cam, w, h)


def test_identical_cameras_leave_every_pixel_where_it_is(full_hd_floor):
    """|motion| < 2^-30 pixel for every foreground pixel of a 1920 x 1080 frame: the Cramer solve's rounding measures 1.4e-12"""
    cam, aov = full_hd_floor
    h, w = aov["depth"].shape
    fg = aov["hits"] > 0
    assert fg.mean() > 0.5
    rgb = np.full((h, w, 3), 0.5, np.float32)
    hist = dict(rgb=rgb, len=np.ones((h, w), np.float32), aov=aov, camera=cam)
    r = reproject(rgb, aov, cam, hist)
    m = r["motion"][fg]
    assert np.isfinite(m).all()
    print(f"\nmax |motion| under identical cameras: {np.abs(m).max():.3g} pixel")
    assert np.abs(m).max() < 2.0 ** -30
    assert np.isnan(r["motion"][~fg]).all() and (r["len"][fg] == 2.0).all() and (r["len"][~fg] == 1.0).all()


def test_chained_frames_under_one_camera_give_the_mean():
    """K fixed images through K chained frames with max_history >= K: the running mean.  Every frame rounds the blend once (and
    the fetched history once): K * 2^-24 relative to the largest value the pixel takes, plus the taps' leakage -- under |motion| <
    2^-30 per axis at most 2 * 2^-30 of a pixel's weight lies on neighbours that differ by at most 2 * max|c|: K * 2^-28 * max|c|"""
    from oracle_py import PtOracle
    w, h, K = 48, 27, 8
    cam = RE.cam_array(PtOracle().init_camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), w, h))
    aov = RE.floor_frame(cam, w, h)
    fg = aov["hits"] > 0
    rng = np.random.default_rng(8)
    imgs = [(rng.random((h, w, 3)) * 4.0).astype(np.float32) for _ in range(K)]
    hist = None
    for k in range(K):
        r = reproject(imgs[k], aov, cam, hist, max_history=float(K), depth_tol=0.05, normal_min=0.9)
        hist = dict(rgb=r["rgb"], len=r["len"], aov=aov, camera=cam)
    stack = np.stack(imgs).astype(np.float64)
    mean, big = stack.mean(axis=0), np.abs(stack).max(axis=0)
    bound = K * 2.0 ** -24 * big + K * 2.0 ** -28 * float(np.abs(stack).max())
    err = np.abs(r["rgb"].astype(np.float64) - mean)
    assert (err[fg] <= bound[fg]).all(), float((err[fg] / bound[fg]).max())
    assert np.allclose(r["len"][fg], K, rtol=2.0 ** -22) and (r["len"][~fg] == 1.0).all()
    assert RE.same_floats(r["rgb"][~fg], imgs[-1][~fg])


# ---- the entry points without a device -------------------------------------------------------------------------------------

def _no_gpu():
    from rt_amd import abi
    return abi.load_shim().rt_hip_device_count() == 0


def test_defaults_and_struct_size():
    from rt_amd import abi
    assert C.sizeof(abi.RtHipReprojectParams) == 32
    p = abi.reproject_params()
    assert p.flags == 0 and p.max_history >= 1 and p.depth_tol >= 0 and math.isfinite(p.normal_min)
    assert (p.max_history, p.depth_tol, p.normal_min) == (RE.DEFAULTS["max_history"], RE.DEFAULTS["depth_tol"], RE.DEFAULTS["normal_min"])
    q = abi.reproject_params(max_history=4, depth_tol=0.5)
    assert (q.max_history, q.depth_tol, q.normal_min) == (4.0, 0.5, p.normal_min)


class _Args:
    """host arrays standing in for every argument (the checks come before the device is looked for, and never read them)"""

    def __init__(self, w=8, h=6):
        from rt_amd import abi
        self.w, self.h = w, h
        f = lambda *s: np.zeros(s, np.float32)
        u = lambda *s: np.zeros(s, np.uint32)
        self.keep = dict(rgb=f(h, w, 3), hrgb=f(h, w, 3), hlen=f(h, w), out=np.full((h, w, 3), 7.0, np.float32), out8=np.full((h, w, 3), 7, np.uint8),
                         olen=np.full((h, w), 7.0, np.float32), motion=np.full((h, w, 2), 7.0, np.float32))
        self.bufs = [dict(normal=f(h, w, 3), depth=f(h, w), hits=u(h, w), object=u(h, w)) for _ in range(2)]
        self.cam, self.hcam = abi.Camera(), abi.Camera()
        self.p = abi.reproject_params()

    def aov(self, k, drop=None):
        from rt_amd import abi
        a = abi.RtHipAov()
        for f, arr in self.bufs[k].items():
            if f != drop:
                setattr(a, f, arr.ctypes.data)
        return a

    def call(self, image, **over):
        from rt_amd import abi
        shim = abi.load_shim()
        k = self.keep
        ptr = lambda a: a.ctypes.data
        a = dict(rgb=ptr(k["rgb"]), aov=C.byref(self.aov(0)), cam=C.byref(self.cam), hrgb=ptr(k["hrgb"]), hlen=ptr(k["hlen"]),
                 haov=C.byref(self.aov(1)), hcam=C.byref(self.hcam), w=self.w, h=self.h, p=C.byref(self.p), out=ptr(k["out"]),
                 out8=ptr(k["out8"]), olen=ptr(k["olen"]), motion=ptr(k["motion"]))
        a.update(over)
        head = (a["rgb"], a["aov"], a["cam"], a["hrgb"], a["hlen"], a["haov"], a["hcam"], a["w"], a["h"], a["p"])
        tail = (a["out"], a["out8"], a["olen"], a["motion"])
        if image:
            return shim.rt_hip_reproject_image(*head, a.get("device", 0), *tail)
        return shim.rt_hip_reproject(*head, *tail, None)


def test_bad_arguments_rejected():
    """EINVAL for every bad argument, before a device is looked for (the same on a machine with or without a GPU)"""
    from rt_amd import abi
    A = _Args()
    ptr = lambda a: a.ctypes.data
    for image in (False, True):
        for w, h in ((1, 6), (8, 1), (0, 6), (8, -1), ((1 << 20) + 1, 2), (1 << 20, 1 << 12), (1 << 16, 1 << 16)):
            assert A.call(image, w=w, h=h) == abi.EINVAL, (image, w, h)
        for f, v in (("flags", 1), ("max_history", 0.5), ("max_history", math.nan), ("max_history", math.inf), ("max_history", -2.0),
                     ("depth_tol", -1e-9), ("depth_tol", math.nan), ("depth_tol", math.inf), ("normal_min", math.nan),
                     ("normal_min", math.inf)):
            p = abi.reproject_params()
            setattr(p, f, v)
            assert A.call(image, p=C.byref(p)) == abi.EINVAL, (image, f, v)
        for name in ("rgb", "aov", "cam", "p", "out", "olen"):
            assert A.call(image, **{name: None}) == abi.EINVAL, (image, name)
        for f in ("normal", "depth", "hits", "object"):
            assert A.call(image, aov=C.byref(A.aov(0, drop=f))) == abi.EINVAL, (image, f)
            assert A.call(image, haov=C.byref(A.aov(1, drop=f))) == abi.EINVAL, (image, "history", f)
        for name in ("hrgb", "hlen", "haov", "hcam"):       # the history comes whole or not at all
            assert A.call(image, **{name: None}) == abi.EINVAL, (image, name)
        k = A.keep
        hist_bufs = [k["hrgb"], k["hlen"]] + list(A.bufs[1].values())
        for name in ("out", "out8", "olen", "motion"):      # no output may alias the history
            for b in hist_bufs:
                assert A.call(image, **{name: ptr(b)}) == abi.EINVAL, (image, name)
        assert A.call(image, out=ptr(k["hrgb"]) + 12) == abi.EINVAL          # ... or overlap it
        for name in ("out8", "olen", "motion"):             # ... or a buffer of the frame, or another output
            for b in [k["rgb"]] + list(A.bufs[0].values()):
                assert A.call(image, **{name: ptr(b)}) == abi.EINVAL, (image, name)
        for b in A.bufs[0].values():
            assert A.call(image, out=ptr(b)) == abi.EINVAL
        assert A.call(image, out=ptr(k["rgb"]) + 12) == abi.EINVAL           # in place means the same address
        assert A.call(image, olen=ptr(k["out"])) == abi.EINVAL and A.call(image, motion=ptr(k["olen"])) == abi.EINVAL
        assert A.call(image, out8=ptr(k["motion"]) + 4) == abi.EINVAL
    # the image form checks its arguments before it looks its device up (99: there is none such)
    assert A.call(True, w=1, device=99) == abi.EINVAL and A.call(True, out=None, device=99) == abi.EINVAL
    assert A.call(True, device=99) == abi.ENODEV
    assert (k["out"] == 7.0).all() and (k["out8"] == 7).all() and (k["olen"] == 7.0).all() and (k["motion"] == 7.0).all()
    # what is allowed gets past the checks: on a machine without a GPU the answer is "no device", not "bad argument"
    if _no_gpu():
        for image in (False, True):
            assert A.call(image) == abi.ENODEV
            assert A.call(image, out=ptr(k["rgb"])) == abi.ENODEV             # in place
            assert A.call(image, out8=None, motion=None) == abi.ENODEV
            assert A.call(image, hrgb=None, hlen=None, haov=None, hcam=None) == abi.ENODEV
        assert b"no HIP device" in abi.load_shim().rt_hip_last_error()


def test_host_library_without_a_device():
    from rt_amd import abi
    host = abi.load_host()
    A = _Args()
    k = A.keep
    img = [abi.RtAovImage() for _ in range(2)]
    for i in range(2):
        img[i].normal, img[i].depth = A.bufs[i]["normal"].ctypes.data, A.bufs[i]["depth"].ctypes.data
        img[i].object_id, img[i].hits = A.bufs[i]["object"].ctypes.data, A.bufs[i]["hits"].ctypes.data
    args = lambda aov: (k["out8"].ctypes.data, k["out"].ctypes.data, k["olen"].ctypes.data, k["motion"].ctypes.data, k["rgb"].ctypes.data,
                        aov, C.byref(A.cam), k["hrgb"].ctypes.data, k["hlen"].ctypes.data, C.byref(img[1]), C.byref(A.hcam), 8, 6, None)
    assert host.reproject_frame(*args(None)) == abi.EINVAL
    if _no_gpu():
        assert host.reproject_frame(*args(C.byref(img[0]))) == abi.ENODEV
        assert (k["out"] == 7.0).all()


# ---- the real-frame pairs of the GPU test are not vacuous --------------------------------------------------------------------

@pytest.fixture(scope="module")
def real_pairs(ref_mesh):
    """per pair: the CPU first-hit buffers (tests/aov_expected.py) of the two cameras and the restatement's account of the step"""
    from aov_expected import expected_image
    from rt_amd import scene as S
    w, h = REAL_SIZE
    frames, out = {}, {}
    for name, (config, cur, prev) in REAL_PAIRS.items():
        sc = S.build_scene(config, w, h, REAL_SPP)
        cams = [S.make_camera(w, h, *cur), S.make_camera(w, h, *prev)]
        bufs = []
        for k in range(2):
            key = (config, (cur, prev)[k], REAL_SEEDS[k])
            if key not in frames:
                frames[key] = expected_image(ref_mesh(5), sc, REAL_SEEDS[k], REAL_SPP, camera=cams[k])
            bufs.append(frames[key])
        # colour stands in for the render (the account below does not depend on it beyond finiteness): the albedo
        hist = dict(rgb=RE.plant_history(bufs[1]["albedo"].copy()), len=np.ones((h, w), np.float32), aov=bufs[1], camera=cams[1])
        info = {}
        reproject(bufs[0]["albedo"], bufs[0], cams[0], hist, info=info, **RE.DEFAULTS)
        out[name] = (bufs[0], info)
        sc.free()
    return out


def test_real_pairs_accept_and_reject_for_every_reason(real_pairs):
    seen = {r: 0 for r in REASONS}
    for name, (aov, info) in real_pairs.items():
        fg = aov["hits"] > 0
        assert fg.sum() > 0.5 * fg.size, name
        took, lost = float((info["blended"] & fg).sum()) / fg.sum(), float((~info["blended"] & fg).sum()) / fg.sum()
        print(f"\n{name}: history accepted for {took:.3f} of the foreground, rejected for {lost:.3f}; "
              + ", ".join(f"{r} {int(info[r].sum())}" for r in REASONS))
        if name != "room_away":
            assert took >= 0.5, (name, took)
            assert lost >= 0.01, (name, lost)
        else:
            assert took == 0.0 and info["behind"].sum() == fg.sum()
        for r in REASONS:
            seen[r] += int(info[r].sum())
    assert all(seen[r] > 0 for r in REASONS), seen

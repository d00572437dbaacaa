"""The overlap rules of the image-space calls, on device memory: an output may overlap nothing the call reads and no other output,
but for the one in-place pair each operator names.  Every rule is pinned once -- the refusal by RT_HIP_EINVAL and the exact text of
rt_hip_last_error(), the allowed pair by a run that equals the out-of-place one bit for bit -- at an 8 x 8 frame and at n = 4
entries.  (The codes of many more placements, on host arrays and without a device: tests/test_reproject_cpu.py,
tests/test_upsample_cpu.py, tests/test_reproject_points_cpu.py.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W = H = 8
N = 4

FRAME = b"an output overlaps a buffer of the frame (only out_rgb == rgb is allowed)"
OUTPUTS = b"two outputs overlap"
HISTORY = b"an output aliases a history buffer"
POINTS = b"an output overlaps the previous points"
IN_PLACE = b"the output overlaps an input (only d_points == d_hits->point is allowed)"
INPUT = b"an output overlaps an input"


@pytest.fixture(scope="module")
def shim():
    import torch
    from rt_amd import abi
    s = abi.load_shim()
    assert s.rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return s


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _refused(shim, rc, text):
    from rt_amd import abi
    assert rc == abi.EINVAL and shim.rt_hip_last_error() == text, (rc, shim.rt_hip_last_error())


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


class _Reproject:
    """a frame, a history and every output of rt_hip_reproject_points, each a device buffer of its own"""

    def __init__(self):
        import torch
        from rt_amd import abi
        rng = np.random.default_rng(8)
        f = lambda *s: _dev(rng.random(s, dtype=np.float32))
        u = lambda *s: _dev(np.zeros(s, np.uint32))
        self.t = dict(rgb=f(H, W, 3), hrgb=f(H, W, 3), hlen=f(H, W), points=_dev(rng.random((H, W, 3))),
                      out=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), out8=torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
                      olen=torch.zeros((H, W), dtype=torch.float32, device="cuda"), motion=torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"))
        self.bufs = [dict(normal=f(H, W, 3), depth=f(H, W), hits=u(H, W), object=u(H, W)) for _ in range(2)]
        self.cam, self.hcam, self.p = abi.Camera(), abi.Camera(), abi.reproject_params()

    def aov(self, k):
        from rt_amd import abi
        a = abi.RtHipAov()
        for name, t in self.bufs[k].items():
            setattr(a, name, t.data_ptr())
        return a

    def call(self, shim, history=True, points=False, **over):
        a = {k: t.data_ptr() for k, t in self.t.items()}
        a.update(over)
        hist = (a["hrgb"], a["hlen"], C.byref(self.aov(1)), C.byref(self.hcam)) if history else (None, None, None, None)
        return shim.rt_hip_reproject_points(a["rgb"], C.byref(self.aov(0)), C.byref(self.cam), *hist, W, H, C.byref(self.p),
                                            a["points"] if points else None, a["out"], a["out8"], a["olen"], a["motion"], None)


def test_reproject(shim):
    R = _Reproject()
    at = lambda name, off=0: R.t[name].data_ptr() + off
    # in place: out_rgb == rgb (no history: the colour passes through, the length is 1)
    assert R.call(shim, history=False) == 0
    apart = [_bits(R.t[k]) for k in ("out", "out8", "olen", "motion")]
    rgb = _bits(R.t["rgb"])
    assert R.call(shim, history=False, out=at("rgb")) == 0
    assert [_bits(R.t[k]) for k in ("rgb", "out8", "olen", "motion")] == apart and apart[0] == rgb
    # an output inside a buffer of the frame, two outputs, an output inside a history buffer, an output inside the previous points
    _refused(shim, R.call(shim, olen=R.bufs[0]["depth"].data_ptr() + 4), FRAME)
    _refused(shim, R.call(shim, motion=at("out", 8)), OUTPUTS)
    _refused(shim, R.call(shim, out8=at("hrgb", 4)), HISTORY)
    _refused(shim, R.call(shim, points=True, olen=at("points", 8)), POINTS)
    assert R.call(shim, points=True) == 0            # the same buffers, each where it belongs
    assert _bits(R.t["rgb"]) == rgb


class _Hits:
    """n = 4 hits on triangle 0 of two, four spheres, and an output of their own each"""

    def __init__(self):
        import torch
        rng = np.random.default_rng(4)
        self.t = dict(status=_dev(np.ones(N, np.uint32)), prim=_dev(np.zeros(N, np.uint32)), object=_dev(np.zeros(N, np.uint32)),
                      bary=_dev(rng.uniform(0.1, 0.4, (N, 2))), point=_dev(rng.random((N, 3))), positions=_dev(rng.random((2, 3, 3))),
                      prev=_dev(rng.uniform(1, 2, (4, 4))), cur=_dev(rng.uniform(1, 2, (4, 4))),
                      out=torch.zeros((N, 3), dtype=torch.float64, device="cuda"))

    def call(self, shim, moved, out):
        from rt_amd import abi
        h = abi.RtHipHits()
        for name in ("status", "prim", "object", "bary", "point"):
            setattr(h, name, self.t[name].data_ptr())
        if moved:
            return shim.rt_hip_prev_points_moved(C.byref(h), N, self.t["positions"].data_ptr(), 2, self.t["prev"].data_ptr(),
                                                 self.t["cur"].data_ptr(), 4, out, None)
        return shim.rt_hip_prev_points(C.byref(h), N, self.t["positions"].data_ptr(), 2, out, None)


@pytest.mark.parametrize("moved", [False, True])
def test_prev_points(shim, moved):
    A = _Hits()
    assert A.call(shim, moved, A.t["out"].data_ptr()) == 0
    apart = _bits(A.t["out"])
    assert np.isfinite(np.frombuffer(apart, np.float64)).all()
    _refused(shim, A.call(shim, moved, A.t["bary"].data_ptr() + 16), IN_PLACE)
    if moved:
        _refused(shim, A.call(shim, moved, A.t["cur"].data_ptr() + 32), IN_PLACE)
    assert _bits(A.t["out"]) == apart
    # in place: d_points == d_hits->point
    assert A.call(shim, moved, A.t["point"].data_ptr()) == 0
    assert _bits(A.t["point"]) == apart


def test_upsample(shim):
    import torch
    from rt_amd import abi
    rng = np.random.default_rng(2)
    f = lambda *s: _dev(rng.random(s, dtype=np.float32))
    u = lambda *s: _dev(np.zeros(s, np.uint32))
    wl = hl = 4
    low = f(hl, wl, 3)
    bufs = [dict(albedo=f(y, x, 3), normal=f(y, x, 3), depth=f(y, x), hits=u(y, x), object=u(y, x)) for x, y in ((wl, hl), (W, H))]
    outs = dict(out=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), out8=torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
                conf=torch.zeros((H, W), dtype=torch.float32, device="cuda"))
    aov = [abi.RtHipAov(), abi.RtHipAov()]
    for k in range(2):
        for name, t in bufs[k].items():
            setattr(aov[k], name, t.data_ptr())
    p = abi.upsample_params()

    def call(**over):
        a = {k: t.data_ptr() for k, t in outs.items()}
        a.update(over)
        return shim.rt_hip_upsample(low.data_ptr(), C.byref(aov[0]), wl, hl, C.byref(aov[1]), W, H, C.byref(p), a["out"], a["out8"], a["conf"], None)
    assert call() == 0
    before = [_bits(t) for t in outs.values()] + [_bits(low)]
    _refused(shim, call(conf=low.data_ptr() + 4), INPUT)
    _refused(shim, call(out8=outs["out"].data_ptr() + 12), OUTPUTS)
    assert [_bits(t) for t in outs.values()] + [_bits(low)] == before

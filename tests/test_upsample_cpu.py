"""Guided upsampling without a GPU: the numpy restatement of the contract (tests/upsample_expected.py) against a scalar one on the
edge inputs the GPU test runs, what plain bilinear at equal sizes must give, that the edge inputs reach every branch of the
contract, and the C-ABI's argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import upsample_expected as UE
from upsample_expected import PARAMS, PIXEL_COUNTS, PLANTED, SIZE_PAIRS, TAP_COUNTS, edge_case, mismatch, scalar_upsample, upsample


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=UE.pair_id)
def test_vectorised_restatement_equals_the_scalar_one_at_the_edges(pair):
    low_rgb, low_aov, aov, planted = edge_case(pair, UE.case_seed(pair))
    (w, h), (wl, hl) = pair
    if min(w * h, wl * hl) * 0.4 >= len(PLANTED):
        assert all(planted[c] for c in PLANTED), planted
    for k in range(len(PARAMS)):
        vec = upsample(low_rgb, low_aov, aov, **UE.params(k))
        with np.errstate(all="ignore"):
            sca = scalar_upsample(low_rgb, low_aov, aov, **UE.params(k))
        assert not mismatch(vec, sca), f"{UE.pair_id(pair)} {UE.params(k)}: {mismatch(vec, sca)}"


def test_scalar_restatement_on_a_hand_computed_pixel():
    """4 x 4 from 2 x 2, one flat surface, no demodulation: every guide weight is 1 (n.n = 1, dz = 0), so the result is plain
    bilinear with conf 1.  Pixel x = 1: fx = (1.5 * 1) / 3 - 0.5 = 0, the low pixel 0 itself; x = 0: fx = -1/3, the only usable tap is
    low pixel 0 with weight 2/3 -- renormalised, the same value; x = 2 and 3 lie 1/3 and 2/3 of the way to low pixel 1"""
    flat = lambda w, h: dict(normal=np.tile(np.float32([0, 1, 0]), (h, w, 1)), depth=np.full((h, w), 5, np.float32),
                             hits=np.full((h, w), 4, np.uint32))
    low = np.zeros((2, 2, 3), np.float32)
    low[:, 1] = 3.0
    for fn in (upsample, scalar_upsample):
        r = fn(low, flat(2, 2), flat(4, 4), demodulate=False)
        assert (r["conf"] == 1.0).all()
        assert (r["rgb"][:, 0] == 0.0).all() and (r["rgb"][:, 1] == 0.0).all()
        np.testing.assert_allclose(r["rgb"][:, 2], 1.0, rtol=2.0 ** -22)      # fx = 2.5 / 3 - 0.5 = 1/3 of the way from 0 to 3
        np.testing.assert_allclose(r["rgb"][:, 3], 2.0, rtol=2.0 ** -22)      # fx = 3.5 / 3 - 0.5 = 2/3
        # the right half of the high frame sees another surface: its taps on the left low column are rejected
        hi = flat(4, 4)
        hi["normal"][:, 2:] = (1, 0, 0)
        lo = flat(2, 2)
        lo["normal"][:, 1] = (1, 0, 0)
        r = fn(low, lo, hi, demodulate=False)
        assert (r["rgb"][:, :2] == 0.0).all() and (r["rgb"][:, 2:] == 3.0).all()
        assert (r["conf"][:, :2] == 1.0).all()
        np.testing.assert_allclose(r["conf"][:, 2], 1.0 / 3.0, rtol=2.0 ** -22)
        np.testing.assert_allclose(r["conf"][:, 3], 2.0 / 3.0, rtol=2.0 ** -22)


@pytest.mark.parametrize("pair", [p for p in SIZE_PAIRS] + [((9, 8), (9, 8)), ((33, 31), (33, 31))], ids=UE.pair_id)
def test_plain_bilinear_at_equal_sizes_is_the_identity(pair):
    """with equal sizes fx is exactly x: the one tap of weight 1 is the pixel itself, and without guides and demodulation a finite
    pixel comes back bit for bit with conf 1 (but for a -0.0, which the sum from +0.0 turns into +0.0); a non-finite one has no
    usable tap"""
    size = pair[1]
    low_rgb, low_aov, _, _ = edge_case((size, size), UE.case_seed(pair))
    r = upsample(low_rgb, low_aov, low_aov, demodulate=False, guided=False)
    fin = np.isfinite(low_rgb).all(axis=2)
    assert fin.any()
    want = np.where(low_rgb == 0, np.float32(0.0), low_rgb)
    assert UE.same_bits(r["rgb"][fin], want[fin]) and (r["conf"][fin] == 1.0).all()
    assert (r["rgb"][~fin] == 0.0).all() and (r["conf"][~fin] == -1.0).all()


def test_edge_cases_reach_every_branch():
    """counted over all size pairs, per parameter row: taps accepted, taps that are not usable (non-finite), taps rejected by the
    hits, by the normal and by the depth, pixels blended, pixels on the fallback and pixels without a usable tap -- under every
    row; taps rejected by the object id under the rows with OBJECT_EDGES and none without.  sigma_depth = DBL_MAX accepts
    background pairs only (Zn overflows), but for a planted depth of 0 (D = 0: a tap of depth 0 too has Zd == 0)"""
    for k in range(len(PARAMS)):
        tot = dict.fromkeys(TAP_COUNTS + PIXEL_COUNTS, 0)
        for pair in SIZE_PAIRS:
            low_rgb, low_aov, aov, _ = edge_case(pair, UE.case_seed(pair))
            info = {}
            upsample(low_rgb, low_aov, aov, info=info, **UE.params(k))
            for f in tot:
                tot[f] += info[f]
        print(f"\n{UE.params(k)}: " + ", ".join(f"{f} {n}" for f, n in tot.items()))
        for f in tot:
            if f == "object":
                assert (tot[f] > 0) == PARAMS[k][3], (k, tot)
            else:
                assert tot[f] > 0, (k, f, tot)
    # DBL_MAX: whatever is accepted is a pair of background pixels (or of depths 0)
    k = [p[0] for p in PARAMS].index(UE.DBL_MAX)
    for pair in SIZE_PAIRS:
        low_rgb, low_aov, aov, _ = edge_case(pair, UE.case_seed(pair))
        r = upsample(low_rgb, low_aov, aov, **UE.params(k))
        assert not ((r["conf"] > 0) & (aov["hits"] > 0) & (aov["depth"] != 0)).any()
        assert ((r["conf"] == 0) & (aov["hits"] > 0)).any()                        # ... and the fallback carries the surfaces


# ---- the entry points without a device -------------------------------------------------------------------------------------

def _no_gpu():
    from rt_amd import abi
    return abi.load_shim().rt_hip_device_count() == 0


def test_defaults_and_struct_size():
    from rt_amd import abi
    assert C.sizeof(abi.RtHipUpsampleParams) == 16
    p = abi.upsample_params()
    assert p.flags == abi.UPSAMPLE_DEMODULATE
    assert (p.sigma_depth, p.normal_power_log2) == (UE.DEFAULTS["sigma_depth"], UE.DEFAULTS["normal_power_log2"])
    q = abi.upsample_params(sigma_depth=0.5, demodulate=False, object_edges=True)
    assert (q.sigma_depth, q.normal_power_log2, q.flags) == (0.5, p.normal_power_log2, abi.UPSAMPLE_OBJECT_EDGES)
    abi.load_shim().rt_hip_upsample_defaults(None)   # a NULL is ignored


class _Args:
    """host arrays standing in for every argument (the checks come before the device is looked for, and never read them)"""

    def __init__(self, w=8, h=6, wl=4, hl=3):
        from rt_amd import abi
        self.w, self.h, self.wl, self.hl = w, h, wl, hl
        f = lambda *s: np.zeros(s, np.float32)
        u = lambda *s: np.zeros(s, np.uint32)
        self.keep = dict(low=f(hl, wl, 3), out=np.full((h, w, 3), 7.0, np.float32), out8=np.full((h, w, 3), 7, np.uint8),
                         conf=np.full((h, w), 7.0, np.float32))
        self.bufs = [dict(albedo=f(y, x, 3), normal=f(y, x, 3), depth=f(y, x), hits=u(y, x), object=u(y, x)) for x, y in ((wl, hl), (w, h))]
        self.p = abi.upsample_params()

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
        a = dict(low=ptr(k["low"]), laov=C.byref(self.aov(0)), wl=self.wl, hl=self.hl, aov=C.byref(self.aov(1)), w=self.w, h=self.h,
                 p=C.byref(self.p), out=ptr(k["out"]), out8=ptr(k["out8"]), conf=ptr(k["conf"]))
        a.update(over)
        head = (a["low"], a["laov"], a["wl"], a["hl"], a["aov"], a["w"], a["h"], a["p"])
        tail = (a["out"], a["out8"], a["conf"])
        if image:
            return shim.rt_hip_upsample_image(*head, a.get("device", 0), *tail)
        return shim.rt_hip_upsample(*head, *tail, None)


def test_bad_arguments_rejected():
    """EINVAL for every bad argument, before a device is looked for (the same on a machine with or without a GPU)"""
    from rt_amd import abi
    A = _Args()
    ptr = lambda a: a.ctypes.data
    k = A.keep
    for image in (False, True):
        for bad in ((1, 6), (8, 1), (0, 6), (8, -1), ((1 << 20) + 1, 2), (1 << 20, 1 << 12), (1 << 16, 1 << 16)):
            assert A.call(image, w=bad[0], h=bad[1]) == abi.EINVAL, (image, bad)
            assert A.call(image, wl=bad[0], hl=bad[1]) == abi.EINVAL, (image, "low", bad)
        for f, v in (("flags", 4), ("flags", 0x80000001), ("normal_power_log2", 11), ("sigma_depth", 0.0), ("sigma_depth", -1.0),
                     ("sigma_depth", math.nan), ("sigma_depth", math.inf)):
            p = abi.upsample_params()
            setattr(p, f, v)
            assert A.call(image, p=C.byref(p)) == abi.EINVAL, (image, f, v)
        for name in ("low", "laov", "aov", "p", "out"):
            assert A.call(image, **{name: None}) == abi.EINVAL, (image, name)
        both = abi.upsample_params(demodulate=True, object_edges=True)
        for f in ("normal", "depth", "hits", "albedo", "object"):     # a guide the flags need, missing at either size
            assert A.call(image, p=C.byref(both), laov=C.byref(A.aov(0, drop=f))) == abi.EINVAL, (image, "low", f)
            assert A.call(image, p=C.byref(both), aov=C.byref(A.aov(1, drop=f))) == abi.EINVAL, (image, f)
        assert A.call(image, laov=C.byref(A.aov(0, drop="albedo"))) == abi.EINVAL            # the defaults demodulate
        inputs = [k["low"]] + [b for bufs in A.bufs for b in bufs.values()]
        for name in ("out", "out8", "conf"):                             # no output may overlap an input ...
            for b in inputs:
                assert A.call(image, p=C.byref(both), **{name: ptr(b)}) == abi.EINVAL, (image, name)
        assert A.call(image, out=ptr(k["low"]) + 12) == abi.EINVAL
        assert A.call(image, out8=ptr(k["out"])) == abi.EINVAL and A.call(image, conf=ptr(k["out"]) + 4) == abi.EINVAL   # ... or another
        assert A.call(image, conf=ptr(k["out8"])) == abi.EINVAL
    # the image form checks its arguments before it looks its device up (99: there is none such)
    assert A.call(True, w=1, device=99) == abi.EINVAL and A.call(True, out=None, device=99) == abi.EINVAL
    assert A.call(True, device=99) == abi.ENODEV
    assert (k["out"] == 7.0).all() and (k["out8"] == 7).all() and (k["conf"] == 7.0).all()
    # what is allowed gets past the checks: on a machine without a GPU the answer is "no device", not "bad argument"
    if _no_gpu():
        plain = abi.upsample_params(demodulate=False)
        for image in (False, True):
            assert A.call(image) == abi.ENODEV
            assert A.call(image, out8=None, conf=None) == abi.ENODEV
            assert A.call(image, wl=A.w, hl=A.h, laov=C.byref(A.aov(1)), low=ptr(np.zeros((A.h, A.w, 3), np.float32))) == abi.ENODEV
            # guides the flags do not need may be missing, and may be anything: an output may even be one of them
            assert A.call(image, p=C.byref(plain), laov=C.byref(A.aov(0, drop="albedo")), aov=C.byref(A.aov(1, drop="object"))) == abi.ENODEV
        assert b"no HIP device" in abi.load_shim().rt_hip_last_error()


def test_host_library_without_a_device():
    from rt_amd import abi
    host = abi.load_host()
    A = _Args()
    k = A.keep
    img = [abi.RtAovImage() for _ in range(2)]
    for i in range(2):
        img[i].albedo, img[i].normal, img[i].depth = (A.bufs[i][f].ctypes.data for f in ("albedo", "normal", "depth"))
        img[i].object_id, img[i].hits = A.bufs[i]["object"].ctypes.data, A.bufs[i]["hits"].ctypes.data
    args = lambda lo, hi, out: (k["out8"].ctypes.data, out, k["conf"].ctypes.data, k["low"].ctypes.data, lo, A.wl, A.hl, hi, A.w, A.h, None)
    assert host.upsample_frame(*args(None, C.byref(img[1]), k["out"].ctypes.data)) == abi.EINVAL
    assert host.upsample_frame(*args(C.byref(img[0]), None, k["out"].ctypes.data)) == abi.EINVAL
    if _no_gpu():
        assert host.upsample_frame(*args(C.byref(img[0]), C.byref(img[1]), k["out"].ctypes.data)) == abi.ENODEV
        assert host.upsample_frame(*args(C.byref(img[0]), C.byref(img[1]), None)) == abi.ENODEV      # linear_out may be NULL
        assert (k["out"] == 7.0).all()


def test_cli_rejects_what_does_not_go_with_a_preview(tmp_path):
    """-u with -g > 1, -e or -q ends with a message before anything is rendered; -u 1 is a usage error"""
    import os
    import subprocess
    from rt_amd import abi
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    base = [cli, "-w", "64", "-h", "36", "-s", "4", "-o", str(tmp_path / "x.png")]
    for extra in (["-g", "2"], ["-e", "0.1"], ["-q", "1,1"]):
        r = subprocess.run(base + ["-u", "2"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "-u renders a preview on one GPU" in r.stderr and "seed" not in r.stdout, (extra, r.stderr)
    r = subprocess.run(base + ["-u", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage:" in r.stderr
    assert not os.listdir(tmp_path)

"""The denoiser without a GPU: the numpy restatement of the contract (tests/denoise_expected.py) on hand-built cases whose answer is
known, and the C-ABI, host library and CLI entry points checked for their arguments and for failing loudly without a device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from denoise_expected import COLD, DEMODULATE, HOT, OBJECT_EDGES, _edge_inputs, denoise, same_floats

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


# ---- the vectorised restatement against a scalar one, at the edges of the accepted range -------------------------------------
# denoise() is the expectation of the GPU tests; its np.where / clamped-index forms are pinned above on ordinary values only.
# scalar_denoise follows include/rt_hip.h steps 1-4 line by line: Python floats are IEEE doubles (+, -, * never raise and never
# fuse; / goes through _div, Python's own raising on a zero divisor), f32() is each stored rounding.

def f32(x):
    """a double rounded to float32 (RNE; overflow to inf, denormals kept), widened back exactly"""
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def _div(a, b):
    """IEEE 754 a / b"""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def scalar_denoise(rgb, albedo, normal, depth, hits, obj, iterations=5, sigma_color=0.5, normal_power_log2=3, sigma_depth=1.0,
                   flags=DEMODULATE):
    h, w = depth.shape
    eps = 2.0 ** -10
    h5 = [1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16]
    c = [[[float(rgb[y, x, k]) for k in range(3)] for x in range(w)] for y in range(h)]
    # 1. a pixel is invalid if any channel of c is not finite
    valid = [[all(math.isfinite(v) for v in c[y][x]) for x in range(w)] for y in range(h)]
    # 2. e0 = float(c / (a + eps)) with DEMODULATE, else c
    if flags & DEMODULATE:
        a = [[[float(albedo[y, x, k]) + eps for k in range(3)] for x in range(w)] for y in range(h)]
        e = [[[f32(_div(c[y][x][k], a[y][x][k])) for k in range(3)] for x in range(w)] for y in range(h)]
    else:
        e = [[list(c[y][x]) for x in range(w)] for y in range(h)]
    n = [[[float(normal[y, x, k]) for k in range(3)] for x in range(w)] for y in range(h)]
    z = [[float(depth[y, x]) for x in range(w)] for y in range(h)]
    # 3. the iterations
    for i in range(iterations):
        s = 2 ** i
        sigma_i = sigma_color * 2.0 ** -i
        S2 = sigma_i * sigma_i
        nxt = [[list(e[y][x]) for x in range(w)] for y in range(h)]
        for y in range(h):
            for x in range(w):
                if not valid[y][x]:
                    continue
                W, A = 0.0, [0.0, 0.0, 0.0]
                ep = e[y][x]
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + s * dx, y + s * dy
                        if dx == 0 and dy == 0:
                            wt = 9.0 / 64.0
                        else:
                            if qx < 0 or qx >= w or qy < 0 or qy >= h or not valid[qy][qx]:
                                continue
                            if flags & OBJECT_EDGES and int(obj[qy, qx]) != int(obj[y, x]):
                                continue
                            hp, hq = int(hits[y, x]), int(hits[qy, qx])
                            if hp == 0 and hq == 0:
                                wn = Zn = Zd = 1.0
                            elif hp == 0 or hq == 0:
                                continue
                            else:
                                g = (n[y][x][0] * n[qy][qx][0] + n[y][x][1] * n[qy][qx][1]) + n[y][x][2] * n[qy][qx][2]
                                g = g if g > 0 else 0.0
                                wn = g
                                for _ in range(normal_power_log2):
                                    wn = wn * wn
                                D = (sigma_depth * z[y][x]) * float(s * max(abs(dx), abs(dy)))
                                Zn = D * D
                                dz = z[qy][qx] - z[y][x]
                                Zd = Zn + dz * dz
                                if Zd == 0:
                                    Zn = Zd = 1.0
                            de = [e[qy][qx][k] - ep[k] for k in range(3)]
                            dc = (de[0] * de[0] + de[1] * de[1]) + de[2] * de[2]
                            wt = _div(((h5[dx + 2] * h5[dy + 2]) * wn) * (S2 * Zn), (S2 + dc) * Zd)
                        W += wt
                        for k in range(3):
                            A[k] += wt * e[qy][qx][k]
                nxt[y][x] = [f32(_div(A[k], W)) for k in range(3)]
        e = nxt
    # 4. out = float(e_L * (a + eps)) with DEMODULATE, else e_L; invalid pixels pass c through
    out = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            for k in range(3):
                if not valid[y][x]:
                    out[y, x, k] = rgb[y, x, k]
                else:
                    out[y, x, k] = np.float32(f32(e[y][x][k] * a[y][x][k]) if flags & DEMODULATE else e[y][x][k])
    return out


def _both(rgb, aov, **p):
    vec = denoise(rgb, aov["albedo"], aov["normal"], aov["depth"], aov["hits"], aov["object"], **p)
    with np.errstate(all="ignore"):
        sca = scalar_denoise(rgb, aov["albedo"], aov["normal"], aov["depth"], aov["hits"], aov["object"], **p)
    return vec, sca


def test_scalar_restatement_gives_the_hand_computed_values():
    c = np.zeros((3, 3, 3), np.float32)
    c[1, 1] = 1.0
    b = _flat(3, 3, c)
    out = scalar_denoise(b["rgb"], b["albedo"], b["normal"], b["depth"], b["hits"], b["obj"], iterations=1, sigma_color=1.0,
                         normal_power_log2=0, flags=0)
    assert np.all(out[1, 1] == np.float32(9 / 19)) and np.all(out[0, 0] == np.float32(4 / 109)) and np.all(out[0, 1] == np.float32(3 / 68))
    assert f32(1e39) == math.inf and f32(2.0 ** -149) == 2.0 ** -149 and f32(2.0 ** -150) == 0.0 and f32(3 * 2.0 ** -150) == 2.0 ** -148
    assert math.copysign(1.0, f32(-1e-60)) == -1.0 and math.isnan(_div(0.0, 0.0)) and _div(-1.0, 0.0) == -math.inf == _div(1.0, -0.0)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("size", [(12, 9), (7, 5), (1, 11), (11, 1), (1, 1), (2, 40), (40, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_restatement_equals_the_scalar_one_at_the_edges(size, flags):
    """_edge_inputs with every hot value (hot_band = 1) and with none, L 0 .. 10, k 0 .. 10, sigmas up to the ends of the accepted
    range.  Without hot values and at k <= 3 most valid pixels stay finite, so that equality is not NaN == NaN alone"""
    w, h = size
    sig = ((0.5, 1.0), (1e-6, 1e6), (1e6, 1e-6), (float.fromhex("0x1.6a09e667f3bcdp-529"), 1.7976931348623157e308), (math.nextafter(2.0 ** 512, 0.0), 5e-324))
    for hot_band in (0.0, 1.0):
        rgb, aov, planted = _edge_inputs(w, h, np.random.default_rng(w * 100 + h + 7 * flags), hot_band=hot_band)
        if hot_band and w * h >= 100:
            assert all(len(planted[c]) for c in COLD + HOT)
        valid = np.isfinite(rgb).all(axis=2)
        for n, (L, k) in enumerate(((0, 3), (1, 0), (2, 3), (5, 3), (3, 10), (10, 2), (10, 10), (7, 8), (4, 1))):
            sc, sz = sig[n % len(sig)] if n >= 4 else (0.5, 1.0)
            vec, sca = _both(rgb, aov, iterations=L, normal_power_log2=k, sigma_color=sc, sigma_depth=sz, flags=flags)
            assert same_floats(vec, sca), f"{w}x{h} flags {flags} hot {hot_band} L {L} k {k} sigma {sc} {sz}: " \
                f"{int((vec.view(np.uint32) != sca.view(np.uint32)).sum())} words differ"
            assert np.array_equal(vec[~valid].view(np.uint32), rgb[~valid].view(np.uint32))
            if not hot_band and n < 4 and valid.sum() >= 20:
                assert np.isfinite(vec[valid]).all(axis=1).mean() > 0.5, f"{w}x{h} flags {flags} L {L}: mostly non-finite"


def test_edge_inputs_plant_what_they_say_and_the_nan_cap_holds():
    """every category in its share of the pixels, next to ordinary ones; and the condition the GPU test relies on: at 320 x 200
    with the hot values in the left eighth, at most half of the valid pixels are non-finite after five iterations, per flags"""
    w, h = 320, 200
    rgb, aov, planted = _edge_inputs(w, h, np.random.default_rng(99))
    n_cat = len(COLD) + len(HOT)
    for cat in COLD:
        assert abs(len(planted[cat]) - 0.4 * w * h / n_cat) <= 2, cat
    for cat in HOT:
        assert 0.06 * 0.4 * w * h / n_cat < len(planted[cat]) < 0.2 * 0.4 * w * h / n_cat, cat
        assert (planted[cat] % w < 40).all()
    every = np.concatenate(list(planted.values()))
    assert len(np.unique(every)) == len(every) and 0.3 < len(every) / (w * h) < 0.4
    flat = lambda a: a.reshape(w * h, -1)
    fmax = np.float32(np.finfo(np.float32).max)
    assert (flat(rgb)[planted["flt_max"]] == fmax).all() and (flat(rgb)[planted["neg_flt_max"]] == -fmax).any(axis=1).all()
    d = flat(rgb)[planted["denormal"]]
    assert (d > 0).all() and (d < np.finfo(np.float32).tiny).all()
    assert np.signbit(flat(rgb)[planted["neg_zero"]]).all() and (flat(rgb)[planted["neg_zero"]] == 0).all()
    assert (flat(rgb)[planted["negative"]] < 0).all()
    assert (flat(aov["albedo"])[planted["albedo_minus_eps"]][:, :2] == np.float32(-2.0 ** -10)).all()
    assert (flat(aov["albedo"])[planted["albedo_zero"]] == 0).all() and (flat(aov["albedo"])[planted["albedo_flt_max"]] == fmax).all()
    assert (flat(aov["depth"])[planted["depth_minus_inf"]] == -np.inf).all() and (flat(aov["depth"])[planted["depth_flt_max"]] == fmax).all()
    assert (flat(aov["depth"])[planted["hit_with_inf_depth"]] == np.inf).all() and (flat(aov["hits"])[planted["hit_with_inf_depth"]] > 0).all()
    assert (flat(aov["hits"])[planted["miss_with_depth"]] == 0).all() and np.isfinite(flat(aov["depth"])[planted["miss_with_depth"]]).all()
    assert (flat(aov["object"])[planted["no_object_id"]] == 0xFFFFFFFF).all() and (flat(aov["hits"])[planted["no_object_id"]] > 0).all()
    ln = lambda cat: np.linalg.norm(flat(aov["normal"])[planted[cat]].astype(np.float64), axis=1)
    assert (ln("normal_zero") == 0).all() and (ln("normal_1e19") > 0.9e19).all() and (ln("normal_1e-19") < 1.1e-19).all()
    valid = np.isfinite(rgb).all(axis=2)
    assert not valid.reshape(-1)[planted["invalid"]].any()
    for flags in range(4):
        out = denoise(rgb, aov["albedo"], aov["normal"], aov["depth"], aov["hits"], aov["object"], iterations=5, flags=flags)
        bad = float((~np.isfinite(out).all(axis=2) & valid).sum()) / float(valid.sum())
        assert 0.01 < bad <= 0.5, f"flags {flags}: {bad:.3f} of the valid pixels non-finite"


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

    def call_image(rgb=ptr(b["rgb"]), aov=None, w=8, h=6, p=good, out=ptr(b["out"]), out8=ptr(b["out8"]), device=0):
        return shim.rt_hip_denoise_image(rgb, C.byref(aov if aov is not None else _aov(b)), w, h,
                                         C.byref(p) if p is not None else None, device, out, out8)

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
    # the image form checks its arguments before it looks its device up (99: there is none such)
    assert call_image(w=0, device=99) == abi.EINVAL and call_image(out=None, out8=None, device=99) == abi.EINVAL
    assert call_image(device=99) == abi.ENODEV
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

"""The guided upsampling's contract (include/rt_hip.h, rt_hip_upsample) restated in numpy: vectorised over the pixels of the high
frame, sequential over the four taps in the contract's order, fp64 +, -, *, /, floor in the written order (numpy's float64
arithmetic is IEEE and never fuses), every stored value rounded to float32.  A skipped tap is not added (np.where keeps the old
sum).  scalar_upsample is the same contract pixel by pixel on Python floats.  edge_case builds the inputs both are compared on, and
the GPU against them: two samplings of one synthetic view, with the values of PLANTED put into random pixels."""
import math

import numpy as np

from reproject_expected import DBL_MAX, DENORM_MIN, FLT_MAX, _div, f32, same_bits, same_floats, tonemap8  # noqa: F401 (re-exported)

EPS = 2.0 ** -10
DEFAULTS = dict(sigma_depth=0.05, normal_power_log2=3, demodulate=True, object_edges=False)
# what became of a tap that is inside with wt > 0 (one of these), and of a pixel (guided / fallback / no_usable)
TAP_COUNTS = ("accepted", "nonfinite", "hits", "object", "normal", "depth")
PIXEL_COUNTS = ("guided", "fallback", "no_usable")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def demodulated(rgb, aov, demodulate):
    """step 2's e_q of every pixel of a frame: float(c / (albedo + eps)) or c"""
    c = _f32(rgb)
    if not demodulate:
        return c
    with np.errstate(all="ignore"):
        return (c.astype(np.float64) / (_f32(aov["albedo"]).astype(np.float64) + EPS)).astype(np.float32)


def upsample(low_rgb, low_aov, aov, sigma_depth=0.05, normal_power_log2=3, demodulate=True, object_edges=False, guided=True, info=None):
    """low_rgb float32 [hl,wl,3]; low_aov, aov: dicts with normal float32 [.,.,3], depth float32, hits uint32 (albedo float32
    [.,.,3] with demodulate, object uint32 with object_edges) at the low and at the high size -> dict(rgb float32 [h,w,3], conf
    float32 [h,w]).  guided=False: g = 1 for every usable tap, i.e. plain bilinear.  info: a dict that receives the counts of
    TAP_COUNTS (taps) and PIXEL_COUNTS (pixels)"""
    e_low = demodulated(low_rgb, low_aov, demodulate)
    hl, wl = e_low.shape[:2]
    h, w = np.asarray(aov["depth"]).shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        fx = ((xs.astype(np.float64) + 0.5) * (float(wl) - 1.0)) / (float(w) - 1.0) - 0.5          # 1.
        fy = ((ys.astype(np.float64) + 0.5) * (float(hl) - 1.0)) / (float(h) - 1.0) - 0.5
        x0d, y0d = np.floor(fx), np.floor(fy)
        a, b = fx - x0d, fy - y0d
        x0, y0 = x0d.astype(np.int64), y0d.astype(np.int64)
        n_p = _f32(aov["normal"]).astype(np.float64)
        z_p = _f32(aov["depth"]).astype(np.float64)
        bg_p = np.asarray(aov["hits"], np.uint32) == 0
        ln, lz = _f32(low_aov["normal"]).astype(np.float64), _f32(low_aov["depth"]).astype(np.float64)
        lh = np.asarray(low_aov["hits"], np.uint32)
        D = sigma_depth * z_p
        Zn_p = D * D
        W, A = np.zeros((h, w)), np.zeros((h, w, 3))
        U, A2 = np.zeros((h, w)), np.zeros((h, w, 3))
        any_usable = np.zeros((h, w), bool)
        count = dict.fromkeys(TAP_COUNTS, 0)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j                                                            # 2.
                inside = (qx >= 0) & (qx < wl) & (qy >= 0) & (qy < hl)
                qxc, qyc = np.clip(qx, 0, wl - 1), np.clip(qy, 0, hl - 1)
                wt = (a if i else 1.0 - a) * (b if j else 1.0 - b)
                eq = e_low[qyc, qxc]
                live = inside & (wt > 0)
                usable = live & np.isfinite(eq).all(axis=2)
                bg_q = lh[qyc, qxc] == 0                                                           # 3.
                d = _dot(n_p, ln[qyc, qxc])
                d = np.where(d > 0, d, 0.0)
                wn = d
                for _ in range(normal_power_log2):
                    wn = wn * wn
                Zn = Zn_p
                dz = lz[qyc, qxc] - z_p
                Zd = Zn + dz * dz
                zero = Zd == 0
                Zn, Zd = np.where(zero, 1.0, Zn), np.where(zero, 1.0, Zd)
                g = (wn * Zn) / Zd
                surface = ~bg_p & ~bg_q
                other = np.zeros((h, w), bool)
                if object_edges:
                    other = surface & (np.asarray(low_aov["object"], np.uint32)[qyc, qxc] != np.asarray(aov["object"], np.uint32))
                    g = np.where(other, 0.0, g)
                g = np.where(bg_p != bg_q, 0.0, g)
                g = np.where(bg_p & bg_q, 1.0, g)
                if not guided:
                    g = np.ones((h, w))
                om = wt * g
                take = usable & (om > 0) & (om < np.inf)
                eq64 = eq.astype(np.float64)
                any_usable |= usable
                U = np.where(usable, U + wt, U)
                A2 = np.where(usable[..., None], A2 + wt[..., None] * eq64, A2)
                W = np.where(take, W + om, W)
                A = np.where(take[..., None], A + om[..., None] * eq64, A)
                if guided:
                    lost = usable & ~take
                    same = lost & surface & ~other
                    count["accepted"] += int(take.sum())
                    count["nonfinite"] += int((live & ~usable).sum())
                    count["hits"] += int((lost & (bg_p != bg_q)).sum())
                    count["object"] += int((lost & other).sum())
                    count["normal"] += int((same & ~(wn > 0)).sum())
                    count["depth"] += int((same & (wn > 0)).sum())
        is_guided = W > 0                                                                          # 4.
        den = np.where(is_guided, W, U)
        e = (np.where(is_guided[..., None], A, A2) / den[..., None]).astype(np.float32)
        conf = np.where(is_guided, (W / U).astype(np.float32), np.float32(0.0)).astype(np.float32)
        none = ~is_guided & ~any_usable
        e[none] = 0.0
        conf[none] = -1.0
        out = e                                                                                    # 5.
        if demodulate:
            out = (e.astype(np.float64) * (_f32(aov["albedo"]).astype(np.float64) + EPS)).astype(np.float32)
    if info is not None:
        info.update(count, guided=int(is_guided.sum()), fallback=int((~is_guided & any_usable).sum()), no_usable=int(none.sum()))
    return dict(rgb=out, conf=conf)


# ---- the same, pixel by pixel from the contract's text -----------------------------------------------------------------------

def scalar_upsample(low_rgb, low_aov, aov, sigma_depth=0.05, normal_power_log2=3, demodulate=True, object_edges=False):
    low_rgb = _f32(low_rgb)
    hl, wl = low_rgb.shape[:2]
    h, w = np.asarray(aov["depth"]).shape
    out = np.zeros((h, w, 3), np.float32)
    conf = np.zeros((h, w), np.float32)
    inf = math.inf
    for y in range(h):
        for x in range(w):
            # 1.
            fx = _div((x + 0.5) * (wl - 1.0), w - 1.0) - 0.5
            fy = _div((y + 0.5) * (hl - 1.0), h - 1.0) - 0.5
            x0, y0 = math.floor(fx), math.floor(fy)
            a, b = fx - x0, fy - y0
            n_p = [float(t) for t in aov["normal"][y, x]]
            z_p = float(aov["depth"][y, x])
            W, U = 0.0, 0.0
            A, A2 = [0.0] * 3, [0.0] * 3
            usable_taps = 0
            for j in (0, 1):
                for i in (0, 1):
                    # 2.
                    qx, qy = x0 + i, y0 + j
                    wt = (a if i else 1.0 - a) * (b if j else 1.0 - b)
                    if qx < 0 or qx >= wl or qy < 0 or qy >= hl or not wt > 0:
                        continue
                    if demodulate:
                        e = [f32(_div(float(low_rgb[qy, qx, k]), float(low_aov["albedo"][qy, qx, k]) + EPS)) for k in range(3)]
                    else:
                        e = [float(low_rgb[qy, qx, k]) for k in range(3)]
                    if not all(math.isfinite(t) for t in e):
                        continue
                    usable_taps += 1
                    U += wt
                    for k in range(3):
                        A2[k] += wt * e[k]
                    # 3.
                    hp, hq = int(aov["hits"][y, x]), int(low_aov["hits"][qy, qx])
                    if hp == 0 and hq == 0:
                        g = 1.0
                    elif hp == 0 or hq == 0:
                        g = 0.0
                    elif object_edges and int(low_aov["object"][qy, qx]) != int(aov["object"][y, x]):
                        g = 0.0
                    else:
                        n_q = [float(t) for t in low_aov["normal"][qy, qx]]
                        d = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
                        d = d if d > 0 else 0.0
                        wn = d
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        D = sigma_depth * z_p
                        Zn = D * D
                        dz = float(low_aov["depth"][qy, qx]) - z_p
                        Zd = Zn + dz * dz
                        if Zd == 0:
                            Zn = Zd = 1.0
                        g = _div(wn * Zn, Zd)
                    om = wt * g
                    if not (om > 0 and om < inf):
                        continue
                    W += om
                    for k in range(3):
                        A[k] += om * e[k]
            # 4.
            if W > 0:
                e = [f32(_div(A[k], W)) for k in range(3)]
                c = f32(_div(W, U))
            elif usable_taps:
                e = [f32(_div(A2[k], U)) for k in range(3)]
                c = 0.0
            else:
                e = [0.0] * 3
                c = -1.0
            # 5.
            for k in range(3):
                out[y, x, k] = np.float32(e[k] * (float(aov["albedo"][y, x, k]) + EPS)) if demodulate else np.float32(e[k])
            conf[y, x] = c
    return dict(rgb=out, conf=conf)


def mismatch(got, exp):
    """'' when rgb (NaN equal to NaN) and conf (bit for bit) are equal, else which differ and in how many words"""
    msgs = []
    for f, same in (("rgb", same_floats), ("conf", same_bits)):
        if not same(got[f], exp[f]):
            g, e = _f32(got[f]), _f32(exp[f])
            bad = np.argwhere((g.view(np.uint32) != e.view(np.uint32)) & ~(np.isnan(g) & np.isnan(e))) if g.shape == e.shape else []
            first = tuple(bad[0]) if len(bad) else None
            msgs.append(f"{f}: {len(bad)} words differ, first at {first}: got {g[first]!r} expected {e[first]!r}" if first else f"{f}: shape")
    return "; ".join(msgs)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

# ((w, h), (wl, hl)): the trivial frame, odd and even ratios near 2, 3 and 1.5, a column, and downsampling
SIZE_PAIRS = [((2, 2), (2, 2)), ((17, 15), (9, 8)), ((16, 16), (8, 8)), ((33, 31), (16, 16)), ((31, 33), (11, 11)), ((40, 30), (27, 20)),
              ((2, 40), (2, 13)), ((16, 16), (33, 31))]
# (sigma_depth, k, demodulate, object_edges): the defaults, k = 0 and k = 10, sigma_depth 2^-40 and DBL_MAX (Zn overflows: every
# surface tap is rejected and the fallback carries the frame)
PARAMS = ((0.05, 3, True, False), (0.05, 0, False, True), (1.0, 10, True, True), (2.0 ** -40, 3, False, False), (DBL_MAX, 3, True, False))
VALUES = ("flt_max", "neg_flt_max", "denormal", "neg_zero", "nan", "inf")
PLANTED = tuple(f"low_rgb_{v}" for v in VALUES) + tuple(f"low_albedo_{v}" for v in VALUES + ("neg_eps",)) + \
    tuple(f"albedo_{v}" for v in VALUES + ("neg_eps",)) + \
    ("low_normal_nan", "low_normal_zero", "normal_nan", "normal_zero", "low_depth_zero", "low_depth_negative", "low_depth_inf",
     "low_depth_nan", "depth_zero", "depth_negative", "depth_inf", "depth_nan", "low_miss_with_depth", "miss_with_depth",
     "low_object", "object")
_NORMALS = np.array([(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, 0.8, 0.0), (0.0, 0.6, 0.8), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0)])


def params(k):
    sd, kk, dm, oe = PARAMS[k]
    return dict(sigma_depth=sd, normal_power_log2=kk, demodulate=dm, object_edges=oe)


def pair_id(pair):
    (w, h), (wl, hl) = pair
    return f"{w}x{h}from{wl}x{hl}"


def case_seed(pair):
    (w, h), (wl, hl) = pair
    return ((w * 64 + h) * 64 + wl) * 64 + hl


def view(w, h, rng_albedo):
    """first-hit buffers of one synthetic view sampled at the centres of a w x h grid, (x + 0.5) / (w - 1) as get_camera_ray maps
    them: a 3 x 2 patchwork of objects (normals of _NORMALS, flat or sloping depths) with the background beyond u + v > 1.6"""
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = (xs + 0.5) / (w - 1.0), (ys + 0.5) / (h - 1.0)
    obj = (np.minimum(np.floor(u * 3), 2) + 3 * np.minimum(np.floor(v * 2), 1)).astype(np.int64)
    hit = u + v <= 1.6
    depth = np.where(obj % 2 == 0, 4.0 + obj, 4.0 + obj + 3.0 * u + 0.5 * v)       # even objects are flat: dz == 0 between taps
    albedo = (0.05 + 0.9 * rng_albedo.random((h, w, 3))).astype(np.float32)
    albedo[~hit] = (0.3, 0.5, 0.9)
    return dict(albedo=albedo, normal=np.where(hit[..., None], _NORMALS[obj], 0.0).astype(np.float32),
                depth=np.where(hit, depth, np.inf).astype(np.float32), hits=np.where(hit, 4, 0).astype(np.uint32),
                object=np.where(hit, obj, 0xFFFFFFFF).astype(np.uint32))


def _value(name, k):
    return dict(flt_max=FLT_MAX, neg_flt_max=-FLT_MAX, denormal=DENORM_MIN * (1 + k % 7), neg_zero=-0.0, nan=np.nan,
                inf=[np.inf, -np.inf][k % 2], neg_eps=-EPS)[name]


def edge_case(pair, seed, share=0.4):
    """-> low_rgb, low_aov, aov, planted: category -> how many.  The two samplings of view(), ordinary colours, `share` of the
    pixels of each frame planted with the PLANTED values in turn, and (where the low frame has room) a block of 4 x 4 low pixels
    with a non-finite colour: the high pixels whose four taps lie in it have no usable tap"""
    (w, h), (wl, hl) = pair
    rng = np.random.default_rng(seed)
    aov, low_aov = view(w, h, rng), view(wl, hl, rng)
    low_rgb = (rng.random((hl, wl, 3)) * rng.choice([0.1, 1.0, 30.0], (hl, wl, 1))).astype(np.float32)
    planted = dict.fromkeys(PLANTED, 0)
    k = 0
    for low, (fw, fh) in ((True, (wl, hl)), (False, (w, h))):
        cats = [c for c in PLANTED if c.startswith("low_") == low]
        bufs = low_aov if low else aov
        for p in rng.permutation(fw * fh)[: int(share * fw * fh)]:
            cat = cats[k % len(cats)]
            k += 1
            planted[cat] += 1
            y, x = divmod(int(p), fw)
            ch = int(rng.integers(0, 3))
            name = cat[4:] if low else cat
            if name.startswith("rgb_"):
                low_rgb[y, x, ch] = _value(name[4:], k)
            elif name.startswith("albedo_"):
                bufs["albedo"][y, x, ch] = _value(name[7:], k)
            elif name == "normal_nan":
                bufs["normal"][y, x, ch] = np.nan
            elif name == "normal_zero":
                bufs["normal"][y, x] = 0
            elif name == "depth_zero":
                bufs["depth"][y, x] = 0
            elif name == "depth_negative":
                bufs["depth"][y, x] = -3.5
            elif name == "depth_inf":
                bufs["depth"][y, x], bufs["hits"][y, x] = np.inf, 3
            elif name == "depth_nan":
                bufs["depth"][y, x], bufs["hits"][y, x] = np.nan, 2
            elif name == "miss_with_depth":
                bufs["hits"][y, x], bufs["depth"][y, x] = 0, np.float32(3.25)
            elif name == "object":
                bufs["object"][y, x] = 77
            else:
                raise ValueError(cat)
    if wl >= 8 and hl >= 8:
        bx, by = int(rng.integers(0, wl - 3)), int(rng.integers(0, hl - 3))
        low_rgb[by:by + 4, bx:bx + 4, 1] = np.nan
    return low_rgb, low_aov, aov, planted


def clip_rms(a, b):
    """clipped linear RMS, the quality measure of the tools and tests"""
    clip = lambda x: np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=1.0), 0, 1)
    return float(np.sqrt(((clip(a) - clip(b)) ** 2).mean()))
